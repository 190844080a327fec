#!/usr/bin/env python3
"""Device time of `ccx_sample_actions` (masked categorical sampling with log-probs, include/ccx.h CCX_SAMPLE) from replayed
HIP graphs, in ONE process so that every variant sees the same machine.  Per shape:

  sample                  the kernel with masks and logp (what a PPO actor loop calls)
  no mask / no logp /     the kernel without masks; without logp (actions only); with logp and entropy; the masked argmax
  + entropy / argmax      with logp
  (a) gumbel graph        the composition of examples/masked_policy.py captured: unpack_action_masks -> masked_fill ->
                          exponential_ -> log -> subtract -> argmax -> cast, plus log_softmax + gather for the log-prob
  (b) categorical graph   torch.distributions.Categorical(logits=masked).sample() + log_prob, captured (validate_args off:
                          the validation synchronises the host)
  (c) step                one `step` of the same batch (full outputs): the launch the sampling sits next to

The protocol of gae_timing.py: a graph holds CALLS calls; a repeat replays it REPLAYS times between two synchronisations;
the variants alternate over 15 repeats; the median is reported with min .. max.  Logits are random, the masks those of a
reset state.

    python profiles/sample_timing.py [--out profiles/sample_timing.txt]
"""

import argparse
import statistics
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
REPEATS = 15
# label, workload, E, calls per graph, replays per repeat
SHAPES = [("C2", "c2", 4096, 20, 10), ("C3", "c3", 4096, 20, 10), ("C5-64", "c5_64", 1024, 20, 10)]


def measure(wl, E, calls, replays):
    import bench
    import torch

    from collectivecrossing_amd import BatchedCollectiveCrossing, unpack_action_masks
    cfg, _ = bench.workload_config(wl)
    side = torch.cuda.Stream()
    graphs = {}
    with torch.cuda.stream(side):
        env = BatchedCollectiveCrossing(cfg, E)
        env.use_stream(side)
        env.make_reset_pool(0, 1024)
        env.reset_from_pool()
        N = env.num_agents
        masks = env.action_masks()
        logits = torch.randn((E, N, 5), device=env.device) * 3.0
        full, lite, both = env.alloc_sample(True, False), env.alloc_sample(False, False), env.alloc_sample(True, True)
        noise = torch.empty((E, N, 5), device=env.device)
        t_actions = torch.empty((E, N), dtype=torch.uint8, device=env.device)
        t_logp = torch.empty((E, N), device=env.device)
        step_actions = torch.randint(0, 5, (E, N), dtype=torch.uint8, device=env.device)

        def gumbel():
            legal = unpack_action_masks(masks)
            masked = logits.masked_fill(~legal, float("-inf"))
            noise.exponential_()
            a = (masked - noise.log()).argmax(-1)
            t_actions.copy_(a.to(torch.uint8))
            t_logp.copy_(torch.log_softmax(masked, -1).gather(-1, a.unsqueeze(-1)).squeeze(-1))

        def categorical():
            legal = unpack_action_masks(masks)
            dist = torch.distributions.Categorical(logits=logits.masked_fill(~legal, float("-inf")), validate_args=False)
            a = dist.sample()
            t_actions.copy_(a.to(torch.uint8))
            t_logp.copy_(dist.log_prob(a))

        bodies = {
            "sample": lambda: env.sample_actions(logits, masks, out=full),
            "no mask": lambda: env.sample_actions(logits, None, out=full),
            "no logp": lambda: env.sample_actions(logits, masks, out=lite),
            "+ entropy": lambda: env.sample_actions(logits, masks, out=both),
            "argmax": lambda: env.sample_actions(logits, masks, deterministic=True, out=full),
            "gumbel graph": gumbel,
            "categorical graph": categorical,
            "step": lambda: env.step(step_actions),
        }
        for name, body in bodies.items():
            body()                                                  # warm-up: code objects, allocator blocks
            side.synchronize()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, stream=side):
                for _ in range(calls):
                    body()
            for _ in range(2):
                g.replay()
            side.synchronize()
            graphs[name] = g
        times = {k: [] for k in graphs}
        for _ in range(REPEATS):
            for name, g in graphs.items():                          # alternate the variants
                side.synchronize()
                t0 = time.perf_counter()
                for _ in range(replays):
                    g.replay()
                side.synchronize()
                times[name].append((time.perf_counter() - t0) / (replays * calls) * 1e6)
        # the torch compositions sample from the same distribution: a wrong yardstick would be no yardstick
        env.reset_from_pool()                   # the step variant ran every episode to its end: a dead slot's 255 is no index to gather with
        gumbel()
        bodies["sample"]()
        side.synchronize()
        legal = unpack_action_masks(masks)
        assert bool(legal.gather(-1, t_actions.long().unsqueeze(-1)).all()) and bool(legal.gather(-1, full.actions.long().unsqueeze(-1)).all())
        want = torch.log_softmax(logits.masked_fill(~legal, float("-inf")), -1).gather(-1, full.actions.long().unsqueeze(-1)).squeeze(-1)
        assert float((want - full.logp).abs().max()) < 1e-5
    env.close()
    return times, N


def cell(v):
    return f"{statistics.median(v):.2f} ({min(v):.2f} .. {max(v):.2f})"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", type=Path, default=ROOT / "profiles" / "sample_timing.txt")
    args = ap.parse_args()
    sys.path.insert(0, str(ROOT))
    import torch

    assert torch.cuda.is_available(), "this is a measurement on the GPU"
    cols = ("sample", "no mask", "no logp", "+ entropy", "argmax", "gumbel graph", "categorical graph", "step")
    names = {"gumbel graph": "(a) gumbel graph", "categorical graph": "(b) categorical graph", "step": "(c) step"}
    lines = [f"# {torch.cuda.get_device_name(0)}; us per call, median of {REPEATS} alternating repeats (min .. max); a repeat = replays of a "
             f"graph of several calls between two synchronisations",
             "# sample: ccx_sample_actions with masks and logp; no mask / no logp / + entropy / argmax: its variants; (a) the Gumbel-max",
             "# composition of examples/masked_policy.py plus log_softmax + gather, captured; (b) Categorical.sample + log_prob, captured;",
             "# (c) one step of the same batch with full outputs",
             f"{'shape':<8}{'E x N':>10}" + "".join(f"{names.get(c, c):>24}" for c in cols) + f"{'sample/(a)':>12}{'sample/(b)':>12}{'sample/(c)':>12}"]
    print("\n".join(lines), flush=True)
    for label, wl, E, calls, replays in SHAPES:
        t, N = measure(wl, E, calls, replays)
        med = {k: statistics.median(v) for k, v in t.items()}
        row = f"{label:<8}{f'{E} x {N}':>10}" + "".join(f"{cell(t[c]):>24}" for c in cols)
        row += f"{med['sample'] / med['gumbel graph']:>12.3f}{med['sample'] / med['categorical graph']:>12.3f}{med['sample'] / med['step']:>12.3f}"
        lines.append(row)
        print(row, flush=True)
    args.out.parent.mkdir(parents=True, exist_ok=True)
    args.out.write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
