#!/usr/bin/env python3
"""Device time of `ccx_evaluate_actions` / `ccx_evaluate_actions_backward` (stored actions under new logits, include/ccx.h
CCX_EVALUATE) from replayed HIP graphs, in ONE process on ONE build so that every variant sees the same machine.  Per shape:

  fwd               the forward kernel with masks: logp and entropy
  fwd + bwd         forward, then the backward kernel with both incoming gradients
  fwd + bwd logp    forward without entropy, then the backward kernel with grad_logp alone
  (a) torch graph   THE YARDSTICK: the same quantities and their gradient as a user writes them with torch alone --
                    `masked_fill(-inf)`, `log_softmax`, `gather`, an entropy with the `p > 0` guard, `torch.autograd.grad`
                    with the same two incoming gradients -- captured and replayed
  (b) copy          `torch.Tensor.copy_` of as many bytes as fwd + bwd moves (reads + writes, half in, half out)

The protocol of gae_timing.py: a graph holds CALLS calls; a repeat replays it REPLAYS times between two synchronisations; the
variants alternate over 15 repeats; the median is reported with min .. max.

    python profiles/evaluate_timing.py [--out profiles/evaluate_timing.txt]
"""

import argparse
import statistics
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
REPEATS = 15
# label, rows, calls per graph, replays per repeat
SHAPES = [("4096 x 8 x 16", 4096 * 8 * 16, 10, 10), ("32768", 32768, 20, 10)]


def torch_composition(x, actions64, legal, glp, gent):
    import torch

    lp = torch.log_softmax(x.masked_fill(~legal, -torch.inf), -1)
    logp = lp.gather(-1, actions64[:, None])[:, 0]
    p = lp.exp()
    zero = torch.zeros_like(lp)
    entropy = -torch.where(p > 0, p * torch.where(p > 0, lp, zero), zero).sum(-1)
    grad, = torch.autograd.grad((logp, entropy), x, grad_outputs=(glp, gent))
    return logp, entropy, grad


def measure(env, M, calls, replays):
    import torch

    from collectivecrossing_amd import unpack_action_masks

    side = torch.cuda.Stream()
    graphs = {}
    dev = env.device
    with torch.cuda.stream(side):
        env.use_stream(side)
        gen = torch.Generator(device=dev).manual_seed(M)
        logits = torch.randn((M, 5), device=dev, generator=gen) * 3.0
        actions = torch.randint(0, 5, (M,), device=dev, generator=gen).to(torch.uint8)
        masks = torch.randint(0, 16, (M,), device=dev, generator=gen).to(torch.uint8) | 0x10
        masks |= torch.bitwise_left_shift(torch.ones_like(actions), actions)          # the stored action is legal
        glp, gent = torch.randn(M, device=dev, generator=gen), torch.randn(M, device=dev, generator=gen)
        legal = unpack_action_masks(masks)
        actions64 = actions.long()
        x = logits.clone().requires_grad_(True)
        out = env.alloc_evaluate((M,), want_entropy=True)
        out_lp = env.alloc_evaluate((M,), want_entropy=False)
        grad = torch.empty_like(logits)
        nbytes = M * ((20 + 1 + 1 + 4 + 4) + (20 + 1 + 1 + 4 + 4 + 20))              # fwd + bwd, reads + writes
        src = torch.empty(nbytes // 2, dtype=torch.uint8, device=dev)
        dst = torch.empty_like(src)

        def fwd():
            env.evaluate_actions(logits, actions, masks, out=out)

        def fwd_bwd():
            env.evaluate_actions(logits, actions, masks, out=out)
            env.evaluate_actions_backward(logits, actions, masks, glp, gent, out=grad)

        def fwd_bwd_logp():
            env.evaluate_actions(logits, actions, masks, out=out_lp)
            env.evaluate_actions_backward(logits, actions, masks, glp, None, out=grad)

        held = {}

        def torch_graph():
            held["t"] = torch_composition(x, actions64, legal, glp, gent)

        bodies = {"fwd": fwd, "fwd + bwd": fwd_bwd, "fwd + bwd logp": fwd_bwd_logp, "torch graph": torch_graph,
                  "copy": lambda: dst.copy_(src)}
        # the torch composition computes the same quantities (to rounding): a wrong yardstick would be no yardstick
        fwd_bwd()
        t_logp, t_entropy, t_grad = torch_composition(x, actions64, legal, glp, gent)
        side.synchronize()
        for a, b in ((t_logp, out.logp), (t_entropy, out.entropy), (t_grad, grad)):
            err = (a.detach() - b).abs().max().item()
            assert err <= 1e-4 * max(1.0, b.abs().max().item()), err
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
        graphs.clear()
        held.clear()
    env.use_stream(None)
    return times, nbytes


def cell(v):
    return f"{statistics.median(v):.1f} ({min(v):.1f} .. {max(v):.1f})"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", type=Path, default=ROOT / "profiles" / "evaluate_timing.txt")
    args = ap.parse_args()
    sys.path.insert(0, str(ROOT))
    import bench
    import torch

    from collectivecrossing_amd import BatchedCollectiveCrossing

    assert torch.cuda.is_available(), "this is a measurement on the GPU"
    cfg, _ = bench.workload_config("c2")
    env = BatchedCollectiveCrossing(cfg, 64)                        # the rule never reads env state: the batch supplies device and stream
    lines = [f"# {torch.cuda.get_device_name(0)}; us per call, median of {REPEATS} alternating repeats (min .. max); a repeat = replays of a "
             f"graph of several calls between two synchronisations",
             "# fwd: ccx_evaluate_actions with masks, logp and entropy; fwd + bwd: then ccx_evaluate_actions_backward with both gradients;",
             "# fwd + bwd logp: forward without entropy, backward with grad_logp alone; (a) the captured torch composition for the same",
             "# quantities and their gradient (masked_fill, log_softmax, gather, guarded entropy, autograd.grad): the yardstick; (b) a torch",
             "# copy of the bytes fwd + bwd moves (reads + writes)"]
    cols = ("fwd", "fwd + bwd", "fwd + bwd logp", "torch graph", "copy")
    names = {"torch graph": "(a) torch graph", "copy": "(b) copy"}
    head = f"{'rows':<16}{'MB moved':>10}" + "".join(f"{names.get(c, c):>28}" for c in cols) + f"{'fwd+bwd/(a)':>13}{'GB/s':>8}"
    lines.append(head)
    print("\n".join(lines), flush=True)
    for label, M, calls, replays in SHAPES:
        t, nbytes = measure(env, M, calls, replays)
        med = {k: statistics.median(v) for k, v in t.items()}
        row = f"{label:<16}{nbytes / 1e6:>10.1f}" + "".join(f"{cell(t[c]):>28}" for c in cols)
        row += f"{med['fwd + bwd'] / med['torch graph']:>13.4f}{nbytes / med['fwd + bwd'] / 1e3:>8.0f}"
        lines.append(row)
        print(row, flush=True)
    env.close()
    args.out.parent.mkdir(parents=True, exist_ok=True)
    args.out.write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
