#!/usr/bin/env python3
"""Device time of the policy head (include/ccx.h CCX_MLP: Linear(L, 64) -> Tanh -> Linear(64, 5)) from replayed HIP graphs, in
ONE process on ONE build so that every variant sees the same machine.  Per shape:

  mlp_forward            ccx_mlp_forward alone: rows -> logits, one kernel
  mlp_sample_actions     ccx_mlp_sample_actions: rows -> actions, logp, one kernel
  forward + sample       ccx_mlp_forward, then ccx_sample_actions: two kernels
  (a) torch + sample     THE YARDSTICK: a captured torch.nn.Sequential of the same sizes (hipBLASLt's kernels and the tanh),
                         then ccx_sample_actions
  step                   a plain one-step launch of the env (C2 / C3 shapes only): what the actor loop alternates with

The protocol of evaluate_timing.py: a graph holds CALLS calls; a repeat replays it REPLAYS times between two synchronisations;
the variants alternate over 15 repeats; the median is reported with min .. max.

    python profiles/mlp_timing.py [--out profiles/mlp_timing.txt]
"""

import argparse
import statistics
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
REPEATS = 15
H = 64
# label, workload, envs, calls per graph, replays per repeat
SHAPES = [("C2 4096 x 8", "c2", 4096, 20, 10), ("C3 4096 x 32", "c3", 4096, 10, 10), ("C2 64 x 8", "c2", 64, 20, 10)]
FLAT_ROWS, FLAT_L = 524288, 38


def time_graphs(torch, side, bodies, calls, replays):
    graphs = {}
    for name, body in bodies.items():
        body()                                                      # warm-up: code objects, allocator blocks
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
        for name, g in graphs.items():                              # alternate the variants
            side.synchronize()
            t0 = time.perf_counter()
            for _ in range(replays):
                g.replay()
            side.synchronize()
            times[name].append((time.perf_counter() - t0) / (replays * calls) * 1e6)
    graphs.clear()
    return times


def measure_env(cfg, E, calls, replays):
    import torch

    from collectivecrossing_amd import BatchedCollectiveCrossing

    env = BatchedCollectiveCrossing(cfg, E)
    env.make_reset_pool(seed0=0, size=4096)
    env.reset_from_pool()
    N = env.num_agents
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        env.use_stream(side)
        torch.manual_seed(0)
        head = env.mlp_head(H)
        seq = head.to_sequential()
        obs, masks = env.observe(), env.action_masks()
        logits = torch.empty((E, N, 5), device=env.device)
        out = env.alloc_sample(want_logp=True)
        actions = torch.zeros((1, E, N), dtype=torch.uint8, device=env.device)
        step_out = env.alloc_rollout(1)
        held = {}

        def torch_sample():
            with torch.no_grad():
                held["l"] = seq(obs)
            env.sample_actions(held["l"], masks, out=out)

        def forward():
            with torch.no_grad():
                head(obs, out=logits)

        def forward_sample():
            forward()
            env.sample_actions(logits, masks, out=out)

        bodies = {"mlp_forward": forward, "mlp_sample_actions": lambda: env.mlp_sample_actions(head, obs, masks, out=out),
                  "forward + sample": forward_sample, "torch + sample": torch_sample,
                  "step": lambda: env.rollout(actions, out=step_out)}
        forward()
        with torch.no_grad():
            err = (seq(obs) - logits).abs().max().item()            # the yardstick computes the same logits (to rounding)
        assert err <= 1e-4, err
        times = time_graphs(torch, side, bodies, calls, replays)
        held.clear()
    env.use_stream(None)
    env.close()
    return times, E * N


def measure_flat(cfg, rows, L, calls, replays):
    """rows of L floats that belong to no env: the forward against the torch module (nothing to sample for)."""
    import torch

    from collectivecrossing_amd import BatchedCollectiveCrossing

    env = BatchedCollectiveCrossing(cfg, 64)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        env.use_stream(side)
        torch.manual_seed(0)
        head = env.mlp_head(H, L=L)
        seq = head.to_sequential()
        x = torch.randint(0, 13, (rows, L), device=env.device).float()
        y = torch.empty((rows, 5), device=env.device)
        held = {}

        def forward():
            with torch.no_grad():
                head(x, out=y)

        def torch_forward():
            with torch.no_grad():
                held["l"] = seq(x)

        times = time_graphs(torch, side, {"mlp_forward": forward, "torch + sample": torch_forward}, calls, replays)
        held.clear()
    env.use_stream(None)
    env.close()
    return times, rows


def cell(v):
    return "-" if v is None else f"{statistics.median(v):.1f} ({min(v):.1f} .. {max(v):.1f})"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", type=Path, default=ROOT / "profiles" / "mlp_timing.txt")
    args = ap.parse_args()
    sys.path.insert(0, str(ROOT))
    import bench
    import torch

    assert torch.cuda.is_available(), "this is a measurement on the GPU"
    lines = [f"# {torch.cuda.get_device_name(0)}; us per call, median of {REPEATS} alternating repeats (min .. max); a repeat = replays of a "
             f"graph of several calls between two synchronisations",
             f"# the head: Linear(L, {H}) -> Tanh -> Linear({H}, 5); mlp_forward: ccx_mlp_forward; mlp_sample_actions: rows -> actions and logp",
             "# in one kernel; forward + sample: ccx_mlp_forward, then ccx_sample_actions; (a) the captured torch.nn.Sequential of the same",
             "# sizes, then ccx_sample_actions: the yardstick (in the last row, where no env is behind the rows: the Sequential alone",
             "# against mlp_forward alone); step: one plain env step"]
    cols = ("mlp_forward", "mlp_sample_actions", "forward + sample", "torch + sample", "step")
    names = {"torch + sample": "(a) torch + sample"}
    lines.append(f"{'shape':<16}{'rows':>9}" + "".join(f"{names.get(c, c):>27}" for c in cols) + f"{'fused/(a)':>11}")
    print("\n".join(lines), flush=True)
    for label, workload, E, calls, replays in SHAPES:
        cfg, _ = bench.workload_config(workload)
        t, rows = measure_env(cfg, E, calls, replays)
        med = {k: statistics.median(v) for k, v in t.items()}
        row = f"{label:<16}{rows:>9}" + "".join(f"{cell(t.get(c)):>27}" for c in cols) + f"{med['mlp_sample_actions'] / med['torch + sample']:>11.3f}"
        lines.append(row)
        print(row, flush=True)
    cfg, _ = bench.workload_config("c2")
    t, rows = measure_flat(cfg, FLAT_ROWS, FLAT_L, 5, 10)
    med = {k: statistics.median(v) for k, v in t.items()}
    row = f"{'rows of 38':<16}{rows:>9}" + "".join(f"{cell(t.get(c)):>27}" for c in cols) + f"{med['mlp_forward'] / med['torch + sample']:>11.3f}"
    lines.append(row)
    print(row, flush=True)
    args.out.parent.mkdir(parents=True, exist_ok=True)
    args.out.write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
