#!/usr/bin/env python3
"""Device time of the policy head's backward pass (include/ccx.h CCX_MLP, backward: Linear(L, 64) -> Tanh -> Linear(64, 5)) from
replayed HIP graphs, in ONE process on ONE build so that every variant sees the same machine.  Per shape:

  mlp_backward           ccx_mlp_backward on static buffers: two kernels, the four parameter gradients by the written rule
  autograd device        the same through autograd: torch.autograd.grad over a head with backward="device"
  (a) autograd torch     THE YARDSTICK: what the head ran before and still runs by default, backward="torch" -- five f32 matrix
                         products and sums of hipBLASLt and torch on the saved activations

The protocol of mlp_timing.py: a graph holds CALLS calls; a repeat replays it REPLAYS times between two synchronisations; the
variants alternate over 15 repeats; the median is reported with min .. max.

    python profiles/mlp_backward_timing.py [--out profiles/mlp_backward_timing.txt]
"""

import argparse
import statistics
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "profiles"))
H, O = 64, 5
# rows, L, calls per graph, replays per repeat
SHAPES = [(512, 38, 20, 10), (32768, 38, 10, 10), (131072, 38, 5, 10), (524288, 38, 3, 5), (131072, 134, 3, 5)]


def measure(cfg, rows, L, calls, replays):
    import torch
    from mlp_timing import time_graphs

    from collectivecrossing_amd import BatchedCollectiveCrossing

    env = BatchedCollectiveCrossing(cfg, 64)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        env.use_stream(side)
        heads = {}
        for mode in ("device", "torch"):
            torch.manual_seed(0)
            heads[mode] = env.mlp_head(H, O, L=L, backward=mode)
        x = torch.randint(0, 13, (rows, L), device=env.device).float()
        gy = torch.randn((rows, O), device=env.device) / rows
        hidden = torch.empty((rows, H), device=env.device)
        with torch.no_grad():
            heads["device"](x, hidden_out=hidden)
        out = env.alloc_mlp_backward(heads["device"], (rows,))
        ys = {mode: head(x) for mode, head in heads.items()}          # the autograd graphs the two yardstick bodies walk
        held = {}

        def through_autograd(mode):
            def body():
                held[mode] = torch.autograd.grad(ys[mode], list(heads[mode].parameters()), gy, retain_graph=True)
            return body

        bodies = {"mlp_backward": lambda: env.mlp_backward(heads["device"], x, hidden, gy, out=out),
                  "autograd device": through_autograd("device"), "autograd torch": through_autograd("torch")}
        for body in bodies.values():
            body()
        side.synchronize()
        for a, b, c in zip(held["device"], held["torch"], (out.w1t, out.b1, out.w2, out.b2)):   # the same gradients
            assert torch.equal(a, c), "autograd device = mlp_backward, bit for bit"
            assert float((a - b).abs().max()) <= 1e-4 * max(1.0, float(b.abs().max())), float((a - b).abs().max())
        times = time_graphs(torch, side, bodies, calls, replays)
        held.clear()
        ys.clear()
    env.use_stream(None)
    env.close()
    return times


def cell(v):
    return f"{statistics.median(v):.1f} ({min(v):.1f} .. {max(v):.1f})"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", type=Path, default=ROOT / "profiles" / "mlp_backward_timing.txt")
    args = ap.parse_args()
    sys.path.insert(0, str(ROOT))
    import bench
    import torch

    assert torch.cuda.is_available(), "this is a measurement on the GPU"
    lines = [f"# {torch.cuda.get_device_name(0)}; us per call, median of 15 alternating repeats (min .. max); a repeat = replays of a graph",
             "# of several calls between two synchronisations",
             f"# the head: Linear(L, {H}) -> Tanh -> Linear({H}, {O}); mlp_backward: ccx_mlp_backward on static buffers (two kernels);",
             "# autograd device / (a) autograd torch: torch.autograd.grad of the four parameters through backward=\"device\" / \"torch\"",
             "# (the torch composition on the saved activations: the yardstick)"]
    cols = ("mlp_backward", "autograd device", "autograd torch")
    names = {"autograd torch": "(a) autograd torch"}
    lines.append(f"{'rows':>9}{'L':>5}" + "".join(f"{names.get(c, c):>27}" for c in cols) + f"{'backward/(a)':>14}{'device/(a)':>12}")
    print("\n".join(lines), flush=True)
    cfg, _ = bench.workload_config("c2")
    for rows, L, calls, replays in SHAPES:
        t = measure(cfg, rows, L, calls, replays)
        med = {k: statistics.median(v) for k, v in t.items()}
        row = (f"{rows:>9}{L:>5}" + "".join(f"{cell(t[c]):>27}" for c in cols)
               + f"{med['mlp_backward'] / med['autograd torch']:>14.3f}{med['autograd device'] / med['autograd torch']:>12.3f}")
        lines.append(row)
        print(row, flush=True)
    args.out.parent.mkdir(parents=True, exist_ok=True)
    args.out.write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
