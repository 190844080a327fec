#!/usr/bin/env python3
"""Device time of the optimiser step (include/ccx.h CCX_ADAM: global-norm clipping + Adam) from replayed HIP graphs, in ONE
process on ONE build so that every variant sees the same machine.  Per parameter set:

  adam_step              ccx_adam_step without clipping (max_grad_norm = 0): three launches, the norm still computed
  adam_step clip         ccx_adam_step with max_grad_norm = 0.5
  (a) torch foreach      THE YARDSTICK: torch.nn.utils.clip_grad_norm_(0.5, foreach=True) followed by
                         torch.optim.Adam(capturable=True, foreach=True).step(), captured
  (b) torch fused        the same with Adam(capturable=True, fused=True), where this torch offers it

The protocol of mlp_backward_timing.py: a graph holds CALLS calls; a repeat replays it REPLAYS times between two
synchronisations; the variants alternate over 15 repeats; the median is reported with min .. max.  Measured, not gated: the
value of the device step is its written rule and the single graph, not a speed-up.

    python profiles/adam_timing.py [--out profiles/adam_timing.txt]
"""

import argparse
import statistics
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "profiles"))
# name, tensor shapes, calls per graph, replays per repeat
SETS = [("actor + critic, L = 38, H = 64", [(38, 64), (64,), (5, 64), (5,), (38, 64), (64,), (1, 64), (1,)], 20, 10),
        ("one head, L = 512, H = 256, O = 8", [(512, 256), (256,), (8, 256), (8,)], 20, 10)]
COLS = ("adam_step", "adam_step clip", "(a) torch foreach", "(b) torch fused")


def measure(cfg, shapes, calls, replays):
    import torch
    from mlp_timing import time_graphs

    from collectivecrossing_amd import BatchedCollectiveCrossing

    env = BatchedCollectiveCrossing(cfg, 64)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        env.use_stream(side)
        torch.manual_seed(0)
        start = [torch.randn(s, device=env.device) * 0.3 for s in shapes]
        grads = [torch.randn(s, device=env.device) * 0.02 for s in shapes]
        bodies = {}
        ours = {}
        for name, mgn in (("adam_step", 0.0), ("adam_step clip", 0.5)):
            ours[name] = env.adam([p.clone() for p in start], lr=3e-4, max_grad_norm=mgn)
            bodies[name] = lambda opt=ours[name]: opt.step(grads=grads)
        theirs = {}
        for name, kw in (("(a) torch foreach", dict(foreach=True)), ("(b) torch fused", dict(fused=True))):
            params = [torch.nn.Parameter(p.clone()) for p in start]
            for p, g in zip(params, grads):
                p.grad = g.clone()
            try:
                opt = torch.optim.Adam(params, lr=3e-4, capturable=True, **kw)
            except (RuntimeError, TypeError, ValueError) as e:          # this torch has no such implementation
                print(f"# {name}: not offered by this torch ({e})", flush=True)
                continue
            theirs[name] = (params, opt)

            def body(params=params, opt=opt):
                torch.nn.utils.clip_grad_norm_(params, 0.5, foreach=True)
                opt.step()
            bodies[name] = body
        times = time_graphs(torch, side, bodies, calls, replays)
        side.synchronize()
        for name, opt in ours.items():                                # every replay advanced the device's step count
            assert opt.counts()[0] > calls and opt.counts()[1] == 0, (name, opt.counts())
    env.use_stream(None)
    env.close()
    return times


def cell(v):
    return f"{statistics.median(v):.1f} ({min(v):.1f} .. {max(v):.1f})" if v else "-"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", type=Path, default=ROOT / "profiles" / "adam_timing.txt")
    args = ap.parse_args()
    sys.path.insert(0, str(ROOT))
    import bench
    import torch

    assert torch.cuda.is_available(), "this is a measurement on the GPU"
    lines = [f"# {torch.cuda.get_device_name(0)}; us per optimiser step, median of 15 alternating repeats (min .. max); a repeat = replays",
             "# of a graph of several steps between two synchronisations",
             "# adam_step: ccx_adam_step (three launches: block partials of the norm, one final wave, the element update), without and",
             "# with max_grad_norm = 0.5; (a) / (b): captured clip_grad_norm_(0.5, foreach=True) + torch.optim.Adam(capturable=True,",
             "# foreach=True / fused=True).step() on the same shapes (the yardsticks)"]
    lines.append(f"{'parameters':>36}{'numel':>8}" + "".join(f"{c:>24}" for c in COLS) + f"{'clip/(a)':>10}{'clip/(b)':>10}")
    print("\n".join(lines), flush=True)
    cfg, _ = bench.workload_config("c2")
    for name, shapes, calls, replays in SETS:
        t = measure(cfg, shapes, calls, replays)
        med = {k: statistics.median(v) for k, v in t.items()}
        numel = sum(int(torch.Size(s).numel()) for s in shapes)
        ratio = lambda k: f"{med['adam_step clip'] / med[k]:>10.3f}" if k in med else f"{'-':>10}"  # noqa: E731
        row = f"{name:>36}{numel:>8}" + "".join(f"{cell(t.get(c)):>24}" for c in COLS) + ratio("(a) torch foreach") + ratio("(b) torch fused")
        lines.append(row)
        print(row, flush=True)
    args.out.parent.mkdir(parents=True, exist_ok=True)
    args.out.write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
