#!/usr/bin/env python3
"""Device time of the wide head (include/ccx.h CCX_MLP_WIDE: Linear(38, 64) -> Tanh -> Linear(64, 255), the C51 head of the
8-agent batch at A = 51) from replayed HIP graphs, in ONE process on ONE build so that every variant sees the same machine.
Per row count:

  forward             ccx_mlp_wide_forward: rows -> [rows, 5, 51] logits and the hidden activations, one kernel
  forward + grads     then ccx_mlp_wide_backward: the four parameter gradients, two more kernels
  (a) torch fwd       THE YARDSTICK: a captured torch.nn.Sequential of the same sizes (hipBLASLt's kernels and the tanh)
  (a) torch fwd+grad  .. and torch.autograd.grad of its four parameters under the same grad_y
  (b) copy            `torch.Tensor.copy_` of as many bytes as forward + grads moves (reads + writes, half in, half out)
  five narrow         the workaround this head replaces, for scale: five ccx_mlp_forward of O = 8 and five ccx_mlp_backward
                      (40 outputs, not 255: tests/test_gpu_c51_chain.py's network)

The protocol of mlp_timing.py: a graph holds CALLS calls; a repeat replays it REPLAYS times between two synchronisations; the
variants alternate over 15 repeats; the median is reported with min .. max.  A gain over (a) is claimed only where the median
lies below (a)'s by more than the observed min .. max spread of both (profiles/c51_timing.py's rule).  The layer-2 arithmetic
here is unfused f32 on the vector ALUs, in a fixed order; hipBLASLt's is MFMA: the head is there for the bits.

    python profiles/mlp_wide_timing.py [--out profiles/mlp_wide_timing.txt]
"""

import argparse
import statistics
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "profiles"))
from mlp_timing import REPEATS, cell, time_graphs  # noqa: E402

L, H, A = 38, 64, 51
O = 5 * A
# rows, calls per graph, replays per repeat
SHAPES = [(4096, 10, 10), (32768, 5, 10)]


def measure(env, rows, calls, replays):
    import torch

    from collectivecrossing_amd import WideMlpHead

    dev, f = env.device, torch.float32
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        env.use_stream(side)
        torch.manual_seed(0)
        head = WideMlpHead(env, H, O, L=L, out_shape=(5, A))
        seq = head.to_sequential()
        x = torch.randint(0, 13, (rows, L), device=dev).float()
        gy = torch.randn((rows, 5, A), device=dev)
        y, hid = torch.empty((rows, 5, A), device=dev), torch.empty((rows, H), device=dev)
        grads = head.alloc_param_grads((rows,))
        narrow = [env.mlp_head(H, O=8, L=L) for _ in range(5)]
        ny, nh = [torch.empty((rows, 8), device=dev) for _ in range(5)], [torch.empty((rows, H), device=dev) for _ in range(5)]
        ngy = [torch.randn((rows, 8), device=dev) for _ in range(5)]
        ngrads = [env.alloc_mlp_backward(h, (rows,)) for h in narrow]
        held = {}
        # the bytes forward + grads moves: x, y, hidden written; x, hidden, grad_y read; the parameters and gradients are small
        nbytes = 4 * rows * (L + O + H) + 4 * rows * (L + H + O)
        src, dst = torch.empty(nbytes // 2, dtype=torch.uint8, device=dev), torch.empty(nbytes // 2, dtype=torch.uint8, device=dev)

        def forward():
            with torch.no_grad():
                head(x, out=y, hidden_out=hid)

        def forward_grads():
            forward()
            head.param_grads(x, hid, gy, out=grads)

        def torch_forward():
            with torch.no_grad():
                held["y"] = seq(x)

        def torch_forward_grad():
            with torch.enable_grad():
                out = seq(x)
                held["g"] = torch.autograd.grad(out, list(seq.parameters()), gy.view(rows, O))

        def five_narrow():
            with torch.no_grad():
                for k, h in enumerate(narrow):
                    h(x, out=ny[k], hidden_out=nh[k])
            for k, h in enumerate(narrow):
                env.mlp_backward(h, x, nh[k], ngy[k], out=ngrads[k])

        forward()
        with torch.no_grad():
            err = (seq(x).view(rows, 5, A) - y).abs().max().item()      # the yardstick computes the same logits (to rounding)
        assert err <= 1e-4, err
        assert y.dtype is f
        bodies = {"forward": forward, "forward + grads": forward_grads, "torch fwd": torch_forward, "torch fwd+grad": torch_forward_grad,
                  "copy": lambda: dst.copy_(src), "five narrow": five_narrow}
        times = time_graphs(torch, side, bodies, calls, replays)
        held.clear()
    env.use_stream(None)
    return times, nbytes


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", type=Path, default=ROOT / "profiles" / "mlp_wide_timing.txt")
    args = ap.parse_args()
    sys.path.insert(0, str(ROOT))
    import bench
    import torch

    from collectivecrossing_amd import BatchedCollectiveCrossing

    assert torch.cuda.is_available(), "this is a measurement on the GPU"
    cfg, _ = bench.workload_config("c2")
    env = BatchedCollectiveCrossing(cfg, 64)
    lines = [f"# {torch.cuda.get_device_name(0)}; us per call, median of {REPEATS} alternating repeats (min .. max); a repeat = replays of a "
             f"graph of several calls between two synchronisations",
             f"# the head: Linear({L}, {H}) -> Tanh -> Linear({H}, {O}).  forward: ccx_mlp_wide_forward with hidden; forward + grads: then",
             "# ccx_mlp_wide_backward (three kernels in all); (a) the captured torch.nn.Sequential of the same sizes, and with autograd.grad",
             "# of its four parameters: the yardstick; (b) a torch copy of the bytes forward + grads moves (reads + writes); five narrow:",
             "# five ccx_mlp_forward + five ccx_mlp_backward at O = 8, the workaround this head replaces (40 outputs, not 255).",
             "# The arrays of both shapes fit the Infinity Cache: no figure here is an HBM rate.",
             "# gain: yes where the median lies below (a)'s by more than the min .. max spread of both, else no (forward; forward + grads)"]
    cols = ("forward", "forward + grads", "torch fwd", "torch fwd+grad", "copy", "five narrow")
    names = {"torch fwd": "(a) torch fwd", "torch fwd+grad": "(a) torch fwd+grad", "copy": "(b) copy"}
    lines.append(f"{'rows':<8}{'MB moved':>10}" + "".join(f"{names.get(c, c):>30}" for c in cols) + f"{'fwd/(a)':>10}{'f+g/(a)':>10}{'f+g/(b)':>10}{'gain':>10}")
    print("\n".join(lines), flush=True)
    for rows, calls, replays in SHAPES:
        t, nbytes = measure(env, rows, calls, replays)
        med = {k: statistics.median(v) for k, v in t.items()}
        gains = []
        for ours, theirs in (("forward", "torch fwd"), ("forward + grads", "torch fwd+grad")):
            spread = (max(t[ours]) - min(t[ours])) + (max(t[theirs]) - min(t[theirs]))
            gains.append("yes" if med[theirs] - med[ours] > spread else "no")
        row = f"{rows:<8}{nbytes / 1e6:>10.1f}" + "".join(f"{cell(t[c]):>30}" for c in cols)
        row += (f"{med['forward'] / med['torch fwd']:>10.3f}{med['forward + grads'] / med['torch fwd+grad']:>10.3f}"
                f"{med['forward + grads'] / med['copy']:>10.2f}{'; '.join(gains):>10}")
        lines.append(row)
        print(row, flush=True)
    env.close()
    args.out.parent.mkdir(parents=True, exist_ok=True)
    args.out.write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
