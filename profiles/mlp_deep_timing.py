#!/usr/bin/env python3
"""Device time of the deep head (include/ccx.h CCX_MLP_DEEP: Linear(38, H1) -> Tanh -> Linear(H1, H2) -> Tanh -> Linear(H2, 5))
from replayed HIP graphs, in ONE process on ONE build so that every variant sees the same machine.  Per head and row count:

  forward             ccx_mlp_deep_forward with both hiddens: rows -> logits, one kernel
  forward + grads     then ccx_mlp_deep_backward: the six parameter gradients, three more kernels
  sample_actions      ccx_mlp_deep_sample_actions: rows -> actions and logp, one kernel
  (a) torch fwd       THE YARDSTICK: a captured torch.nn.Sequential of the same sizes (hipBLASLt's kernels and the tanh)
  (a) torch fwd+grad  .. and torch.autograd.grad of its six parameters under the same grad_y
  (b) copy            `torch.Tensor.copy_` of as many bytes as forward + grads moves (reads + writes, half in, half out)
  (c) two launches    the forward without this head: Linear + Tanh in torch, then ccx_mlp_forward on its output

The protocol of mlp_timing.py: a graph holds CALLS calls; a repeat replays it REPLAYS times between two synchronisations; the
variants alternate over 15 repeats; the median is reported with min .. max.  A gain over (a) is claimed only where the median
lies below (a)'s by more than the observed min .. max spread of both (profiles/c51_timing.py's rule).  The layers here are
unfused f32 on the vector ALUs, in a fixed order; hipBLASLt's are MFMA: the head is there for the bits and for the one-launch
actor step.

    python profiles/mlp_deep_timing.py [--out profiles/mlp_deep_timing.txt]
"""

import argparse
import statistics
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "profiles"))
from mlp_timing import REPEATS, cell, time_graphs  # noqa: E402

O = 5
HEADS = ((64, 64), (256, 256))
# envs (x 8 agents = rows), calls per graph, replays per repeat
SHAPES = ((512, 10, 5), (4096, 5, 4))


def measure(cfg, E, H1, H2, calls, replays):
    import torch

    from collectivecrossing_amd import BatchedCollectiveCrossing, DeepMlpHead

    env = BatchedCollectiveCrossing(cfg, E)
    env.make_reset_pool(seed0=0, size=4096)
    env.reset_from_pool()
    N, L = env.num_agents, env.obs_len
    rows = E * N
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        env.use_stream(side)
        torch.manual_seed(0)
        head = DeepMlpHead(env, H1, H2, O)
        seq = head.to_sequential()
        first = torch.nn.Sequential(seq[0], seq[1])
        obs, masks = env.observe(), env.action_masks()
        x = obs.view(rows, L)
        gy = torch.randn((rows, O), device=env.device)
        y, h1, h2 = (torch.empty((rows, k), device=env.device) for k in (O, H1, H2))
        y2 = torch.empty((rows, O), device=env.device)
        grads = head.alloc_param_grads((rows,))
        out = env.alloc_sample(want_logp=True)
        # bytes forward + grads moves: x twice, both hiddens written and read, y, grad_y (the parameters are small beside them)
        nbytes = 4 * rows * (2 * L + 2 * (H1 + H2) + 2 * O)
        src = torch.empty(nbytes // 2, dtype=torch.uint8, device=env.device)
        dst = torch.empty_like(src)
        held = {}

        def forward():
            with torch.no_grad():
                head(x, out=y, hidden1_out=h1, hidden2_out=h2)

        def forward_grads():
            forward()
            head.param_grads(x, h1, h2, gy, out=grads)

        def torch_forward():
            with torch.no_grad():
                held["y"] = seq(x)

        def torch_forward_grad():
            with torch.enable_grad():
                held["g"] = torch.autograd.grad(seq(x), list(seq.parameters()), gy)

        def two_launches():
            with torch.no_grad():
                held["h"] = first(x)
            env._enqueue(env._lib.ccx_mlp_forward, rows, H1, H2, O, 0, held["h"], head.w2t, head.b2, head.w3, head.b3, y2, None)

        forward()
        two_launches()
        with torch.no_grad():
            err = (seq(x) - y).abs().max().item()                       # the yardstick computes the same logits (to rounding)
            err2 = (y2 - y).abs().max().item()
        assert err <= 1e-4 and err2 <= 1e-4, (err, err2)
        bodies = {"forward": forward, "forward + grads": forward_grads,
                  "sample_actions": lambda: head.sample_actions(obs, masks, out=out), "torch fwd": torch_forward,
                  "torch fwd+grad": torch_forward_grad, "copy": lambda: dst.copy_(src), "two launches": two_launches}
        times = time_graphs(torch, side, bodies, calls, replays)
        held.clear()
    env.use_stream(None)
    env.close()
    return times, rows, nbytes


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", type=Path, default=ROOT / "profiles" / "mlp_deep_timing.txt")
    args = ap.parse_args()
    sys.path.insert(0, str(ROOT))
    import bench
    import torch

    assert torch.cuda.is_available(), "this is a measurement on the GPU"
    cfg, _ = bench.workload_config("c2")
    lines = [f"# {torch.cuda.get_device_name(0)}; us per call, median of {REPEATS} alternating repeats (min .. max); a repeat = replays of a "
             f"graph of several calls between two synchronisations",
             f"# the head: Linear(38, H1) -> Tanh -> Linear(H1, H2) -> Tanh -> Linear(H2, {O}) on the observation rows of the C2 workload.",
             "# forward: ccx_mlp_deep_forward with both hiddens; forward + grads: then ccx_mlp_deep_backward (four kernels in all);",
             "# sample_actions: rows -> actions and logp in one kernel; (a) the captured torch.nn.Sequential of the same sizes, and with",
             "# autograd.grad of its six parameters: the yardstick; (b) a torch copy of the bytes forward + grads moves (reads + writes);",
             "# (c) the forward as two existing launches: Linear + Tanh in torch, then ccx_mlp_forward.",
             "# The arrays of every shape fit the Infinity Cache: no figure here is an HBM rate.",
             "# gain: yes where the median lies below (a)'s by more than the min .. max spread of both, else no (forward; forward + grads)"]
    cols = ("forward", "forward + grads", "sample_actions", "torch fwd", "torch fwd+grad", "copy", "two launches")
    names = {"torch fwd": "(a) torch fwd", "torch fwd+grad": "(a) torch fwd+grad", "copy": "(b) copy", "two launches": "(c) two launches"}
    lines.append(f"{'head':<12}{'rows':>7}{'MB moved':>10}" + "".join(f"{names.get(c, c):>29}" for c in cols)
                 + f"{'fwd/(a)':>9}{'f+g/(a)':>9}{'fwd/(c)':>9}{'gain':>10}")
    print("\n".join(lines), flush=True)
    for H1, H2 in HEADS:
        for E, calls, replays in SHAPES:
            t, rows, nbytes = measure(cfg, E, H1, H2, calls, replays)
            med = {k: statistics.median(v) for k, v in t.items()}
            gains = []
            for ours, theirs in (("forward", "torch fwd"), ("forward + grads", "torch fwd+grad")):
                spread = (max(t[ours]) - min(t[ours])) + (max(t[theirs]) - min(t[theirs]))
                gains.append("yes" if med[theirs] - med[ours] > spread else "no")
            row = f"{f'38-{H1}-{H2}-{O}':<12}{rows:>7}{nbytes / 1e6:>10.1f}" + "".join(f"{cell(t[c]):>29}" for c in cols)
            row += (f"{med['forward'] / med['torch fwd']:>9.3f}{med['forward + grads'] / med['torch fwd+grad']:>9.3f}"
                    f"{med['forward'] / med['two launches']:>9.3f}{'; '.join(gains):>10}")
            lines.append(row)
            print(row, flush=True)
    args.out.parent.mkdir(parents=True, exist_ok=True)
    args.out.write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
