#!/usr/bin/env python3
"""Device time of `ccx_c51_q_values`, `ccx_c51_loss` and `ccx_c51_loss_backward` (categorical Q-heads, include/ccx.h CCX_C51)
from replayed HIP graphs, in ONE process on ONE build so that every variant sees the same machine.  A = 51 atoms, double-Q
with masks and `valid`.  Per shape:

  q_values          the expected values of [rows, 5, A] logits
  loss              the two launches of the loss (block partials, final wave) with row_loss and proj
  loss + bwd        then the backward kernel
  one row           the same two launches on ONE row: the fixed cost of the two-launch structure
  (a) torch graph   THE YARDSTICK: the same quantities and their gradient as a user writes them with torch alone -- softmax,
                    expected values, masked argmax, gather, floor / ceil with `index_add_`, `log_softmax`, a mean over `valid`,
                    `torch.autograd.grad` (examples/c51_dqn.py: torch_c51_loss) -- captured and replayed
  (b) copy          `torch.Tensor.copy_` of as many bytes as loss + bwd moves (reads + writes, half in, half out)

The protocol of evaluate_timing.py: a graph holds CALLS calls; a repeat replays it REPLAYS times between two synchronisations;
the variants alternate over 15 repeats; the median is reported with min .. max.  A gain over (a) is claimed only where the
median lies below (a)'s by more than the observed min .. max spread of both.

    python profiles/c51_timing.py [--out profiles/c51_timing.txt]
"""

import argparse
import statistics
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
REPEATS = 15
ATOMS, GAMMA = 51, 0.99
# label, leading shape, calls per graph, replays per repeat
SHAPES = [("512 x 8", (512, 8), 10, 5), ("32768", (32768,), 10, 3)]


def measure(env, lead, calls, replays):
    import torch

    sys.path.insert(0, str(ROOT / "examples"))
    from c51_dqn import torch_c51_loss

    from collectivecrossing_amd import CategoricalQ

    side = torch.cuda.Stream()
    graphs = {}
    dev = env.device
    A = ATOMS
    M = 1
    for n in lead:
        M *= n
    with torch.cuda.stream(side):
        env.use_stream(side)
        cq = CategoricalQ(env, atoms=A)
        gen = torch.Generator(device=dev).manual_seed(M)
        logits, nt, no = (torch.randn(lead + (5, A), device=dev, generator=gen) * 2.0 for _ in range(3))
        actions = torch.randint(0, 5, lead, device=dev, generator=gen).to(torch.uint8)
        masks = torch.randint(0, 32, lead, device=dev, generator=gen).to(torch.uint8)
        valid = (torch.rand(lead, device=dev, generator=gen) < 0.9).to(torch.uint8)
        done = (torch.rand(lead, device=dev, generator=gen) < 0.1).to(torch.uint8)
        reward = torch.randn(lead, device=dev, generator=gen).double()
        x = logits.clone().requires_grad_(True)
        out, one = cq.alloc_loss(lead), cq.alloc_loss((1,))
        q = torch.empty(lead + (5,), device=dev)
        first = tuple(t.reshape((-1,) + t.shape[len(lead):])[:1] for t in (logits, actions, reward, done, nt, no, masks, valid))
        # loss + bwd, reads + writes: the rows of A floats (logits[a], five of next_online, next_target[k*], proj out; logits[a]
        # and proj in, 5 A out), the small arrays, row_loss
        nbytes = M * (4 * A * (1 + 5 + 1 + 1) + (1 + 8 + 1 + 1 + 1) + 4 + 4 * A * (1 + 1 + 5) + (1 + 1))
        src = torch.empty(nbytes // 2, dtype=torch.uint8, device=dev)
        dst = torch.empty_like(src)

        def loss():
            cq.loss(logits, actions, reward, done, nt, no, masks, valid, gamma=GAMMA, out=out)

        def loss_bwd():
            loss()
            cq.loss_backward(logits, actions, out.proj, valid, stats=out.stats, out=out)

        held = {}

        def torch_graph():
            l, proj = torch_c51_loss(x, actions, reward, done, nt, no, masks, valid, cq.support, GAMMA)
            held["t"] = (l, proj, torch.autograd.grad(l, x)[0])

        bodies = {"q_values": lambda: cq.q_values(logits, out=q), "loss": loss, "loss + bwd": loss_bwd,
                  "one row": lambda: cq.loss(*first, gamma=GAMMA, out=one), "torch graph": torch_graph, "copy": lambda: dst.copy_(src)}
        # the torch composition computes the same quantities (to rounding): a wrong yardstick would be no yardstick
        loss_bwd()
        torch_graph()
        side.synchronize()
        t_loss, t_proj, t_grad = held["t"]
        assert abs(t_loss.item() - out.stats[0].item()) <= 1e-3 * max(1.0, abs(out.stats[0].item())), (t_loss.item(), out.stats[0].item())
        for a, b, tail in ((t_proj.detach(), out.proj, 1), (t_grad * M, out.grad_logits * M, 2)):
            off = ((a - b).abs().reshape((M, -1)).amax(-1) > 1e-3).float().mean().item()
            assert off <= 1e-3, off                                 # (a row whose two best next-values all but tie may bootstrap from the other)
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
    ap.add_argument("--out", type=Path, default=ROOT / "profiles" / "c51_timing.txt")
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
             f"# A = {ATOMS} atoms, double-Q with masks and valid.  q_values: ccx_c51_q_values; loss: ccx_c51_loss with row_loss and proj;",
             "# loss + bwd: then ccx_c51_loss_backward; one row: ccx_c51_loss on ONE row (the fixed cost of its two launches); (a) the",
             "# captured torch composition for the same quantities and their gradient (softmax, expected values, masked argmax, gather,",
             "# floor / ceil with index_add_, log_softmax, a mean over valid, autograd.grad): the yardstick; (b) a torch copy of the bytes",
             "# loss + bwd moves (reads + writes).  The arrays of both shapes fit the Infinity Cache: no figure here is an HBM rate.",
             "# gain: yes where the median of loss + bwd lies below (a)'s by more than the min .. max spread of both, else no"]
    cols = ("q_values", "loss", "loss + bwd", "one row", "torch graph", "copy")
    names = {"torch graph": "(a) torch graph", "copy": "(b) copy"}
    head = f"{'rows':<10}{'MB moved':>10}" + "".join(f"{names.get(c, c):>30}" for c in cols) + f"{'loss+bwd/(a)':>14}{'loss+bwd/(b)':>14}{'gain':>6}"
    lines.append(head)
    print("\n".join(lines), flush=True)
    for label, lead, calls, replays in SHAPES:
        t, nbytes = measure(env, lead, calls, replays)
        med = {k: statistics.median(v) for k, v in t.items()}
        spread = (max(t["loss + bwd"]) - min(t["loss + bwd"])) + (max(t["torch graph"]) - min(t["torch graph"]))
        gain = med["torch graph"] - med["loss + bwd"] > spread
        row = f"{label:<10}{nbytes / 1e6:>10.1f}" + "".join(f"{cell(t[c]):>30}" for c in cols)
        row += f"{med['loss + bwd'] / med['torch graph']:>14.4f}{med['loss + bwd'] / med['copy']:>14.2f}{'yes' if gain else 'no':>6}"
        lines.append(row)
        print(row, flush=True)
    env.close()
    args.out.parent.mkdir(parents=True, exist_ok=True)
    args.out.write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
