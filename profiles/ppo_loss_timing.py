#!/usr/bin/env python3
"""Device time of `ccx_ppo_loss` / `ccx_ppo_loss_backward` / `ccx_masked_moments` (include/ccx.h CCX_PPO_LOSS) from replayed
HIP graphs, in ONE process on ONE build so that every variant sees the same machine.  Per shape:

  fwd               ccx_ppo_loss with masks, valid and norm: two launches
  fwd + bwd         then ccx_ppo_loss_backward with both gradients: three launches
  moments           ccx_masked_moments: two launches
  two launches      ccx_ppo_loss on ONE row: what the two-launch structure costs when there is no work -- about twice what the
                    final wave's launch adds to fwd (and to moments)
  (a) eval + torch  YARDSTICK: evaluate_actions (autograd: its two kernels) for logp and entropy, the rest of the loss as torch
                    ops with weights valid / n instead of boolean indexing (static shape), `torch.autograd.grad` to logits and
                    values -- captured and replayed
  (b) torch graph   YARDSTICK: the whole loss in torch alone (masked_fill, log_softmax, gather, guarded entropy, exp, clamp,
                    minimum, weighted sums, autograd.grad), captured and replayed
  (c) copy          `torch.Tensor.copy_` of as many bytes as fwd + bwd moves (reads + writes, half in, half out)

The protocol of evaluate_timing.py: a graph holds CALLS calls; a repeat replays it REPLAYS times between two
synchronisations; the variants alternate over 15 repeats; the median is reported with min .. max.

    python profiles/ppo_loss_timing.py [--out profiles/ppo_loss_timing.txt]
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
HYPER = dict(clip=0.2, vf_coef=0.5, ent_coef=0.01, adv_eps=1e-8)


def rest_of_the_loss(logp, entropy, v, lpo, adv, ret, w, norm):
    import torch

    ratio = torch.exp(logp - lpo)
    an = (adv - norm[1]) / (norm[2] + HYPER["adv_eps"])
    surr = torch.minimum(ratio * an, ratio.clamp(1 - HYPER["clip"], 1 + HYPER["clip"]) * an)
    return -(surr * w).sum() + HYPER["vf_coef"] * ((v - ret).pow(2) * w).sum() - HYPER["ent_coef"] * (entropy * w).sum()


def torch_loss(x, v, actions64, legal, lpo, adv, ret, w, norm):
    import torch

    lp = torch.log_softmax(x.masked_fill(~legal, -torch.inf), -1)
    logp = lp.gather(-1, actions64[:, None])[:, 0]
    p = lp.exp()
    zero = torch.zeros_like(lp)
    entropy = -torch.where(p > 0, p * torch.where(p > 0, lp, zero), zero).sum(-1)
    return rest_of_the_loss(logp, entropy, v, lpo, adv, ret, w, norm)


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
        valid = (torch.rand(M, device=dev, generator=gen) < 0.8).to(torch.uint8)
        values, adv, ret = (torch.randn(M, device=dev, generator=gen) for _ in range(3))
        lpo = env.evaluate_actions(logits, actions, masks, want_entropy=False).logp + 0.3 * torch.randn(M, device=dev, generator=gen)
        legal = unpack_action_masks(masks)
        actions64 = actions.long()
        w = valid.float() / valid.float().sum()
        x = logits.clone().requires_grad_(True)
        v = values.clone().requires_grad_(True)
        out = env.alloc_ppo_loss((M,))
        one = env.alloc_ppo_loss((1,))
        norm = env.masked_moments(adv, valid)
        norm_out = torch.empty_like(norm)
        inputs = dict(logits=logits, values=values, actions=actions, logp_old=lpo, advantages=adv, returns=ret, masks=masks,
                      valid=valid, norm=norm, **HYPER)
        first = {k: (t[:1] if isinstance(t, torch.Tensor) and k != "norm" else t) for k, t in inputs.items()}
        # fwd + bwd: reads logits, actions, masks, valid, four f32 arrays, twice; writes both gradients
        nbytes = M * (2 * (20 + 1 + 1 + 1 + 16) + 20 + 4)
        src = torch.empty(nbytes // 2, dtype=torch.uint8, device=dev)
        dst = torch.empty_like(src)

        def fwd():
            env.ppo_loss(**inputs, out=out)

        def fwd_bwd():
            env.ppo_loss(**inputs, out=out)
            env.ppo_loss_backward(**inputs, stats=out.stats, out=out)

        def moments():
            env.masked_moments(adv, valid, out=norm_out, workspace=out.workspace)

        def two_launches():
            env.ppo_loss(**first, out=one)

        held = {}

        def eval_torch():
            ev = env.evaluate_actions(x, actions, masks)
            held["a"] = torch.autograd.grad(rest_of_the_loss(ev.logp, ev.entropy, v, lpo, adv, ret, w, norm), (x, v))

        def torch_graph():
            held["b"] = torch.autograd.grad(torch_loss(x, v, actions64, legal, lpo, adv, ret, w, norm), (x, v))

        bodies = {"fwd": fwd, "fwd + bwd": fwd_bwd, "moments": moments, "two launches": two_launches, "eval + torch": eval_torch,
                  "torch graph": torch_graph, "copy": lambda: dst.copy_(src)}
        # the yardsticks compute the same loss and gradients (to rounding): a wrong yardstick would be no yardstick
        fwd_bwd()
        eval_torch()
        torch_graph()
        t_loss = torch_loss(x, v, actions64, legal, lpo, adv, ret, w, norm)
        side.synchronize()
        assert abs(t_loss.item() - out.loss.item()) <= 1e-4 * max(1.0, abs(out.loss.item())), (t_loss.item(), out.loss.item())
        for key in ("a", "b"):
            for a, b in zip(held[key], (out.grad_logits, out.grad_values)):
                err = (a - b).abs().max().item() * M
                assert err <= 1e-3 * max(1.0, b.abs().max().item() * M), (key, err)
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
    ap.add_argument("--out", type=Path, default=ROOT / "profiles" / "ppo_loss_timing.txt")
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
             "# fwd: ccx_ppo_loss with masks, valid (80 % set) and norm; fwd + bwd: then ccx_ppo_loss_backward with both gradients; moments:",
             "# ccx_masked_moments; two launches: ccx_ppo_loss on one row (the cost of the two-launch structure without work); (a)",
             "# evaluate_actions with autograd plus the rest of the loss as captured torch ops on weights valid / n; (b) the whole loss as",
             "# captured torch ops; (c) a torch copy of the bytes fwd + bwd moves (reads + writes)"]
    cols = ("fwd", "fwd + bwd", "moments", "two launches", "eval + torch", "torch graph", "copy")
    names = {"eval + torch": "(a) eval + torch", "torch graph": "(b) torch graph", "copy": "(c) copy"}
    head = (f"{'rows':<16}{'MB moved':>10}" + "".join(f"{names.get(c, c):>26}" for c in cols)
            + f"{'fwd+bwd/(a)':>13}{'fwd+bwd/(b)':>13}{'final wave':>12}")
    lines.append(head)
    print("\n".join(lines), flush=True)
    for label, M, calls, replays in SHAPES:
        t, nbytes = measure(env, M, calls, replays)
        med = {k: statistics.median(v) for k, v in t.items()}
        row = f"{label:<16}{nbytes / 1e6:>10.1f}" + "".join(f"{cell(t[c]):>26}" for c in cols)
        # the final wave's launch: half of the no-work pair, as a share of fwd (it reads 48 B bytes more when there is work)
        row += f"{med['fwd + bwd'] / med['eval + torch']:>13.4f}{med['fwd + bwd'] / med['torch graph']:>13.4f}"
        row += f"{0.5 * med['two launches'] / med['fwd']:>12.2f}"
        lines.append(row)
        print(row, flush=True)
    lines.append("# final wave: half of `two launches` over fwd -- the share of a forward call that the second launch takes, estimated "
                 "from the pair without work")
    env.close()
    args.out.parent.mkdir(parents=True, exist_ok=True)
    args.out.write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
