#!/usr/bin/env python3
"""Device time of `ccx_q_actions`, `ccx_td_loss` and `ccx_td_loss_backward` (include/ccx.h CCX_QLEARN) from replayed HIP
graphs, in ONE process on ONE build so that every variant sees the same machine.  Per shape:

  q_actions         ccx_q_actions with masks and a rate of 0.1: one launch
  (a) torch actions YARDSTICK: masked argmax, `rand < eps`, a uniform choice over the legal set by rank, dead slots to 255 --
                    captured torch ops
  fwd               ccx_td_loss, double-Q, with masks_next and valid: two launches
  fwd + bwd         then ccx_td_loss_backward: three launches
  two launches      ccx_td_loss on ONE row: what the two-launch structure costs when there is no work
  (b) torch fwd     YARDSTICK: the double-DQN Huber loss in torch (masked argmax, two gathers, where(done), huber_loss, a mean
                    with weights valid / n: static shape), captured and replayed
  (c) torch fwd+bwd YARDSTICK: the same with `torch.autograd.grad` to the Q-values
  (d) copy          `torch.Tensor.copy_` of as many bytes as fwd + bwd moves (reads + writes, half in, half out)

The protocol of ppo_loss_timing.py: a graph holds CALLS calls; a repeat replays it REPLAYS times between two
synchronisations; the variants alternate over 15 repeats; the median is reported with min .. max.

    python profiles/td_loss_timing.py [--out profiles/td_loss_timing.txt]
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
GAMMA, DELTA, EPS = 0.99, 1.0, 0.1


def torch_actions(q, legal, dead, eps):
    import torch

    greedy = q.masked_fill(~legal, -torch.inf).argmax(-1)
    explore = torch.rand(greedy.shape, device=q.device) < eps
    n = legal.sum(-1)
    idx = (torch.rand(greedy.shape, device=q.device) * n).long()
    rank = legal.cumsum(-1) - 1
    choice = (legal & (rank == idx[..., None])).to(torch.uint8).argmax(-1)
    act = torch.where(explore, choice, greedy)
    return torch.where(dead, torch.full_like(act, 255), act).to(torch.uint8), explore & ~dead


def torch_td(x, a64, r32, done, qt, qo, legal, w):
    import torch

    qa = x.gather(-1, a64[:, None])[:, 0]
    k = qo.masked_fill(~legal, -torch.inf).argmax(-1)
    boot = qt.gather(-1, k[:, None])[:, 0]
    y = r32 + torch.where(done, torch.zeros_like(boot), GAMMA * boot)
    return (torch.nn.functional.huber_loss(qa, y, reduction="none", delta=DELTA) * w).sum()


def measure(cfg, M, calls, replays):
    import torch

    from collectivecrossing_amd import BatchedCollectiveCrossing, QLearning, unpack_action_masks

    probe = BatchedCollectiveCrossing(cfg, 1)
    N = probe.num_agents
    probe.close()
    env = BatchedCollectiveCrossing(cfg, M // N)                    # q_actions works on the batch's own [E, N] slots
    E = env.num_envs
    side = torch.cuda.Stream()
    graphs = {}
    dev = env.device
    with torch.cuda.stream(side):
        env.use_stream(side)
        env.make_reset_pool(seed0=0, size=4096)
        env.reset_from_pool()
        env.rollout_greedy(30, auto_reset=False, want_obs=False, want_actions=False)       # some agents have arrived: dead slots
        ql = QLearning(env, epsilon=EPS)
        gen = torch.Generator(device=dev).manual_seed(M)
        q = torch.randn((M, 5), device=dev, generator=gen) * 2.0
        qt = torch.randn((M, 5), device=dev, generator=gen) * 2.0
        qo = torch.randn((M, 5), device=dev, generator=gen) * 2.0
        actions = torch.randint(0, 5, (M,), device=dev, generator=gen).to(torch.uint8)
        masks = torch.randint(0, 16, (M,), device=dev, generator=gen).to(torch.uint8) | 0x10
        valid = (torch.rand(M, device=dev, generator=gen) < 0.8).to(torch.uint8)
        done = (torch.rand(M, device=dev, generator=gen) < 0.1).to(torch.uint8)
        reward = torch.randn(M, device=dev, generator=gen, dtype=torch.float64)
        legal = unpack_action_masks(masks)
        a64, r32, done_b = actions.long(), reward.float(), done.bool()
        w = valid.float() / valid.float().sum()
        x = q.clone().requires_grad_(True)
        st = env.get_state()
        dead = torch.from_numpy((st["terminated"] | st["truncated"]) != 0).to(dev)
        q_en, masks_en, legal_en = q.view(E, N, 5), masks.view(E, N), legal.view(E, N, 5)
        acts_out = ql.alloc_q_actions(want_explored=True)
        out, one = ql.alloc_td_loss((M,), want_td_error=False), ql.alloc_td_loss((1,), want_td_error=False)
        args = (q, actions, reward, done, qt, qo, masks)
        first = tuple(t[:1] for t in args)
        kw = dict(gamma=GAMMA, huber_delta=DELTA)
        # fwd + bwd: reads three Q arrays, actions, reward, done, masks_next and valid, twice; writes grad_q
        nbytes = M * (2 * (60 + 1 + 8 + 1 + 1 + 1) + 20)
        src = torch.empty(nbytes // 2, dtype=torch.uint8, device=dev)
        dst = torch.empty_like(src)
        held = {}

        def q_actions():
            ql.q_actions(q_en, masks_en, out=acts_out)

        def t_actions():
            held["a"] = torch_actions(q_en, legal_en, dead, ql.epsilon_dev)

        def fwd():
            ql.td_loss(*args, valid=valid, **kw, out=out)

        def fwd_bwd():
            ql.td_loss(*args, valid=valid, **kw, out=out)
            ql.td_loss_backward(*args, valid=valid, **kw, stats=out.stats, out=out)

        def two_launches():
            ql.td_loss(*first, valid=valid[:1], **kw, out=one)

        def t_fwd():
            with torch.no_grad():
                held["b"] = torch_td(q, a64, r32, done_b, qt, qo, legal, w)

        def t_fwd_bwd():
            held["c"] = torch.autograd.grad(torch_td(x, a64, r32, done_b, qt, qo, legal, w), x)

        bodies = {"q_actions": q_actions, "torch actions": t_actions, "fwd": fwd, "fwd + bwd": fwd_bwd, "two launches": two_launches,
                  "torch fwd": t_fwd, "torch fwd+bwd": t_fwd_bwd, "copy": lambda: dst.copy_(src)}
        # the yardsticks compute the same things (to rounding): a wrong yardstick would be no yardstick
        q_actions()
        t_actions()
        fwd_bwd()
        t_fwd()
        t_fwd_bwd()
        side.synchronize()
        live = ~dead
        assert (acts_out.actions[dead] == 255).all() and (held["a"][0][dead] == 255).all()
        assert abs(acts_out.explored[live].float().mean().item() - EPS) < 0.02 and abs(held["a"][1][live].float().mean().item() - EPS) < 0.02
        quiet = live & (acts_out.explored == 0) & ~held["a"][1]           # neither side explored: the same masked argmax
        assert (acts_out.actions[quiet] == held["a"][0][quiet]).all()
        assert abs(held["b"].item() - out.loss.item()) <= 1e-4 * max(1.0, abs(out.loss.item())), (held["b"].item(), out.loss.item())
        err = (held["c"][0] - out.grad_q).abs().max().item() * M
        assert err <= 1e-3 * max(1.0, out.grad_q.abs().max().item() * M), err
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
    env.close()
    return times, nbytes


def cell(v):
    return f"{statistics.median(v):.1f} ({min(v):.1f} .. {max(v):.1f})"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", type=Path, default=ROOT / "profiles" / "td_loss_timing.txt")
    args = ap.parse_args()
    sys.path.insert(0, str(ROOT))
    import bench
    import torch

    assert torch.cuda.is_available(), "this is a measurement on the GPU"
    cfg, _ = bench.workload_config("c2")
    lines = [f"# {torch.cuda.get_device_name(0)}; us per call, median of {REPEATS} alternating repeats (min .. max); a repeat = replays of a "
             f"graph of several calls between two synchronisations",
             "# q_actions: ccx_q_actions with masks, rate 0.1; (a) the captured torch composition (masked argmax, rand < eps, uniform over the",
             "# legal set); fwd: ccx_td_loss, double-Q, with masks_next and valid (80 % set); fwd + bwd: then ccx_td_loss_backward; two",
             "# launches: ccx_td_loss on one row; (b) / (c) the double-DQN Huber loss as captured torch ops without / with autograd.grad;",
             "# (d) a torch copy of the bytes fwd + bwd moves (reads + writes)"]
    cols = ("q_actions", "torch actions", "fwd", "fwd + bwd", "two launches", "torch fwd", "torch fwd+bwd", "copy")
    names = {"torch actions": "(a) torch actions", "torch fwd": "(b) torch fwd", "torch fwd+bwd": "(c) torch fwd+bwd", "copy": "(d) copy"}
    head = (f"{'rows':<16}{'MB moved':>10}" + "".join(f"{names.get(c, c):>26}" for c in cols)
            + f"{'q_act/(a)':>11}{'fwd/(b)':>10}{'fwd+bwd/(c)':>13}")
    lines.append(head)
    print("\n".join(lines), flush=True)
    for label, M, calls, replays in SHAPES:
        t, nbytes = measure(cfg, M, calls, replays)
        med = {k: statistics.median(v) for k, v in t.items()}
        row = f"{label:<16}{nbytes / 1e6:>10.1f}" + "".join(f"{cell(t[c]):>26}" for c in cols)
        row += f"{med['q_actions'] / med['torch actions']:>11.4f}{med['fwd'] / med['torch fwd']:>10.4f}"
        row += f"{med['fwd + bwd'] / med['torch fwd+bwd']:>13.4f}"
        lines.append(row)
        print(row, flush=True)
    args.out.parent.mkdir(parents=True, exist_ok=True)
    args.out.write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
