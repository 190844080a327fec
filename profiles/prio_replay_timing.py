#!/usr/bin/env python3
"""Device time of prioritised replay (include/ccx.h CCX_PRIO) from replayed HIP graphs, in ONE process on ONE build so that
every variant sees the same machine.  Per shape (E envs x N agents, a ring of S steps, minibatches of B):

  sample            PrioritizedReplay.sample: the refresh of the sums, the draw, the counter, and the ring's fetch
  prio_sample       its library call alone (ccx_prio_sample: refresh + draw + counter), without the fetch
  refresh+1         the same call with B = 1: the refresh's launches, a draw of one lane, the counter -- what is left of
                    prio_sample when the draw is (all but) taken away; `draw` in the table is prio_sample minus this
  fetch             ReplayRing.fetch on the drawn indices
  update            PrioritizedReplay.update_priorities from two td_error arrays: two launches
  push / ring push  PrioritizedReplay.push of K = 1 (the ring's two launches and one more) against ReplayRing.push
  (a) torch         YARDSTICK: what a user writes in torch today on the same ring, captured: cumsum of f32 priorities,
                    rand * total, searchsorted, ReplayRing.fetch, pow weights -- and, timed on its own as `(a) update`,
                    the index_put_ of new priorities (ill-defined for duplicates; timed all the same)
  (b) uniform       YARDSTICK: ReplayRing.sample, the uniform draw: the feature cannot be cheaper than this

The protocol of replay_timing.py: a graph holds CALLS calls; a repeat replays it REPLAYS times between two synchronisations;
the variants alternate over 15 repeats; the median is reported with min .. max.

    python profiles/prio_replay_timing.py [--out profiles/prio_replay_timing.txt]
"""

import argparse
import statistics
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
REPEATS = 15
# workload, label, ring steps, minibatch, calls per graph, replays per repeat
SHAPES = [("c2", "C2 4096 x 8", 64, 4096, 10, 10), ("c3", "C3 4096 x 32", 16, 1024, 10, 10)]
ALPHA, BETA, EPS = 0.6, 0.4, 1e-6


def measure(cfg, E, S, B, calls, replays):
    import torch

    from collectivecrossing_amd import BatchedCollectiveCrossing, PrioritizedReplay, ReplayRing

    env = BatchedCollectiveCrossing(cfg, E)
    N, dev = env.num_agents, env.device
    R = S * E
    side = torch.cuda.Stream()
    graphs = {}
    with torch.cuda.stream(side):
        env.use_stream(side)
        env.make_reset_pool(seed0=0, size=4096)
        env.reset_from_pool()
        env.set_rng_seed(7)
        u8 = torch.uint8
        ring, plain = ReplayRing(env, steps=S), ReplayRing(env, steps=S)
        pr = PrioritizedReplay(ring, alpha=ALPHA, beta=BETA, eps=EPS)
        traj = env.alloc_rollout(1, want_obs=True, want_compact=True, want_final=True)
        acts = torch.empty((1, E, N), dtype=u8, device=dev)
        masks = env.action_masks()
        first = env.observe()
        obs_c = torch.stack([first[:, 1, 6:10]] + [first[:, 0, 6 + 4 * j:10 + 4 * j] for j in range(1, N)], dim=1).contiguous()
        for _ in range(S):                                           # S real steps fill both rings
            env.policy_actions("greedy", out=acts[0])
            acts[0][acts[0] == 255] = 4
            env.rollout(acts, auto_reset=True, reset_obs="next", out=traj, want_compact=True, masks_out=masks)
            pr.push(obs_c, acts, traj, masks_next=masks.view(1, E, N))
            plain.push(obs_c, acts, traj, masks_next=masks.view(1, E, N))
            obs_c = traj.obs_compact[0].clone()
        torch.manual_seed(0)
        tds = tuple(torch.randn((B, N), device=dev) for _ in range(2))
        every = torch.arange(R, dtype=torch.int64, device=dev)
        for a in range(0, R, B):                                     # every leaf gets a priority of its own
            pr.update_priorities(every[a:a + B], tuple(torch.randn((min(B, R - a), N), device=dev) for _ in range(2)))
        side.synchronize()
        assert ring.state[:2].tolist() == [S, 0] and int((pr.leaf > 0).sum()) == R and pr.leaf.unique().numel() > R // 100

        pmb, one = pr.alloc_batch(B), pr.alloc_batch(1)
        mb, umb = pmb.batch, plain.alloc_batch(B)
        lib = env._lib
        # the torch composition on the same ring: f32 priorities, one per record
        prio = (pr.leaf.to(torch.float32) / 65536.0).contiguous()
        cum, u = torch.empty_like(prio), torch.empty((B,), device=dev)
        idx, p_i, w = torch.empty((B,), dtype=torch.int64, device=dev), torch.empty((B,), device=dev), torch.empty((B, N), device=dev)
        tmb = ring.alloc_batch(B)

        def prio_sample(out):
            env._enqueue(lib.ccx_prio_sample, ring.steps, pr.leaf, pr.pstate, pr.beta_dev, pr.tree, out.batch.index.numel(), 1,
                         out.batch.index, out.weights, out.leaf_drawn)

        def torch_sample():
            torch.cumsum(prio, 0, out=cum)
            torch.rand((B,), out=u)
            u.mul_(cum[-1])
            torch.searchsorted(cum, u, out=idx)
            idx.clamp_(max=R - 1)
            ring.fetch(idx, out=tmb)
            torch.index_select(prio, 0, idx, out=p_i)
            torch.div(prio.min(), p_i, out=p_i)
            w.copy_(p_i.pow_(BETA)[:, None].expand(B, N))

        def torch_update():
            new = torch.maximum(tds[0].abs().amax(dim=1), tds[1].abs().amax(dim=1)).add_(EPS).pow_(ALPHA)
            prio.index_put_((idx,), new)

        bodies = {"sample": lambda: pr.sample(B, out=pmb), "prio_sample": lambda: prio_sample(pmb), "refresh+1": lambda: prio_sample(one),
                  "fetch": lambda: ring.fetch(mb.index, out=mb), "update": lambda: pr.update_priorities(mb.index, tds),
                  "push": lambda: pr.push(obs_c, acts, traj, masks_next=masks.view(1, E, N)),
                  "ring push": lambda: plain.push(obs_c, acts, traj, masks_next=masks.view(1, E, N)),
                  "torch": torch_sample, "torch update": torch_update, "uniform": lambda: plain.sample(B, out=umb)}
        pr.sample(B, out=pmb)
        side.synchronize()
        assert int(mb.index.min()) >= 0 and int(mb.index.max()) < R and torch.equal(pmb.leaf_drawn, pr.leaf[mb.index])
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
        sizes = (4 * R, 8 * pr.tree.numel())
    env.use_stream(None)
    env.close()
    return times, sizes


def cell(v):
    return f"{statistics.median(v):.1f} ({min(v):.1f} .. {max(v):.1f})"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", type=Path, default=ROOT / "profiles" / "prio_replay_timing.txt")
    args = ap.parse_args()
    sys.path.insert(0, str(ROOT))
    import bench
    import torch

    assert torch.cuda.is_available(), "this is a measurement on the GPU"
    lines = [f"# {torch.cuda.get_device_name(0)}; us per call, median of {REPEATS} alternating repeats (min .. max); a repeat = replays of a "
             f"graph of several calls between two synchronisations",
             "# sample: PrioritizedReplay.sample (refresh + draw + counter + the ring's fetch); prio_sample: ccx_prio_sample alone;",
             "# refresh+1: ccx_prio_sample with B = 1; draw = prio_sample - refresh+1 (medians); fetch: ReplayRing.fetch; update:",
             "# update_priorities from two td_error arrays; push / ring push: K = 1; (a) torch: cumsum + rand + searchsorted + fetch + pow",
             "# weights, captured; (a) update: index_put_ of new priorities; (b) uniform: ReplayRing.sample"]
    cols = ("sample", "prio_sample", "refresh+1", "fetch", "update", "push", "ring push", "torch", "torch update", "uniform")
    names = {"torch": "(a) torch", "torch update": "(a) update", "uniform": "(b) uniform"}
    head = (f"{'shape':<14}{'S':>4}{'B':>6}{'leaf MB':>9}{'tree MB':>9}" + "".join(f"{names.get(c, c):>24}" for c in cols)
            + f"{'draw':>8}{'sample/(a)':>12}{'sample/(b)':>12}{'update/(a)':>12}{'push/ring':>11}")
    lines.append(head)
    print("\n".join(lines), flush=True)
    for workload, label, S, B, calls, replays in SHAPES:
        cfg, E = bench.workload_config(workload)
        t, (leaf_b, tree_b) = measure(cfg, E, S, B, calls, replays)
        med = {k: statistics.median(v) for k, v in t.items()}
        row = f"{label:<14}{S:>4}{B:>6}{leaf_b / 1e6:>9.2f}{tree_b / 1e6:>9.2f}" + "".join(f"{cell(t[c]):>24}" for c in cols)
        row += f"{med['prio_sample'] - med['refresh+1']:>8.1f}{med['sample'] / med['torch']:>12.4f}{med['sample'] / med['uniform']:>12.4f}"
        row += f"{med['update'] / med['torch update']:>12.4f}{med['push'] / med['ring push']:>11.4f}"
        lines.append(row)
        print(row, flush=True)
    args.out.parent.mkdir(parents=True, exist_ok=True)
    args.out.write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
