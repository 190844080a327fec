#!/usr/bin/env python3
"""Device time of CCX_NSTEP (include/ccx.h) from replayed HIP graphs, in ONE process on ONE build so that every variant sees the
same machine.  Per shape (E envs x N agents, a ring of S steps filled by the greedy policy with auto-reset, minibatches of B):

  fetch n=1/3/8     NStepReplay.fetch on B fixed random indices: ONE launch
  ring fetch        ReplayRing.fetch on the same indices: ONE launch (what n = 1 costs over it is the price of the generality)
  sample / ring     NStepReplay.sample (n = 3) against ReplayRing.sample: two launches each
  push / ring       NStepReplay.push of K = 1 (three launches) against ReplayRing.push (two)
  td disc / gamma   td_loss(discount=) + td_loss_backward(discount=) against the same pair with gamma=, B N rows, double-Q
  (a) torch         YARDSTICK: the captured torch composition a user would write for n = 3 on the compact ring: per successor
                    `index_select` of cut / done / valid / reward, the `where` chain, the gather of the last record's next_c
                    and masks_next, and two `expand_observations` (it reads `head` from the ring's device state)

The protocol of replay_timing.py: a graph holds CALLS calls; a repeat replays it REPLAYS times between two synchronisations;
the variants alternate over 15 repeats; the median is reported with min .. max.

    python profiles/nstep_timing.py [--out profiles/nstep_timing.txt]
"""

import argparse
import statistics
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
REPEATS = 15
GAMMA = 0.9900000095367432                     # 0.99 as the f32 the library sees: the yardstick multiplies by the same number
# workload, label, ring steps, minibatch, calls per graph, replays per repeat
SHAPES = [("c2", "C2 4096 x 8", 64, 4096, 10, 10), ("c3", "C3 4096 x 32", 16, 1024, 10, 10)]


def measure(cfg, E, S, B, calls, replays):
    import torch

    from collectivecrossing_amd import BatchedCollectiveCrossing, NStepReplay, QLearning, ReplayRing

    env = BatchedCollectiveCrossing(cfg, E)
    N, L, dev = env.num_agents, env.obs_len, env.device
    R = S * E
    side = torch.cuda.Stream()
    graphs = {}
    with torch.cuda.stream(side):
        env.use_stream(side)
        env.make_reset_pool(seed0=0, size=4096)
        env.reset_from_pool()
        env.set_rng_seed(7)
        u8 = torch.uint8
        plain = ReplayRing(env, steps=S)
        ns = {n: NStepReplay(ReplayRing(env, steps=S), n=n, gamma=GAMMA) for n in (1, 3, 8)}
        traj = env.alloc_rollout(1, want_obs=True, want_compact=True, want_final=True)
        acts = torch.empty((1, E, N), dtype=u8, device=dev)
        masks = env.action_masks()
        first = env.observe()
        obs_c = torch.stack([first[:, 1, 6:10]] + [first[:, 0, 6 + 4 * j:10 + 4 * j] for j in range(1, N)], dim=1).contiguous()
        for _ in range(S + S // 2):                                   # the ring is rewritten once by half
            env.policy_actions("greedy", out=acts[0])
            acts[0][acts[0] == 255] = 4
            env.rollout(acts, auto_reset=True, reset_obs="next", out=traj, want_compact=True, masks_out=masks)
            for r in (plain, *ns.values()):
                r.push(obs_c, acts, traj, masks_next=masks.view(1, E, N))
            obs_c = traj.obs_compact[0].clone()
        side.synchronize()
        ring, cut = ns[3].ring, ns[3].cut
        assert ring.state[:2].tolist() == [S + S // 2, 0]
        cuts = int(cut.count_nonzero())                             # (C3's episodes are longer than the ring: it may hold none)

        g = torch.Generator(device=dev).manual_seed(3)
        idx = torch.randint(0, R, (B,), device=dev, generator=g)
        outs = {n: r.alloc_batch(B) for n, r in ns.items()}
        mb_plain, mb_drawn, mb_ring_drawn = plain.alloc_batch(B), ns[3].alloc_batch(B), plain.alloc_batch(B)
        ql = QLearning(env)
        lead = (B, N)
        q, qt, qo = (torch.randn(lead + (5,), device=dev, generator=g) for _ in range(3))
        loss = ql.alloc_td_loss(lead, want_td_error=True)

        # ---- (a): the torch composition for n = 3 on the compact ring
        f64 = torch.float64
        gamma_t = torch.tensor(GAMMA, dtype=f64, device=dev)
        t_out = dict(G=torch.empty(lead, dtype=f64, device=dev), span=torch.empty(lead, dtype=torch.int64, device=dev),
                     obs=torch.empty((B, N, L), device=dev), next_obs=torch.empty((B, N, L), device=dev))

        def torch_nstep(n=3):
            head = ring.state[0]
            p = idx // E
            e = idx - p * E
            avail = torch.where(head < S, (head - 1 - p).clamp(min=0), (head - 1 - p) % S)
            prev = idx
            env_go = torch.ones((B,), dtype=torch.bool, device=dev)
            go = torch.ones(lead, dtype=torch.bool, device=dev)
            G = ring.reward.index_select(0, idx)
            dn = ring.done.index_select(0, idx)
            span = torch.ones(lead, dtype=torch.int64, device=dev)
            m_env = torch.ones((B,), dtype=torch.int64, device=dev)
            last, gk = idx, 1.0
            for k in range(1, n):
                sk = ((p + k) % S) * E + e
                env_go = env_go & (avail >= k) & (cut.index_select(0, prev) == 0)
                go = go & env_go[:, None] & (ring.done.index_select(0, prev) == 0) & (ring.valid.index_select(0, sk) != 0)
                gk = gk * GAMMA
                G = torch.where(go, G + gk * ring.reward.index_select(0, sk), G)
                dn = torch.where(go, ring.done.index_select(0, sk), dn)
                span = span + go
                m_env = m_env + env_go
                last = torch.where(env_go, sk, last)
                prev = sk
            discount = torch.pow(gamma_t, span).float()
            valid = torch.where((span < m_env[:, None]) & (dn == 0), torch.zeros_like(dn), ring.valid.index_select(0, idx))
            actions = ring.actions.index_select(0, idx)
            masks_next = ring.masks_next.index_select(0, last)
            env.expand_observations(ring.obs_c.index_select(0, idx), out=t_out["obs"])
            env.expand_observations(ring.next_c.index_select(0, last), out=t_out["next_obs"])
            t_out["G"].copy_(G)
            t_out["span"].copy_(span)
            return discount, valid, actions, masks_next, dn

        def td(**kw):
            mb = outs[3].batch
            args = (q, mb.actions, mb.reward, mb.done, qt, qo, mb.masks_next)
            ql.td_loss(*args, valid=mb.valid, **kw, out=loss)
            ql.td_loss_backward(*args, valid=mb.valid, **kw, stats=loss.stats, out=loss)

        def push_all(r):
            return lambda: r.push(obs_c, acts, traj, masks_next=masks.view(1, E, N))

        bodies = {"fetch n=1": lambda: ns[1].fetch(idx, out=outs[1]), "fetch n=3": lambda: ns[3].fetch(idx, out=outs[3]),
                  "fetch n=8": lambda: ns[8].fetch(idx, out=outs[8]), "ring fetch": lambda: plain.fetch(idx, out=mb_plain),
                  "sample": lambda: ns[3].sample(B, out=mb_drawn), "ring sample": lambda: plain.sample(B, out=mb_ring_drawn),
                  "push": push_all(ns[8]), "ring push": push_all(plain),
                  "td disc": lambda: td(discount=outs[3].discount), "td gamma": lambda: td(gamma=GAMMA), "torch": torch_nstep}
        # the yardstick computes the same thing: spans and rows equal, the return within f64 rounding of the library's chain
        ns[3].fetch(idx, out=outs[3])
        discount, valid, actions, masks_next, dn = torch_nstep()
        side.synchronize()
        mb = outs[3].batch
        assert torch.equal(t_out["span"], outs[3].span.long()) and torch.equal(valid, mb.valid) and torch.equal(dn, mb.done)
        assert torch.equal(t_out["obs"], mb.obs) and torch.equal(t_out["next_obs"], mb.next_obs) and torch.equal(masks_next, mb.masks_next)
        assert torch.allclose(t_out["G"], mb.reward, rtol=1e-9, atol=1e-9) and torch.allclose(discount, outs[3].discount)
        spans = torch.bincount(outs[3].span.flatten().long(), minlength=4).tolist()
        for name, body in bodies.items():
            body()                                                  # warm-up: code objects, allocator blocks
            side.synchronize()
            gr = torch.cuda.CUDAGraph()
            with torch.cuda.graph(gr, stream=side):
                for _ in range(calls):
                    body()
            for _ in range(2):
                gr.replay()
            side.synchronize()
            graphs[name] = gr
        times = {k: [] for k in graphs}
        for _ in range(REPEATS):
            for name, gr in graphs.items():                         # alternate the variants
                side.synchronize()
                t0 = time.perf_counter()
                for _ in range(replays):
                    gr.replay()
                side.synchronize()
                times[name].append((time.perf_counter() - t0) / (replays * calls) * 1e6)
        graphs.clear()
    env.use_stream(None)
    env.close()
    return times, spans, cuts


def cell(v):
    return f"{statistics.median(v):.1f} ({min(v):.1f} .. {max(v):.1f})"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", type=Path, default=ROOT / "profiles" / "nstep_timing.txt")
    args = ap.parse_args()
    sys.path.insert(0, str(ROOT))
    import bench
    import torch

    assert torch.cuda.is_available(), "this is a measurement on the GPU"
    lines = [f"# {torch.cuda.get_device_name(0)}; us per call, median of {REPEATS} alternating repeats (min .. max); a repeat = replays of a "
             f"graph of several calls between two synchronisations",
             "# fetch n: NStepReplay.fetch on B fixed random indices; ring fetch: ReplayRing.fetch on the same; sample / ring sample: the",
             "# drawing forms (n = 3); push / ring push: one step; td disc / td gamma: td_loss + td_loss_backward over B N rows with",
             "# discount= / gamma=; (a) torch: the captured torch composition for n = 3 on the compact ring (see the docstring)"]
    cols = ("fetch n=1", "fetch n=3", "fetch n=8", "ring fetch", "sample", "ring sample", "push", "ring push", "td disc", "td gamma", "torch")
    names = {"torch": "(a) torch n=3"}
    head = (f"{'shape':<14}{'S':>4}{'B':>6}" + "".join(f"{names.get(c, c):>24}" for c in cols)
            + f"{'n=1/ring':>10}{'n=3/ring':>10}{'n=3/(a)':>10}{'disc/gamma':>12}{'spans 1,2,3 (n=3)':>24}{'cuts':>8}")
    lines.append(head)
    print("\n".join(lines), flush=True)
    for workload, label, S, B, calls, replays in SHAPES:
        cfg, E = bench.workload_config(workload)
        t, spans, cuts = measure(cfg, E, S, B, calls, replays)
        med = {k: statistics.median(v) for k, v in t.items()}
        row = f"{label:<14}{S:>4}{B:>6}" + "".join(f"{cell(t[c]):>24}" for c in cols)
        row += f"{med['fetch n=1'] / med['ring fetch']:>10.3f}{med['fetch n=3'] / med['ring fetch']:>10.3f}{med['fetch n=3'] / med['torch']:>10.4f}"
        row += f"{med['td disc'] / med['td gamma']:>12.3f}{str(spans[1:4]):>24}{cuts:>8}"
        lines.append(row)
        print(row, flush=True)
    args.out.parent.mkdir(parents=True, exist_ok=True)
    args.out.write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
