#!/usr/bin/env python3
"""Device time of `ccx_replay_push` and `ccx_replay_sample` (include/ccx.h CCX_REPLAY) from replayed HIP graphs, in ONE process
on ONE build so that every variant sees the same machine.  Per shape (E envs x N agents, a ring of S steps, minibatches of B):

  push              ReplayRing.push of K = 1: two launches (the block, the head)
  slices            what examples/dqn_two_policies.py's actor_step does instead: seven slice copies into a ROW-form ring and
                    two `torch.where`, at a fixed ring position -- captured torch ops
  sample            ReplayRing.sample: two launches (draw + gather + expand, the draw counter)
  (a) rows ring     YARDSTICK: the example's captured minibatch on the row-form ring: `torch.randint` + seven `index_select`
  (b) compact ring  YARDSTICK: the same on compact arrays, followed by two `expand_observations`
  (c) copy          YARDSTICK: `torch.Tensor.copy_` of as many bytes as `sample` writes (half in, half out: the bytes it moves
                    if every record were read once)

The protocol of td_loss_timing.py: a graph holds CALLS calls; a repeat replays it REPLAYS times between two synchronisations;
the variants alternate over 15 repeats; the median is reported with min .. max.

    python profiles/replay_timing.py [--out profiles/replay_timing.txt]
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


def measure(cfg, E, S, B, calls, replays):
    import torch

    from collectivecrossing_amd import BatchedCollectiveCrossing, ReplayRing
    from collectivecrossing_amd._abi import AF_LIVE, AF_TERMINATED, EF_RESET

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
        ring = ReplayRing(env, steps=S)
        rows = dict(obs=torch.zeros((R, N, L), device=dev), next_obs=torch.zeros((R, N, L), device=dev),
                    acts=torch.full((R, N), 255, dtype=u8, device=dev), reward=torch.zeros((R, N), dtype=torch.float64, device=dev),
                    done=torch.zeros((R, N), dtype=u8, device=dev), valid=torch.zeros((R, N), dtype=u8, device=dev),
                    masks_next=torch.full((R, N), 0x1F, dtype=u8, device=dev))
        compact = dict(rows, obs=ring.obs_c, next_obs=ring.next_c)      # the compact form of the same seven arrays
        # S real steps fill both rings: the greedy policy with auto-reset, rows and compact records side by side
        traj = env.alloc_rollout(1, want_obs=True, want_compact=True, want_final=True)
        acts = torch.empty((1, E, N), dtype=u8, device=dev)
        masks = env.action_masks()
        obs = env.observe()
        first = obs
        obs_c = torch.stack([first[:, 1, 6:10]] + [first[:, 0, 6 + 4 * j:10 + 4 * j] for j in range(1, N)], dim=1).contiguous()
        everything = torch.tensor(0x1F, dtype=u8, device=dev)

        def slices(at):
            af = traj.agent_flags[0]
            reset = (traj.env_flags[0] & EF_RESET) != 0
            rows["obs"][at:at + E] = obs
            rows["acts"][at:at + E] = acts[0]
            rows["reward"][at:at + E] = traj.reward[0]
            rows["done"][at:at + E] = af & AF_TERMINATED
            rows["valid"][at:at + E] = af & AF_LIVE
            rows["next_obs"][at:at + E] = torch.where(reset[:, None, None], traj.final_obs[0], traj.obs[0])
            rows["masks_next"][at:at + E] = torch.where(reset[:, None], everything, masks)

        for t in range(S):
            env.policy_actions("greedy", out=acts[0])
            acts[0][acts[0] == 255] = 4
            env.rollout(acts, auto_reset=True, reset_obs="next", out=traj, want_compact=True, masks_out=masks)
            slices(t * E)
            ring.push(obs_c, acts, traj, masks_next=masks.view(1, E, N))
            obs, obs_c = traj.obs[0].clone(), traj.obs_compact[0].clone()
        side.synchronize()
        assert ring.state[:2].tolist() == [S, 0]
        assert torch.equal(ring.actions, rows["acts"]) and torch.equal(ring.valid, rows["valid"]) and torch.equal(ring.reward, rows["reward"])
        assert torch.equal(env.expand_observations(ring.next_c[:E]), rows["next_obs"][:E])

        mb = ring.alloc_batch(B)
        idx = torch.zeros((B,), dtype=torch.int64, device=dev)
        out_rows = {k: torch.empty((B,) + tuple(t.shape[1:]), dtype=t.dtype, device=dev) for k, t in rows.items()}
        out_c = {k: torch.empty((B,) + tuple(t.shape[1:]), dtype=t.dtype, device=dev) for k, t in compact.items()}
        exp = [torch.empty((B, N, L), device=dev) for _ in range(2)]
        sample_bytes = B * N * (2 * 4 * L + 12) + 8 * B
        src = torch.empty(sample_bytes // 2, dtype=u8, device=dev)
        dst = torch.empty_like(src)

        def push():
            ring.push(obs_c, acts, traj, masks_next=masks.view(1, E, N))

        def sample():
            ring.sample(B, out=mb)

        def rows_ring():
            torch.randint(0, R, (B,), out=idx)
            for k, t in rows.items():
                torch.index_select(t, 0, idx, out=out_rows[k])

        def compact_ring():
            torch.randint(0, R, (B,), out=idx)
            for k, t in compact.items():
                torch.index_select(t, 0, idx, out=out_c[k])
            env.expand_observations(out_c["obs"], out=exp[0])
            env.expand_observations(out_c["next_obs"], out=exp[1])

        bodies = {"push": push, "slices": lambda: slices(0), "sample": sample, "rows ring": rows_ring, "compact ring": compact_ring,
                  "copy": lambda: dst.copy_(src)}
        # the yardsticks move the same things: a sample equals the gather of its own indices from either ring
        sample()
        side.synchronize()
        at = mb.index
        assert int(at.min()) >= 0 and int(at.max()) < R
        assert torch.equal(mb.obs, rows["obs"][at]) and torch.equal(mb.next_obs, rows["next_obs"][at])
        assert torch.equal(mb.obs, env.expand_observations(ring.obs_c[at])) and torch.equal(mb.masks_next, rows["masks_next"][at])
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
        sizes = (ring.nbytes, ring.rows_form_nbytes(), sample_bytes)
    env.use_stream(None)
    env.close()
    return times, sizes


def cell(v):
    return f"{statistics.median(v):.1f} ({min(v):.1f} .. {max(v):.1f})"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", type=Path, default=ROOT / "profiles" / "replay_timing.txt")
    args = ap.parse_args()
    sys.path.insert(0, str(ROOT))
    import bench
    import torch

    assert torch.cuda.is_available(), "this is a measurement on the GPU"
    lines = [f"# {torch.cuda.get_device_name(0)}; us per call, median of {REPEATS} alternating repeats (min .. max); a repeat = replays of a "
             f"graph of several calls between two synchronisations",
             "# push: ReplayRing.push of one step; slices: the seven slice copies and two torch.where of examples/dqn_two_policies.py's",
             "# actor_step into a row-form ring; sample: ReplayRing.sample; (a) torch.randint + seven index_select on the row-form ring;",
             "# (b) the same on compact arrays + two expand_observations; (c) a torch copy of the bytes sample writes (half in, half out)"]
    cols = ("push", "slices", "sample", "rows ring", "compact ring", "copy")
    names = {"rows ring": "(a) rows ring", "compact ring": "(b) compact ring", "copy": "(c) copy"}
    head = (f"{'shape':<14}{'S':>4}{'B':>6}{'ring MB':>10}{'rows MB':>10}{'batch MB':>10}" + "".join(f"{names.get(c, c):>26}" for c in cols)
            + f"{'push/slices':>13}{'sample/(a)':>12}{'sample/(b)':>12}{'sample/(c)':>12}")
    lines.append(head)
    print("\n".join(lines), flush=True)
    for workload, label, S, B, calls, replays in SHAPES:
        cfg, E = bench.workload_config(workload)
        t, (ring_b, rows_b, batch_b) = measure(cfg, E, S, B, calls, replays)
        med = {k: statistics.median(v) for k, v in t.items()}
        row = f"{label:<14}{S:>4}{B:>6}{ring_b / 1e6:>10.1f}{rows_b / 1e6:>10.1f}{batch_b / 1e6:>10.2f}" + "".join(f"{cell(t[c]):>26}" for c in cols)
        row += f"{med['push'] / med['slices']:>13.4f}{med['sample'] / med['rows ring']:>12.4f}{med['sample'] / med['compact ring']:>12.4f}"
        row += f"{med['sample'] / med['copy']:>12.4f}"
        lines.append(row)
        print(row, flush=True)
    args.out.parent.mkdir(parents=True, exist_ok=True)
    args.out.write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
