#!/usr/bin/env python3
"""Device time of `ccx_episode_stats_update` (episode returns and lengths from a trajectory, include/ccx.h
CCX_EPISODE_STATS) from replayed HIP graphs, in ONE process so that every variant sees the same machine.  Per shape:

  update            the update without a log (one launch)
  update + log      with a finished-episode log (three launches + the 16-byte memset of `clear_episode_log`, so that the
                    log never fills and every record is written on every replay)
  one load/step     the accumulate kernel with ONE dependent load per step (tunable "stats_naive"), no log: what the
                    pipelined loads are measured against.  At K = 1 both variants take the kernel's single-step branch:
                    the column is the same code path there, and a difference in it is register allocation or noise
  (a) producer      the launch the update follows: `rollout(K, auto_reset)` with full outputs, or `step` for K = 1
  (b) stream read   `reward.sum()` + sums over the two flag arrays: a pure streaming read of the same bytes
  (c) torch         the composition a user writes today: masked `cumsum` over the steps with segment resets at the
                    finished steps (K = 1: the elementwise running-sum update).  It reassociates the sum (not bit-exact)
                    and knows nothing of the latch or of a carry-in from the call before.

The protocol of action_mask_timing.py: a graph holds CALLS calls; a repeat replays it REPLAYS times between two
synchronisations; the variants alternate over 15 repeats; the median is reported with min .. max.

    python profiles/episode_stats_timing.py [--out profiles/episode_stats_timing.txt]
"""

import argparse
import statistics
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
REPEATS = 15
# label, workload, E, K, calls per graph, replays per repeat
SHAPES = [("C2 K=500", "c2", 4096, 500, 2, 5), ("C3 K=64", "c3", 4096, 64, 2, 5), ("C2 K=1", "c2", 4096, 1, 20, 25)]
VARIANTS = ("update", "update + log", "one load/step", "producer", "stream read", "torch")


def torch_composition(reward, af, ef, state):
    """(c): what a user of the library writes today with torch alone."""
    import torch

    live = (af & 4) != 0
    r = torch.where(live, reward, 0.0)
    done = (ef & 3) != 0
    K = reward.shape[0]
    if K == 1:                                   # the step-wise loop: running sums carried in `state`
        state["ret"] += r[0]
        state["steps"] += 1
        d = done[0]
        state["last_ret"] = torch.where(d[:, None], state["ret"], state["last_ret"])
        state["last_steps"] = torch.where(d, state["steps"], state["last_steps"])
        reset = (ef[0] & 4) != 0
        state["ret"] = torch.where(reset[:, None], 0.0, state["ret"])
        state["steps"] = torch.where(reset, 0, state["steps"])
        return state["last_ret"]
    cs = r.cumsum(0)                                                        # [K, E, N], a tree / blocked scan
    steps = torch.arange(K, device=reward.device)[:, None].expand(K, ef.shape[1])
    ended_before = torch.zeros_like(done)
    ended_before[1:] = done[:-1]
    start = torch.cummax(torch.where(ended_before, steps, 0), 0).values     # first step of the episode step s belongs to
    base = torch.where((start > 0)[..., None], cs.gather(0, (start - 1).clamp(min=0)[..., None].expand_as(cs)), 0.0)
    ep_ret = cs - base                                                      # return of the episode so far, at every step
    n = done.sum().clamp(min=1)
    mean_ret = (ep_ret * done[..., None]).sum((0, 1)) / n                   # per agent slot, over the finished episodes
    mean_len = ((steps - start + 1) * done).sum() / n
    return mean_ret, mean_len


def measure(label, wl, E, K, calls, replays):
    import bench
    import torch

    from collectivecrossing_amd import BatchedCollectiveCrossing
    cfg, _ = bench.workload_config(wl)
    side = torch.cuda.Stream()
    graphs, keep = {}, []
    with torch.cuda.stream(side):
        def make(log_capacity=None, naive=False):
            env = BatchedCollectiveCrossing(cfg, E)
            env.use_stream(side)
            env.make_reset_pool(0, 1024)
            env.reset_from_pool()
            if naive:
                env.set_tunable("stats_naive", 1)
            keep.append(env)
            return env

        prod = make()
        N = prod.num_agents
        acts = torch.randint(0, 5, (K, E, N), dtype=torch.uint8, device=prod.device)
        traj = prod.alloc_rollout(K) if K > 1 else None
        if K > 1:
            prod.rollout(acts, auto_reset=True, out=traj)          # eager first: buffers, pace calibration, and the data
            reward, af, ef = traj.reward, traj.agent_flags, traj.env_flags
        else:
            prod.rollout(acts.expand(25, E, N).contiguous(), auto_reset=True, want_obs=False)   # somewhere inside episodes
            r1 = prod.step(acts[0])
            reward, af, ef = r1.reward[None], r1.agent_flags[None], r1.env_flags[None]
        side.synchronize()
        plain, logged, naive = make(), make(), make(naive=True)
        plain.track_episodes(0)
        naive.track_episodes(0)
        logged.track_episodes(1 << 18)
        state = dict(ret=torch.zeros((E, N), dtype=torch.float64, device=prod.device),
                     steps=torch.zeros(E, dtype=torch.int32, device=prod.device),
                     last_ret=torch.zeros((E, N), dtype=torch.float64, device=prod.device),
                     last_steps=torch.zeros(E, dtype=torch.int32, device=prod.device))

        def with_log():
            logged.clear_episode_log()
            logged.update_episode_stats(reward, af, ef)

        bodies = {
            "update": lambda: plain.update_episode_stats(reward, af, ef),
            "update + log": with_log,
            "one load/step": lambda: naive.update_episode_stats(reward, af, ef),
            "producer": (lambda: prod.rollout(acts, auto_reset=True, out=traj)) if K > 1 else (lambda: prod.step(acts[0])),
            "stream read": lambda: (reward.sum(), af.sum(dtype=torch.int64), ef.sum(dtype=torch.int64)),
            "torch": lambda: torch_composition(reward, af, ef, state),
        }
        for name in VARIANTS:
            bodies[name]()                                          # warm-up: code objects, allocator blocks
            side.synchronize()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, stream=side):
                for _ in range(calls):
                    bodies[name]()
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
        side.synchronize()
        rec = logged.finished_episodes(clear=False)
        nbytes = reward.numel() * 9 + ef.numel()
    for env in keep:
        env.close()
    return times, N, nbytes, len(rec)


def cell(v):
    return f"{statistics.median(v):.2f} ({min(v):.2f} .. {max(v):.2f})"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", type=Path, default=ROOT / "profiles" / "episode_stats_timing.txt")
    args = ap.parse_args()
    sys.path.insert(0, str(ROOT))
    import torch

    assert torch.cuda.is_available(), "this is a measurement on the GPU"
    lines = [f"# {torch.cuda.get_device_name(0)}; us per call, median of {REPEATS} alternating repeats (min .. max); a repeat = "
             f"replays of a graph of several calls between two synchronisations (C2 K=500 / C3 K=64: 5 x 2 calls, K=1: 25 x 20)",
             "# update: ccx_episode_stats_update without a log (1 launch); + log: 3 launches + a 16-byte memset (log cleared per call);",
             "# one load/step: the accumulate kernel without pipelined loads (tunable stats_naive), no log;",
             "# (a) the launch the update follows (rollout with full outputs / step); (b) reward.sum() + flag sums; (c) torch cumsum composition"]
    head = (f"{'shape':<10}{'E x N':>10}{'MB read':>9}{'records':>9}{'update':>24}{'update + log':>26}{'one load/step':>28}"
            f"{'(a) producer':>28}{'(b) stream read':>26}{'(c) torch':>30}{'update/(a)':>12}{'GB/s':>8}")
    lines.append(head)
    print("\n".join(lines), flush=True)
    for label, wl, E, K, calls, replays in SHAPES:
        t, N, nbytes, records = measure(label, wl, E, K, calls, replays)
        med = {k: statistics.median(v) for k, v in t.items()}
        row = (f"{label:<10}{f'{E} x {N}':>10}{nbytes / 1e6:>9.1f}{records:>9}{cell(t['update']):>24}{cell(t['update + log']):>26}"
               f"{cell(t['one load/step']):>28}{cell(t['producer']):>28}{cell(t['stream read']):>26}{cell(t['torch']):>30}"
               f"{med['update'] / med['producer']:>12.3f}{nbytes / med['update'] / 1e3:>8.0f}")
        lines.append(row)
        print(row, flush=True)
    args.out.parent.mkdir(parents=True, exist_ok=True)
    args.out.write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
