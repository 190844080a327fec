#!/usr/bin/env python3
"""Device time of `ccx_gae` (advantages and returns from a trajectory, include/ccx.h CCX_GAE) from replayed HIP graphs, in
ONE process so that every variant sees the same machine.  Per shape:

  gae               the kernel without final_values (a cut bootstraps from 0), with `valid`
  gae + final       the kernel with final_values (one more load at every cut step)
  (a) producer      the launch it follows: `rollout(K, auto_reset)` with full outputs
  (b) torch eager   the same rule as a reverse loop over the steps of elementwise torch calls (f32, `torch.where` selects),
                    launched call by call
  (c) torch graph   the same loop captured and replayed: THE YARDSTICK (what a user writes today, at its best)
  (d) copy          `torch.Tensor.copy_` of as many bytes as the kernel with final_values moves (reads + writes, half in,
                    half out): the streaming yardstick

The protocol of episode_stats_timing.py: a graph holds CALLS calls; a repeat replays it REPLAYS times between two
synchronisations; the variants alternate over 15 repeats; the median is reported with min .. max.  The trajectory is a
real one (random actions, auto-reset), the values are random.

    python profiles/gae_timing.py [--out profiles/gae_timing.txt] [--label default]

`--label` names the build in the table (the default library, or a `make variant` build loaded through CCX_DIAG_LIB with
another CCX_GAE_CHUNK / CCX_GAE_LANES); `--kernel-only` measures the two kernel columns alone (for such builds).
"""

import argparse
import os
import statistics
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
REPEATS = 15
# label, workload, E, K, calls per graph, replays per repeat
SHAPES = [("C2 K=500", "c2", 4096, 500, 2, 5), ("C2 K=16", "c2", 4096, 16, 10, 10), ("C3 K=64", "c3", 4096, 64, 2, 5)]
GAMMA, LAM = 0.99, 0.95


def torch_gae(reward, af, ef, values, last_values, final_values, adv, ret, valid):
    """(b) / (c): the rule of include/ccx.h as a user writes it with torch alone -- K reverse iterations of elementwise calls."""
    import torch

    K = reward.shape[0]
    g, gl = GAMMA, GAMMA * LAM
    zero = torch.zeros_like(last_values)
    carry = zero
    for s in range(K - 1, -1, -1):
        a, e = af[s], ef[s][:, None]
        live = (a & 4) != 0
        term = (a & 1) != 0
        cut = ((a & 2) != 0) | ((e & 7) != 0)
        nxt = last_values if s == K - 1 else values[s + 1]
        boot = zero if final_values is None else final_values[s]
        nv = torch.where(term, zero, torch.where(cut, boot, nxt))
        c = torch.where(term | cut, zero, carry)
        v = values[s]
        delta = (reward[s].float() + g * nv) - v
        x = delta + gl * c
        carry = torch.where(live, x, zero)
        adv[s] = carry
        ret[s] = torch.where(live, x + v, zero)
        valid[s] = live
    return adv


def measure(label, wl, E, K, calls, replays, kernel_only):
    import bench
    import torch

    from collectivecrossing_amd import BatchedCollectiveCrossing
    cfg, _ = bench.workload_config(wl)
    side = torch.cuda.Stream()
    graphs = {}
    with torch.cuda.stream(side):
        env = BatchedCollectiveCrossing(cfg, E)
        env.use_stream(side)
        env.make_reset_pool(0, 1024)
        env.reset_from_pool()
        N = env.num_agents
        acts = torch.randint(0, 5, (K, E, N), dtype=torch.uint8, device=env.device)
        traj = env.alloc_rollout(K)
        env.rollout(acts, auto_reset=True, out=traj)              # eager first: buffers, pace calibration, and the data
        side.synchronize()
        reward, af, ef = traj.reward.clone(), traj.agent_flags.clone(), traj.env_flags.clone()
        values = torch.randn((K, E, N), device=env.device)
        final_values = torch.randn((K, E, N), device=env.device)
        last_values = torch.randn((E, N), device=env.device)
        out = env.alloc_gae(K)
        t_adv, t_ret, t_valid = torch.empty_like(out.advantages), torch.empty_like(out.returns), torch.empty_like(out.valid, dtype=torch.bool)
        nbytes = reward.numel() * (8 + 1 + 4 + 4 + 4 + 1) + ef.numel() + last_values.numel() * 4     # without final_values
        cuts = int((((af & 2) != 0) | ((ef[..., None] & 7) != 0)).sum())
        src = torch.empty((nbytes + 4 * cuts) // 2, dtype=torch.uint8, device=env.device)
        dst = torch.empty_like(src)
        bodies = {
            "gae": lambda: env.compute_gae((reward, af, ef), values, last_values, None, GAMMA, LAM, out=out),
            "gae + final": lambda: env.compute_gae((reward, af, ef), values, last_values, final_values, GAMMA, LAM, out=out),
        }
        if not kernel_only:
            bodies.update({
                "producer": lambda: env.rollout(acts, auto_reset=True, out=traj),
                "torch graph": lambda: torch_gae(reward, af, ef, values, last_values, final_values, t_adv, t_ret, t_valid),
                "copy": lambda: dst.copy_(src),
            })
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
        if not kernel_only:
            times["torch eager"] = []
        for _ in range(REPEATS):
            for name, g in graphs.items():                          # alternate the variants
                side.synchronize()
                t0 = time.perf_counter()
                for _ in range(replays):
                    g.replay()
                side.synchronize()
                times[name].append((time.perf_counter() - t0) / (replays * calls) * 1e6)
            if not kernel_only:
                side.synchronize()
                t0 = time.perf_counter()
                torch_gae(reward, af, ef, values, last_values, final_values, t_adv, t_ret, t_valid)
                side.synchronize()
                times["torch eager"].append((time.perf_counter() - t0) * 1e6)
        # the torch loop computes the rule (to rounding: it is free to fuse): a wrong yardstick would be no yardstick
        if not kernel_only:
            bodies["gae + final"]()
            side.synchronize()
            live = (af & 4) != 0
            err = (t_adv - out.advantages)[live].abs().max().item()
            scale = out.advantages[live].abs().max().item()
            assert err <= 1e-4 * max(scale, 1.0), (err, scale)
    env.close()
    return times, N, nbytes, cuts


def cell(v):
    return f"{statistics.median(v):.1f} ({min(v):.1f} .. {max(v):.1f})"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", type=Path, default=ROOT / "profiles" / "gae_timing.txt")
    ap.add_argument("--label", default="default")
    ap.add_argument("--kernel-only", action="store_true")
    args = ap.parse_args()
    sys.path.insert(0, str(ROOT))
    if os.environ.get("CCX_DIAG_LIB"):                             # an experimental build of libccx (make variant)
        from collectivecrossing_amd import _lib
        _lib.LIB_PATH = Path(os.environ["CCX_DIAG_LIB"]).resolve()
    import torch

    assert torch.cuda.is_available(), "this is a measurement on the GPU"
    lines = [f"# {torch.cuda.get_device_name(0)}; build: {args.label}; us per call, median of {REPEATS} alternating repeats (min .. max); a repeat = "
             f"replays of a graph of several calls between two synchronisations (torch eager: one loop per repeat, host-timed)",
             "# gae: ccx_gae without final_values; + final: with; (a) the rollout launch it follows (full outputs); (b) / (c) the same rule",
             "# as a reverse torch loop, eager / captured; (d) a torch copy of the kernel's bytes (reads + writes)"]
    cols = ("gae", "gae + final") if args.kernel_only else ("gae", "gae + final", "producer", "torch eager", "torch graph", "copy")
    names = {"producer": "(a) producer", "torch eager": "(b) torch eager", "torch graph": "(c) torch graph", "copy": "(d) copy"}
    head = f"{'shape':<10}{'E x N':>10}{'MB moved':>10}{'cut steps':>11}" + "".join(f"{names.get(c, c):>30}" for c in cols)
    head += "" if args.kernel_only else f"{'gae/(c)':>10}{'gae/(a)':>10}{'GB/s':>8}"
    lines.append(head)
    print("\n".join(lines), flush=True)
    for label, wl, E, K, calls, replays in SHAPES:
        t, N, nbytes, cuts = measure(label, wl, E, K, calls, replays, args.kernel_only)
        med = {k: statistics.median(v) for k, v in t.items()}
        row = f"{label:<10}{f'{E} x {N}':>10}{nbytes / 1e6:>10.1f}{cuts:>11}" + "".join(f"{cell(t[c]):>30}" for c in cols)
        if not args.kernel_only:
            row += f"{med['gae'] / med['torch graph']:>10.4f}{med['gae'] / med['producer']:>10.3f}{nbytes / med['gae'] / 1e3:>8.0f}"
        lines.append(row)
        print(row, flush=True)
    args.out.parent.mkdir(parents=True, exist_ok=True)
    args.out.write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
