#!/usr/bin/env python3
"""Device time of a step loop that feeds `out.obs` back into a policy, with the rows of restarted envs being those of the
NEW episode (`reset_obs="next"`, include/ccx.h: CCX_RESET_OBS), from replayed HIP graphs, in ONE process so that every
variant sees the same machine.  K = 1 `rollout(auto_reset=True)` with full outputs, max_steps = 100:
  (a) terminal   today's default rows;
  (c) fused      `reset_obs="next"`, the step's own launch redirects the rows;
  (d) fixup      `reset_obs="next"` through the stand-alone fix-up kernel (tunable reset_obs_fused = 0): two launches;
  (e) workaround `rollout` + `observe()` + `torch.where` on EF_RESET: what a caller had to do before.
The protocol of action_mask_timing.py: each graph holds 20 steps; a repeat replays it 25 times between two
synchronisations; the variants alternate over 15 repeats and the median per variant is reported, with the spread.
Rollout rows: one K = 500 rollout with and without the fix-up kernel behind it, eager, same alternation.

With `--parent TREE` (a built checkout of the parent commit) (b) the TERMINAL-mode step is also timed against that build:
child processes of this script, this tree and that one in turn, three times each.

    python profiles/reset_obs_timing.py [--parent TREE] > profiles/reset_obs_timing.txt
"""

import argparse
import json
import statistics
import subprocess
import sys
import time
from pathlib import Path

STEPS, REPLAYS, REPEATS = 20, 25, 15
SHAPES = [("C2", "c2", 4096), ("C3", "c3", 4096)]
VARIANTS = ("terminal", "fused", "fixup", "workaround")
ROLLOUT_K = 500


def config_for(wl):
    import bench

    from collectivecrossing_amd.configs import MaxStepsTruncatedConfig
    cfg, _ = bench.workload_config(wl)
    return cfg.model_copy(update=dict(truncated_config=MaxStepsTruncatedConfig(max_steps=100)))


def graphs_for(cfg, E, variants):
    """One handle per variant, all of the same shape on one side stream, one graph of STEPS steps each."""
    import torch

    from collectivecrossing_amd import BatchedCollectiveCrossing
    side = torch.cuda.Stream()
    envs, graphs = {}, {}
    with torch.cuda.stream(side):
        for name in variants:
            env = BatchedCollectiveCrossing(cfg, E)
            env.use_stream(side)
            env.make_reset_pool(0, 1024)
            env.reset_from_pool()
            # (episodes staggered over their length, so that every step sees its share of restarts: ~1 % of the envs)
            env.set_state(step_count=(torch.arange(E) % 100).to(torch.int32).numpy())
            acts = torch.randint(0, 5, (1, E, env.num_agents), dtype=torch.uint8, device=env.device)
            out = env.alloc_rollout(1)
            obs = torch.empty_like(out.obs[0])
            if name == "fixup":
                env.set_tunable("reset_obs_fused", 0)

            def body(env=env, name=name, acts=acts, out=out, obs=obs):
                if name == "terminal":
                    env.rollout(acts, auto_reset=True, out=out)
                elif name in ("fused", "fixup"):
                    env.rollout(acts, auto_reset=True, out=out, reset_obs="next")
                else:
                    env.rollout(acts, auto_reset=True, out=out)
                    env.observe(out=obs)
                    torch.where((out.env_flags[0] & 4).ne(0)[:, None, None], obs, out.obs[0], out=obs)

            body()                                    # warm-up: output buffers, code objects
            side.synchronize()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, stream=side):
                for _ in range(STEPS):
                    body()
            for _ in range(3):
                g.replay()
            side.synchronize()
            envs[name], graphs[name] = env, g
        times = {k: [] for k in graphs}
        for _ in range(REPEATS):
            for name, g in graphs.items():            # alternate the variants
                side.synchronize()
                t0 = time.perf_counter()
                for _ in range(REPLAYS):
                    g.replay()
                side.synchronize()
                times[name].append((time.perf_counter() - t0) / (REPLAYS * STEPS) * 1e6)
    for env in envs.values():
        env.close()
    return times


def rollouts_for(cfg, E):
    """One K = 500 rollout with full outputs: TERMINAL rows, and NEXT rows (the fix-up kernel behind the launch); ms."""
    import torch

    from collectivecrossing_amd import BatchedCollectiveCrossing
    env = BatchedCollectiveCrossing(cfg, E)
    env.make_reset_pool(0, 1024)
    env.reset_from_pool()
    acts = torch.randint(0, 5, (ROLLOUT_K, E, env.num_agents), dtype=torch.uint8, device=env.device)
    out = env.alloc_rollout(ROLLOUT_K)
    times = {"terminal": [], "next": []}
    for rep in range(REPEATS + 3):                    # (three warm-up rounds: the pace controller settles)
        for mode in times:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            env.rollout(acts, auto_reset=True, out=out, reset_obs=mode)
            torch.cuda.synchronize()
            if rep >= 3:
                times[mode].append((time.perf_counter() - t0) * 1e3)
    share = float((out.env_flags & 4).ne(0).float().mean())
    env.close()
    return times, share


def cell(v):
    return f"{statistics.median(v):.2f} ({min(v):.2f} .. {max(v):.2f})"


def terminal_only():
    """Child mode: the TERMINAL-mode step of the tree this process imports, one JSON line."""
    out = {}
    for label, wl, E in SHAPES:
        out[label] = graphs_for(config_for(wl), E, ("terminal",))["terminal"]
    print(json.dumps(out))


def against_parent(parent: Path):
    here = Path(__file__).resolve().parent.parent
    runs = {"this": {s[0]: [] for s in SHAPES}, "parent": {s[0]: [] for s in SHAPES}}
    for _ in range(3):
        for which, root in (("this", here), ("parent", parent)):      # fresh processes, the two builds in turn
            r = subprocess.run([sys.executable, str(Path(__file__).resolve()), "--terminal-only", "--root", str(root)],
                               check=True, capture_output=True, text=True, timeout=300)
            for k, v in json.loads(r.stdout.strip().splitlines()[-1]).items():
                runs[which][k] += v
    print(f"\n# TERMINAL-mode step, this build (a') against the build of the parent commit (b): 3 processes each, in turn, "
          f"{REPEATS} repeats per process")
    print(f"{'shape':<8}{'this build':>26}{'parent build (b)':>26}{'difference of medians':>24}")
    for label, _, _ in SHAPES:
        a, b = runs["this"][label], runs["parent"][label]
        print(f"{label:<8}{cell(a):>26}{cell(b):>26}{statistics.median(a) - statistics.median(b):>24.3f}", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", type=Path, default=None)
    ap.add_argument("--terminal-only", action="store_true")
    ap.add_argument("--root", type=Path, default=Path(__file__).resolve().parent.parent)
    args = ap.parse_args()
    sys.path.insert(0, str(args.root))
    import torch

    assert torch.cuda.is_available(), "this is a measurement on the GPU"
    if args.terminal_only:
        return terminal_only()
    print(f"# {torch.cuda.get_device_name(0)}; us per step, median of {REPEATS} repeats of {REPLAYS} replays of a {STEPS}-step graph "
          f"(min .. max); K = 1 rollout(auto_reset), full outputs, max_steps = 100")
    print(f"{'shape':<7}{'E x N':>10}{'terminal (a)':>22}{'next, fused (c)':>22}{'next, fix-up (d)':>22}{'workaround (e)':>22}"
          f"{'(d) - (c)':>10}{'(c) - (a)':>10}{'spread':>8}")
    for label, wl, E in SHAPES:
        cfg = config_for(wl)
        t = graphs_for(cfg, E, VARIANTS)
        med = {k: statistics.median(v) for k, v in t.items()}
        N = cfg.num_boarding_agents + cfg.num_exiting_agents
        spread = max(max(t[k]) - min(t[k]) for k in ("fused", "fixup"))
        print(f"{label:<7}{f'{E} x {N}':>10}{cell(t['terminal']):>22}{cell(t['fused']):>22}{cell(t['fixup']):>22}"
              f"{cell(t['workaround']):>22}{med['fixup'] - med['fused']:>10.2f}{med['fused'] - med['terminal']:>10.2f}{spread:>8.2f}",
              flush=True)
    print(f"\n# one K = {ROLLOUT_K} rollout(auto_reset), full outputs, eager; ms, median of {REPEATS} alternating repeats (min .. max)")
    print(f"{'shape':<7}{'E x N':>10}{'terminal rows':>26}{'next rows (+ fix-up)':>26}{'difference':>12}{'pairs with EF_RESET':>22}")
    for label, wl, E in SHAPES:
        cfg = config_for(wl)
        t, share = rollouts_for(cfg, E)
        N = cfg.num_boarding_agents + cfg.num_exiting_agents
        print(f"{label:<7}{f'{E} x {N}':>10}{cell(t['terminal']):>26}{cell(t['next']):>26}"
              f"{statistics.median(t['next']) - statistics.median(t['terminal']):>12.3f}{share:>22.4f}", flush=True)
    if args.parent is not None:
        against_parent(args.parent)


if __name__ == "__main__":
    main()
