#!/usr/bin/env python3
"""Device time of a step that also hands out the legal-action masks, from replayed HIP graphs, in ONE process so that
every variant sees the same machine: plain `step` as the floor, (a) `step` + `action_masks()` -- two dependent launches
--, (b) `step(want_masks=True)` -- the step's own launch writes them.  Full outputs (observation rows, rewards, flag
bytes).  The protocol of mixed_step_timing.py: each graph holds 20 steps; a repeat replays it 25 times between two
synchronisations (500 steps, a few ms); the variants alternate over 15 repeats and the median per variant is reported,
with the spread.

With `--parent TREE` (a built checkout of the commit before the masks) plain `step` is also timed against that build:
child processes of this script, this tree and that one in turn, three times each, every child timing plain `step` alone
with the same protocol.

    python profiles/action_mask_timing.py [--parent TREE] > profiles/action_mask_timing.txt
"""

import argparse
import json
import statistics
import subprocess
import sys
import time
from pathlib import Path

STEPS, REPLAYS, REPEATS = 20, 25, 15
SHAPES = [("C2", "c2", 4096), ("C3", "c3", 4096), ("C5-64", "c5_64", 1024)]
VARIANTS = ("step", "composition", "fused")


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
            acts = torch.randint(0, 5, (E, env.num_agents), dtype=torch.uint8, device=env.device)
            masks = torch.empty_like(acts)

            def body(env=env, name=name, acts=acts, masks=masks):
                if name == "step":
                    env.step(acts)
                elif name == "composition":
                    env.step(acts)
                    env.action_masks(out=masks)
                else:
                    env.step(acts, want_masks=True)

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
                envs[name].reset_from_pool()
                side.synchronize()
                t0 = time.perf_counter()
                for _ in range(REPLAYS):
                    g.replay()
                side.synchronize()
                times[name].append((time.perf_counter() - t0) / (REPLAYS * STEPS) * 1e6)
    for env in envs.values():
        env.close()
    return times


def cell(v):
    return f"{statistics.median(v):.2f} ({min(v):.2f} .. {max(v):.2f})"


def plain_only():
    """Child mode: plain `step` of the tree this process imports, one JSON line."""
    import bench
    out = {}
    for label, wl, E in SHAPES:
        cfg, _ = bench.workload_config(wl)
        out[label] = graphs_for(cfg, E, ("step",))["step"]
    print(json.dumps(out))


def against_parent(parent: Path):
    here = Path(__file__).resolve().parent.parent
    runs = {"this": {s[0]: [] for s in SHAPES}, "parent": {s[0]: [] for s in SHAPES}}
    for _ in range(3):
        for which, root in (("this", here), ("parent", parent)):      # fresh processes, the two builds in turn
            r = subprocess.run([sys.executable, str(Path(__file__).resolve()), "--plain-only", "--root", str(root)],
                               check=True, capture_output=True, text=True, timeout=300)
            for k, v in json.loads(r.stdout.strip().splitlines()[-1]).items():
                runs[which][k] += v
    print(f"\n# plain step, this build against the build of the parent commit: 3 processes each, in turn, {REPEATS} repeats per process")
    print(f"{'shape':<8}{'this build':>26}{'parent build':>26}{'difference of medians':>24}")
    for label, _, _ in SHAPES:
        a, b = runs["this"][label], runs["parent"][label]
        print(f"{label:<8}{cell(a):>26}{cell(b):>26}{statistics.median(a) - statistics.median(b):>24.3f}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", type=Path, default=None)
    ap.add_argument("--plain-only", action="store_true")
    ap.add_argument("--root", type=Path, default=Path(__file__).resolve().parent.parent)
    args = ap.parse_args()
    sys.path.insert(0, str(args.root))
    import torch

    assert torch.cuda.is_available(), "this is a measurement on the GPU"
    if args.plain_only:
        return plain_only()
    import bench
    print(f"# {torch.cuda.get_device_name(0)}; us per step, median of {REPEATS} repeats of {REPLAYS} replays of a {STEPS}-step graph "
          f"(min .. max); full outputs")
    print(f"{'shape':<8}{'E x N':>12}{'plain step':>24}{'step + action_masks (a)':>28}{'step(want_masks) (b)':>26}"
          f"{'(a) - (b)':>11}{'(b) - step':>12}{'spread (b)':>12}")
    for label, wl, E in SHAPES:
        cfg, _ = bench.workload_config(wl)
        t = graphs_for(cfg, E, VARIANTS)
        med = {k: statistics.median(v) for k, v in t.items()}
        N = cfg.num_boarding_agents + cfg.num_exiting_agents
        spread = max(max(t[k]) - min(t[k]) for k in ("composition", "fused"))
        print(f"{label:<8}{f'{E} x {N}':>12}{cell(t['step']):>24}{cell(t['composition']):>28}{cell(t['fused']):>26}"
              f"{med['composition'] - med['fused']:>11.2f}{med['fused'] - med['step']:>12.2f}{spread:>12.2f}", flush=True)
    if args.parent is not None:
        against_parent(args.parent)


if __name__ == "__main__":
    main()
