#!/usr/bin/env python3
"""Device time of one mixed-control step, from replayed HIP graphs, in ONE process so that every variant sees the same
machine: (a) the way before `step_mixed` -- policy_actions + torch.where + step, three dependent launches --, (b)
`step_mixed`, one launch, and plain `step` of the same shape as the floor.  Full outputs (observation rows, rewards, flag
bytes).  Each graph holds 20 steps; a repeat replays it 25 times between two synchronisations (500 steps, a few ms);
the variants alternate over 15 repeats and the median per variant is reported, with the spread.

    python profiles/mixed_step_timing.py > profiles/mixed_step_timing.txt
"""

import statistics
import sys
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

import torch  # noqa: E402

import bench  # noqa: E402
from collectivecrossing_amd import BatchedCollectiveCrossing  # noqa: E402
from collectivecrossing_amd.batched import scripted_slot_mask  # noqa: E402

STEPS, REPLAYS, REPEATS = 20, 25, 15
SHAPES = [("C2", "c2", 4096, "exiting"), ("C3", "c3", 4096, "exiting"), ("C5-64", "c5_64", 1024, "all")]


def graphs_for(cfg, E, scripted):
    """Three handles of the same shape on one side stream, one graph of STEPS steps each."""
    side = torch.cuda.Stream()
    mask = scripted_slot_mask(cfg, scripted)
    envs, graphs = {}, {}
    with torch.cuda.stream(side):
        for name in ("step", "composition", "step_mixed"):
            env = BatchedCollectiveCrossing(cfg, E)
            env.use_stream(side)
            env.make_reset_pool(0, 1024)
            env.reset_from_pool()
            N = env.num_agents
            acts = torch.randint(0, 5, (E, N), dtype=torch.uint8, device=env.device)
            pa = torch.empty_like(acts)
            merged = torch.empty_like(acts)
            sel = torch.tensor([(mask >> a) & 1 for a in range(N)], dtype=torch.bool, device=env.device)

            def body(env=env, name=name, acts=acts, pa=pa, merged=merged, sel=sel):
                if name == "step":
                    env.step(acts)
                elif name == "composition":
                    env.policy_actions("greedy", out=pa)
                    torch.where(sel, pa, acts, out=merged)
                    env.step(merged)
                else:
                    env.step_mixed(acts, mask, "greedy")

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


def main():
    assert torch.cuda.is_available(), "this is a measurement on the GPU"
    print(f"# {torch.cuda.get_device_name(0)}; us per step, median of {REPEATS} repeats of {REPLAYS} replays of a {STEPS}-step graph "
          f"(min .. max); greedy policy, full outputs")
    print(f"{'shape':<8}{'E x N':>12}{'scripted':>10}{'plain step':>24}{'policy+where+step (a)':>28}{'step_mixed (b)':>24}"
          f"{'(a) - (b)':>11}{'(b) - step':>12}")
    for label, wl, E, scripted in SHAPES:
        cfg, _ = bench.workload_config(wl)
        t = graphs_for(cfg, E, scripted)
        med = {k: statistics.median(v) for k, v in t.items()}
        cell = lambda k: f"{med[k]:.2f} ({min(t[k]):.2f} .. {max(t[k]):.2f})"  # noqa: E731
        N = cfg.num_boarding_agents + cfg.num_exiting_agents
        print(f"{label:<8}{f'{E} x {N}':>12}{scripted:>10}{cell('step'):>24}{cell('composition'):>28}{cell('step_mixed'):>24}"
              f"{med['composition'] - med['step_mixed']:>11.2f}{med['step_mixed'] - med['step']:>12.2f}", flush=True)


if __name__ == "__main__":
    main()
