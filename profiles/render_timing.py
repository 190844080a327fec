"""Time ccx_render: microseconds per launch and GB/s of frames written (not part of bench.py).

    python profiles/render_timing.py

Shapes: 4096 x C2 (12 x 8) at cell_px 8 (~75 MB), 256 x 100 x 100 at cell_px 4 (~123 MB), and one
CollectiveCrossingEnv.render() (C2, 800 x 1200 figure, device frame + copy to the host).  Each figure is the median of
CCX_RENDER_REPEATS (default 20) launches timed with HIP events after 3 warm-up launches.  Write peak of the MI355X: 8 TB/s.
"""

from __future__ import annotations

import json
import os
import sys
import time
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

from collectivecrossing_amd import CollectiveCrossingEnv  # noqa: E402
from collectivecrossing_amd.batched import BatchedCollectiveCrossing  # noqa: E402
from collectivecrossing_amd.configs import CollectiveCrossingConfig, MaxStepsTruncatedConfig  # noqa: E402

PEAK_GBS = 8000.0
REPEATS = int(os.environ.get("CCX_RENDER_REPEATS", "20"))


def c2():
    return CollectiveCrossingConfig(width=12, height=8, division_y=4, tram_door_left=5, tram_door_right=7, tram_length=9,
                                    num_boarding_agents=5, num_exiting_agents=3, exiting_destination_area_y=0,
                                    boarding_destination_area_y=8, truncated_config=MaxStepsTruncatedConfig(max_steps=100))


def big():
    return CollectiveCrossingConfig(width=100, height=100, division_y=50, tram_door_left=20, tram_door_right=26,
                                    tram_length=60, num_boarding_agents=30, num_exiting_agents=20,
                                    exiting_destination_area_y=5, boarding_destination_area_y=90,
                                    truncated_config=MaxStepsTruncatedConfig(max_steps=100))


def time_batch(name, cfg, E, cp):
    env = BatchedCollectiveCrossing(cfg, E, device="cuda:0")
    env.make_reset_pool(1, 256)
    env.reset_from_pool()
    out = torch.empty((E, *env.frame_shape(cp)), dtype=torch.uint8, device=env.device)
    for _ in range(3):
        env.render(cell_px=cp, out=out)
    torch.cuda.synchronize()
    times = []
    for _ in range(REPEATS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        env.render(cell_px=cp, out=out)
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b) * 1e3)
    us = float(np.median(times))
    gbs = out.numel() / us / 1e3
    env.close()
    return {"shape": name, "envs": E, "cell_px": cp, "bytes": out.numel(), "us_per_launch": round(us, 2),
            "gb_per_s": round(gbs, 1), "of_write_peak": round(gbs / PEAK_GBS, 3)}


def time_env_render():
    env = CollectiveCrossingEnv(config=c2())
    env.reset(seed=0)
    for _ in range(3):
        env.render()
    times = []
    for _ in range(REPEATS):
        t = time.perf_counter()
        env.render()
        times.append((time.perf_counter() - t) * 1e6)
    env.close()
    return {"shape": "env.render() C2 800x1200", "us_per_call": round(float(np.median(times)), 1)}


def main():
    for rec in (time_batch("C2 12x8", c2(), 4096, 8), time_batch("100x100 N=50", big(), 256, 4), time_env_render()):
        print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
