"""HBM traffic of the two split-step kernels from hardware counters (not part of bench.py).

    bash profiles/collect_array_pmc.sh      -> profiles/array_strategies_pmc.txt

Run WITHOUT arguments this is the profiled workload: 4096 envs of the C2 geometry with the built-in rules, 40 times
step_begin + step_finish(auto_reset=True) with observation rows.  The collect script runs it twice under
`rocprofv3 --pmc` (FETCH_SIZE, then WRITE_SIZE: counters only, one pass each, no tracing) and then calls
`--summarise DIR OUT`: the mean over the last 20 dispatches of each kernel, next to the algorithmic bytes."""

from __future__ import annotations

import csv
import glob
import json
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
E, N, L, STEPS = 4096, 8, 38, 40
# per agent slot: begin reads x, y, active, action and writes x, y, active; finish reads x, y and the three flag bytes and
# writes the row, the f64 reward, the flag byte, term_present and the two state flags (+ a few bytes per env: counters,
# step_count, env flag; the cell word comes from an 11 KB table that stays in cache)
ALGORITHMIC = {"step_begin_kernel": {"read": E * N * 10 + E * 4, "written": E * N * 9 + E * 4},
               "step_finish_kernel": {"read": E * N * 11 + E * 8, "written": E * N * (4 * L + 8 + 1 + 1 + 2) + E}}


NOTES = ("FETCH_SIZE / WRITE_SIZE of rocprofv3 (KiB, converted to bytes), one counter-only pass each, mean of the last 20 "
         "dispatches. Reads below the algorithmic bytes: the state a kernel reads was written by the launch before it and "
         "is still in the memory-side cache. Writes: the ratio is what partial-line stores cost; the small outputs of "
         "finish are staged in LDS and leave as contiguous runs (for C2, 64 bytes of flags and 512 bytes of rewards per wave).")


def workload() -> None:
    import numpy as np
    import torch

    from collectivecrossing_amd import configs as C
    from collectivecrossing_amd.batched import BatchedCollectiveCrossing
    from collectivecrossing_amd.reset import build_reset_pool
    config = C.CollectiveCrossingConfig(
        width=12, height=8, division_y=4, tram_door_left=5, tram_door_right=7, tram_length=9, num_boarding_agents=5,
        num_exiting_agents=3, exiting_destination_area_y=0, boarding_destination_area_y=8,
        truncated_config=C.MaxStepsTruncatedConfig(max_steps=100))
    batch = BatchedCollectiveCrossing(config, E)
    batch.set_reset_pool(build_reset_pool(config, 0, 256))
    batch.reset_from_pool()
    actions = torch.from_numpy(np.random.default_rng(0).integers(0, 5, size=(STEPS, E, N), dtype=np.uint8)).cuda()
    for s in range(STEPS):
        batch.step_begin(actions[s])
        batch.step_finish(auto_reset=True)
    batch.synchronize()
    batch.close()


def summarise(directory: str, out: str) -> None:
    values: dict = {}
    for path in glob.glob(f"{directory}/**/*counter_collection.csv", recursive=True):
        with open(path, newline="") as f:
            for row in csv.DictReader(f):
                for kernel in ALGORITHMIC:
                    if kernel in row["Kernel_Name"]:
                        values.setdefault((kernel, row["Counter_Name"]), []).append((int(row["Dispatch_Id"]), float(row["Counter_Value"])))
    lines = []
    for kernel, alg in ALGORITHMIC.items():
        rec = {"kernel": kernel, "envs": E, "agents": N, "algorithmic_bytes": alg}
        for counter, key in (("FETCH_SIZE", "read"), ("WRITE_SIZE", "written")):
            v = [x for _, x in sorted(values.get((kernel, counter), []))][-20:]
            if v:
                measured = 1024.0 * sum(v) / len(v)                 # (the derived metrics are in KiB)
                rec[counter] = {"dispatches": len(v), "bytes_per_launch": round(measured),
                                "ratio_to_algorithmic": round(measured / alg[key], 3)}
            else:
                rec[counter] = None
        lines.append(rec)
    lines.append({"notes": NOTES})
    Path(out).write_text("".join(json.dumps(r) + "\n" for r in lines))
    print(Path(out).read_text(), end="")


if __name__ == "__main__":
    if len(sys.argv) == 4 and sys.argv[1] == "--summarise":
        summarise(sys.argv[2], sys.argv[3])
    else:
        workload()
