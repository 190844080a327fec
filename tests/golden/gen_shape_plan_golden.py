"""Records tests/golden/shape_plan/parent_plans.npz: the launch-shape decisions of a commit over a sweep of inputs.

    python tests/golden/gen_shape_plan_golden.py --commit <hash of the commit whose library is loaded>     (needs the MI355X)
    python tests/golden/gen_shape_plan_golden.py --coverage <libccx built with -DCCX_PLAN_COVERAGE>        (CPU)

The table is the equivalence gate of the launch-shape planner (csrc/ccx_plan.hip): tests/test_shape_plan.py
replays every row through ``ccxi_plan`` on the CPU, tests/test_gpu_shape_plan.py compares live handles with it.  It is
regenerated ONLY by a change that means to alter decisions, on that change's PARENT commit (plus nothing but the read-only
accessor ``ccxi_handle_plan`` where the parent lacks it), so that the change can show the rows it moved.

One row per (inputs, rows flag): the planner's inputs, what the library answered to the setting (``refused``), the
occupancy figure the runtime gave (``blocks_per_cu``) and every field of ``ccxi_plan_out``.  The sweep points are the
places where a rule of the selection switches.  ``--coverage`` replays the table through a build whose planner counts its
rule branches and fails if a branch is never taken.
"""

from __future__ import annotations

import argparse
import ctypes as C
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[2]
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))
TABLE = ROOT / "tests" / "golden" / "shape_plan" / "parent_plans.npz"

GRIDS = [(12, 8), (6, 16), (24, 16), (40, 30), (64, 48), (80, 60), (100, 100), (20, 12), (32, 16)]   # .. c3, c5_50 / c5_64
AGENTS = [1, 2, 3, 4, 5, 8, 12, 16, 20, 32, 50, 64]
ENVS = [1 << b for b in range(6, 17)] + [1000, 2160, 2304, 2430, 2816, 3000, 3072, 5000, 8193, 10000, 10920, 12000, 15800,
                                         16401, 17768, 17776, 17777, 20000, 20500, 36032, 100003]
SUB_GRIDS, SUB_AGENTS, SUB_ENVS = [(12, 8), (64, 48), (100, 100)], [1, 3, 8, 20, 32, 64], [1024, 4096, 10000, 32768]
# (name, values); "G" = the env's lane group
SETTINGS = [("lanes_per_wave", ["G", 64]), ("waves_per_block", [1, 2, 4]), ("writers", [1, 2, 3, 4, 7]),
            ("store_throttle", [-1, 16]), ("step_pace_ns", [-1, 400]), ("pace_start_ns", [700]), ("occ_tables", [0, 1]),
            ("pair_rows", [0, 1]), ("writer_roles", [0, 1]), ("pace_phase", [0]), ("tile_map", [3]), ("step_lanes", [32]),
            ("step_rows", [2]), ("reward_table", [1]), ("term_table", [1])]
TUNABLES = ("occ_tables", "pair_rows", "writer_roles", "pace_phase", "tile_map", "step_lanes", "step_rows")

# ccxi_plan_in (csrc/ccx_plan.h), in order; pace_start_ns is the one float
IN_FIELDS = ["E", "N", "width", "height", "num_cus", "reward_table", "term_table", "lanes_per_wave", "waves_per_block", "writers",
             "store_throttle", "step_pace_ns", "occ_tables", "pair_rows", "writer_roles", "pace_phase", "tile_map", "step_lanes",
             "step_rows", "rows", "pace_start_ns"]
IN_DEFAULTS = dict(reward_table=0, term_table=0, lanes_per_wave=0, waves_per_block=0, writers=0, store_throttle=0, step_pace_ns=0,
                   occ_tables=-1, pair_rows=-1, writer_roles=-1, pace_phase=-1, tile_map=-1, step_lanes=0, step_rows=0,
                   pace_start_ns=0)


class PlanIn(C.Structure):
    _fields_ = [(n, C.c_float if n == "pace_start_ns" else C.c_int32) for n in IN_FIELDS]


def bind(lib):
    """The two internal entry points and the field names of ccxi_plan_out."""
    lib.ccxi_plan_field_names.restype = C.c_char_p
    names = [n for n in lib.ccxi_plan_field_names().decode().split(",") if n]
    lib.ccxi_handle_plan.restype = C.c_int
    lib.ccxi_handle_plan.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_int64), C.POINTER(C.c_int)]
    if hasattr(lib, "ccxi_plan"):
        lib.ccxi_plan.restype = C.c_int
        lib.ccxi_plan.argtypes = [C.POINTER(PlanIn), C.c_int, C.POINTER(C.c_int64)]
    return names


def sweep():
    """(width, height, agents, envs, setting name or None, value): defaults on the full grid, each setting alone on the
    sub-grid."""
    for w, h in GRIDS:
        for n in AGENTS:
            for e in ENVS:
                yield w, h, n, e, None, 0
    for w, h in SUB_GRIDS:
        for n in SUB_AGENTS:
            for e in SUB_ENVS:
                for name, values in SETTINGS:
                    for v in values:
                        yield w, h, n, e, name, (1 << max(0, (n - 1).bit_length())) if v == "G" else v


def plan_inputs(w, h, n, e, name, value, num_cus, rows):
    d = dict(IN_DEFAULTS, E=e, N=n, width=w, height=h, num_cus=num_cus, rows=rows)
    if name:
        d[name] = value
    return d


def params_for(w, h, n):
    """Any valid env of this grid and agent count: the selection reads the grid and the agent count only."""
    from collectivecrossing_amd._abi import CcxParams
    p = CcxParams()
    p.width, p.height, p.division_y = w, h, max(1, h // 2)
    p.tram_left, p.tram_right = 0, w
    p.door_left, p.door_right = max(0, w // 2 - 1), w // 2 + 1
    p.num_boarding, p.num_exiting = (n + 1) // 2, n // 2
    p.boarding_dest_y, p.exiting_dest_y = h, 0
    p.reward_mode = p.terminated_mode = p.truncated_mode = 0
    p.max_steps = 100
    p.boarding_destination_reward, p.tram_door_reward, p.tram_area_reward = 15.0, 10.0, 5.0
    p.distance_penalty_factor, p.goal_reward, p.no_goal_reward, p.step_penalty = 0.1, 1.0, 0.0, -1.0
    return p


def create(lib, w, h, n, e):
    """A handle on device 0, or None where the library refuses it."""
    handle = C.c_void_p()
    p = params_for(w, h, n)
    rc = lib.ccx_create(C.byref(p), e, 0, e, 0, None, C.byref(handle))
    return handle if rc == 0 else None


def apply_setting(lib, handle, w, h, name, value):
    """The library call behind one setting; returns its status."""
    if name == "lanes_per_wave":
        return lib.ccx_set_launch_shape(handle, value, 0)
    if name == "waves_per_block":
        return lib.ccx_set_launch_shape(handle, 0, value)
    if name == "writers":
        return lib.ccx_set_writers(handle, value)
    if name == "store_throttle":
        return lib.ccx_set_store_throttle(handle, value)
    if name == "step_pace_ns":
        return lib.ccx_set_step_pace(handle, value)
    if name == "pace_start_ns":
        return lib.ccx_set_step_pace_start(handle, float(value))
    if name in TUNABLES:
        return lib.ccx_set_tunable(handle, name.encode(), value)
    if name == "reward_table":
        tab = np.zeros((h + 1, w + 1), np.float64)
        return lib.ccx_set_reward_table(handle, tab.ctypes.data, tab.ctypes.data)
    if name == "term_table":
        tab = np.zeros((h + 1, w + 1), np.uint8)
        return lib.ccx_set_terminated_table(handle, tab.ctypes.data, tab.ctypes.data)
    raise ValueError(name)


def handle_rows(lib, nfields, point, num_cus, probe=None):
    """The two rows (rows = 1, 0) of one sweep point from a live handle: (inputs dict, refused, blocks_per_cu, outputs).
    ``probe(handle)`` is called on the live handle, after the setting."""
    w, h, n, e, name, value = point
    handle = create(lib, w, h, n, e)
    if handle is None:
        return [(plan_inputs(w, h, n, e, name, value, num_cus, rows), 2, 0, [0] * nfields) for rows in (1, 0)]   # (2: no handle)
    try:
        refused = 0
        if name and apply_setting(lib, handle, w, h, name, value) != 0:
            refused = 1           # (the handle keeps launching with what it had: the rows record that)
        out = []
        for rows in (1, 0):
            buf = (C.c_int64 * nfields)()
            per_cu = C.c_int(0)
            rc = lib.ccxi_handle_plan(handle, rows, buf, C.byref(per_cu))
            assert rc == 0, lib.ccx_last_error()
            out.append((plan_inputs(w, h, n, e, name, value, num_cus, rows), refused, per_cu.value, list(buf)))
        if probe:
            probe(handle)
        return out
    finally:
        lib.ccx_destroy(handle)


def load_table(path=TABLE):
    z = np.load(path)
    return {k: z[k] for k in z.files}


def record(commit: str) -> None:
    import torch

    from collectivecrossing_amd import _lib
    lib = _lib.load()
    names = bind(lib)
    num_cus = torch.cuda.get_device_properties(0).multi_processor_count
    ins, refused, per_cu, outs = [], [], [], []
    points = list(sweep())
    for i, point in enumerate(points):
        for d, r, b, o in handle_rows(lib, len(names), point, num_cus):
            ins.append([d[f] for f in IN_FIELDS])
            refused.append(r)
            per_cu.append(b)
            outs.append(o)
        if i % 500 == 0:
            print(f"{i} / {len(points)} handles", flush=True)
    TABLE.parent.mkdir(parents=True, exist_ok=True)
    # (field-major: a column of near-constant values compresses far better than a row of unlike ones)
    np.savez_compressed(TABLE, commit=np.array(commit), in_fields=np.array(IN_FIELDS), out_fields=np.array(names),
                        inputs=np.array(ins, np.int64).T.copy(), refused=np.array(refused, np.int8),
                        blocks_per_cu=np.array(per_cu, np.int32), outputs=np.array(outs, np.int64).T.copy())
    print(f"{len(ins)} rows, {sum(refused)} refused, {TABLE.stat().st_size} bytes, commit {commit}")


def plan_row(lib, nfields, in_values, blocks_per_cu):
    """ccxi_plan of one row of the table."""
    pin = PlanIn(*[float(v) if f == "pace_start_ns" else int(v) for f, v in zip(IN_FIELDS, in_values)])
    buf = (C.c_int64 * nfields)()
    rc = lib.ccxi_plan(C.byref(pin), int(blocks_per_cu), buf)
    assert rc == 0
    return list(buf)


def coverage(lib_path: str) -> None:
    lib = C.CDLL(lib_path)
    names = bind(lib)
    lib.ccxi_plan_coverage.restype = C.c_char_p
    t = load_table()
    assert list(t["out_fields"]) == names
    for i in range(t["inputs"].shape[1]):
        plan_row(lib, len(names), t["inputs"][:, i], t["blocks_per_cu"][i])
    counts = dict(item.split("=") for item in lib.ccxi_plan_coverage().decode().split(",") if item)
    for branch, hits in counts.items():
        print(f"{branch:32s} {hits}")
    never = [b for b, hits in counts.items() if int(hits) == 0]
    assert not never, f"rule branches no row of the table takes: {never}"


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--commit", help="hash of the commit the loaded library was built from (recorded in the table)")
    ap.add_argument("--coverage", metavar="LIB", help="replay the table through a -DCCX_PLAN_COVERAGE build and list the branch counts")
    args = ap.parse_args()
    if args.coverage:
        coverage(args.coverage)
    elif args.commit:
        record(args.commit)
    else:
        ap.error("--commit or --coverage")
