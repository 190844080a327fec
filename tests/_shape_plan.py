"""What the planner tests share: the recorded table (tests/golden/shape_plan/parent_plans.npz), the sweep and the
ctypes bindings of its generator (tests/golden/gen_shape_plan_golden.py), and the bindings of the per-call planner's
internal entry points (csrc/ccx_plan.h: ccxi_plan_call, ccxi_handle_call_plan)."""

import ctypes as C
import importlib.util
from pathlib import Path

_GEN = Path(__file__).resolve().parent / "golden" / "gen_shape_plan_golden.py"
_spec = importlib.util.spec_from_file_location("gen_shape_plan_golden", _GEN)
gen = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(gen)


def effective_inputs(table, i):
    """The planner inputs behind row i: a setting the library refused leaves the handle with its defaults."""
    f = list(table["in_fields"])
    values = table["inputs"][:, i].copy()
    if table["refused"][i] == 1:
        for name, v in gen.IN_DEFAULTS.items():
            values[f.index(name)] = v
    return values


def setting_of(table, i):
    """(name, value) of the one setting row i departs from the defaults with, or None."""
    f = list(table["in_fields"])
    for name, v in gen.IN_DEFAULTS.items():
        if table["inputs"][f.index(name), i] != v:
            return name, int(table["inputs"][f.index(name), i])
    return None


# ---- the per-call planner ------------------------------------------------------------------------------------------------
# ccxi_call_in (csrc/ccx_plan.h), in order: the call, then the handle's tunables with their defaults
CALL_FIELDS = ["K", "actions", "order", "actions_out", "policy", "mixed", "writes_obs", "capturing", "masks_bound", "reset_obs_on",
               "hand2", "round_launches", "small_shape", "step_kernel", "max_launch_steps", "reset_obs_fused"]
TUNABLE_DEFAULTS = dict(hand2=1, round_launches=1, small_shape=1, step_kernel=-1, max_launch_steps=0, reset_obs_fused=1)
# (actions, order, policy, actions_out, mixed): tensor, tensor + order, in-kernel policy, policy + actions_out, mixed,
# mixed + order, mixed with every slot scripted and actions_out
DRIVES = [(1, 0, 0, 0, 0), (1, 1, 0, 0, 0), (0, 0, 1, 0, 0), (0, 0, 1, 1, 0), (1, 0, 0, 0, 1), (1, 1, 0, 0, 1), (0, 0, 0, 1, 1)]


class CallIn(C.Structure):
    _fields_ = [(n, C.c_int32) for n in CALL_FIELDS]


def call(K, drive=DRIVES[0], rows=1, capturing=0, masks=0, reset=0, **tunables):
    """One stepping call as a dict of CALL_FIELDS."""
    actions, order, policy, actions_out, mixed = drive
    return dict(TUNABLE_DEFAULTS, K=K, actions=actions, order=order, policy=policy, actions_out=actions_out, mixed=mixed,
                writes_obs=rows, capturing=capturing, masks_bound=masks, reset_obs_on=reset, **tunables)


def bind_call(lib):
    """The two entry points of the per-call planner; returns the field names of ccxi_call_out."""
    lib.ccxi_call_field_names.restype = C.c_char_p
    lib.ccxi_plan_call.restype = C.c_int
    lib.ccxi_plan_call.argtypes = [C.POINTER(gen.PlanIn), C.POINTER(C.c_int), C.POINTER(CallIn), C.c_int, C.POINTER(C.c_int64)]
    lib.ccxi_handle_call_plan.restype = C.c_int
    lib.ccxi_handle_call_plan.argtypes = [C.c_void_p, C.POINTER(CallIn), C.c_int, C.POINTER(C.c_int64)]
    return [n for n in lib.ccxi_call_field_names().decode().split(",") if n]


def plan_call(lib, nfields, in_values, blocks_per_cu, c, launch=0):
    """ccxi_plan_call of the planner inputs `in_values` (gen.IN_FIELDS order), the two occupancy figures and the call c."""
    pin = gen.PlanIn(*[float(v) if f == "pace_start_ns" else int(v) for f, v in zip(gen.IN_FIELDS, in_values)])
    out = (C.c_int64 * nfields)()
    rc = lib.ccxi_plan_call(C.byref(pin), (C.c_int * 2)(*blocks_per_cu), C.byref(CallIn(*[int(c[n]) for n in CALL_FIELDS])), launch, out)
    assert rc == 0, (c, launch)
    return list(out)
