"""What the two shape-plan tests share: the recorded table (tests/golden/shape_plan/parent_plans.npz), the sweep and the
ctypes bindings of its generator (tests/golden/gen_shape_plan_golden.py)."""

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
