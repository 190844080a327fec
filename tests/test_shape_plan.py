"""The launch-shape planner (csrc/ccx_plan.hip) reproduces the decisions recorded from the parent of the change that
introduced it, field for field, on a machine without a GPU.

tests/golden/shape_plan/parent_plans.npz holds one row per (inputs, rows flag) of a sweep over the points where a rule of
the selection switches (tests/golden/gen_shape_plan_golden.py): the inputs, the occupancy figure the runtime answered on
the MI355X and every field of the plan a live handle of that commit launched with.  ``ccxi_plan`` fed with the same inputs
and that occupancy figure must return exactly those integers.  The table is regenerated only by a change that means to
alter decisions, on that change's parent."""

import ctypes as C
from pathlib import Path

import numpy as np
import pytest

from _shape_plan import effective_inputs, gen


@pytest.fixture(scope="module")
def lib():
    from collectivecrossing_amd import _lib

    if not _lib.LIB_PATH.exists():
        pytest.skip("libccx.so not built (run __graft_entry__.build())")
    return C.CDLL(str(_lib.LIB_PATH))


@pytest.fixture(scope="module")
def table():
    return gen.load_table()


def test_internal_entry_points_stay_out_of_the_public_abi(lib):
    from collectivecrossing_amd import _abi

    assert hasattr(lib, "ccxi_plan") and hasattr(lib, "ccxi_handle_plan")
    assert hasattr(lib, "ccxi_plan_call") and hasattr(lib, "ccxi_handle_call_plan") and hasattr(lib, "ccxi_call_field_names")
    header = (Path(__file__).resolve().parents[1] / "include" / "ccx.h").read_text()
    assert "ccxi_" not in header
    assert not [n for n in _abi.PROTOTYPES if n.startswith("ccxi_")]


def test_table_covers_the_sweep(table):
    points = list(gen.sweep())
    assert table["inputs"].shape[1] == 2 * len(points) and list(table["in_fields"]) == gen.IN_FIELDS
    assert len(str(table["commit"])) == 40
    f = gen.IN_FIELDS
    cols = [f.index(n) for n in ("width", "height", "N", "E")]
    got = table["inputs"][cols][:, ::2].T
    assert np.array_equal(got, np.array([[w, h, n, e] for w, h, n, e, _, _ in points]))
    assert np.array_equal(table["inputs"][f.index("rows")], np.tile([1, 0], len(points)))


def test_planner_reproduces_every_recorded_plan(lib, table):
    names = gen.bind(lib)
    assert list(table["out_fields"]) == names
    wrong = []
    for i in range(table["inputs"].shape[1]):
        if table["refused"][i] == 2:          # (no handle: nothing was planned)
            continue
        got = gen.plan_row(lib, len(names), effective_inputs(table, i), table["blocks_per_cu"][i])
        want = [int(v) for v in table["outputs"][:, i]]
        if got != want:
            wrong.append((dict(zip(gen.IN_FIELDS, table["inputs"][:, i].tolist())),
                          [(n, g, w) for n, g, w in zip(names, got, want) if g != w]))
    assert not wrong, f"{len(wrong)} rows differ, the first: {wrong[:3]}"


def test_reward_table_refusals_follow_from_the_plan(lib, table):
    """ccx_set_reward_table refuses a table exactly where a shape planned WITH it exceeds 150 KB of LDS."""
    names = gen.bind(lib)
    f = gen.IN_FIELDS
    asked = np.flatnonzero(table["inputs"][f.index("reward_table")] == 1)
    assert len(asked) and table["refused"][asked].any() and not table["refused"][asked].all()
    assert not np.delete(table["refused"], asked).any()
    for i in asked[::2]:                      # (row i: rows = 1, row i + 1: rows = 0 of the same handle)
        too_big = False
        for j in (i, i + 1):
            lds = gen.plan_row(lib, len(names), table["inputs"][:, j], table["blocks_per_cu"][j])[names.index("lds_bytes")]
            too_big = too_big or lds > 150 * 1024
        assert too_big == bool(table["refused"][i]) == bool(table["refused"][i + 1])
