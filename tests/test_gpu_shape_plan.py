"""Live handles launch with the recorded plans, and with what the pure planner says (csrc/ccx_plan.hip).

On every 7th row of tests/golden/shape_plan/parent_plans.npz plus all of its settings rows: ``ccxi_handle_plan`` of a live
handle equals the table, the occupancy figure the runtime answers is the recorded one, and ``ccxi_plan`` fed with the
handle's own figure returns the same plan.  This pins what tests/test_shape_plan.py cannot see without a GPU: how
choose_shape applies a plan to the handle, and the occupancy query."""

import ctypes as C

import pytest

from _shape_plan import effective_inputs, gen, setting_of

pytestmark = pytest.mark.gpu


def test_live_handles_match_the_table_and_the_planner():
    import torch

    from collectivecrossing_amd import _lib

    lib = _lib.load()
    names = gen.bind(lib)
    table = gen.load_table()
    assert list(table["out_fields"]) == names
    f = gen.IN_FIELDS
    num_cus = torch.cuda.get_device_properties(0).multi_processor_count
    assert num_cus == int(table["inputs"][f.index("num_cus"), 0]), "the table was recorded on a device of another size"
    rows = table["inputs"].shape[1]
    picked = sorted({i - (i % 2) for i in range(0, rows, 7)} | {i for i in range(0, rows, 2) if setting_of(table, i)})
    wrong = []
    for i in picked:                          # (rows i, i + 1: the two shapes of one handle)
        get = lambda name: int(table["inputs"][f.index(name), i])
        point = (get("width"), get("height"), get("N"), get("E"), *(setting_of(table, i) or (None, 0)))
        live = gen.handle_rows(lib, len(names), point, num_cus)
        for j, (inputs, refused, per_cu, out) in zip((i, i + 1), live):
            want = [int(v) for v in table["outputs"][:, j]]
            planned = want if refused == 2 else gen.plan_row(lib, len(names), effective_inputs(table, j), per_cu)
            if not (out == want == planned and refused == table["refused"][j] and per_cu == table["blocks_per_cu"][j]
                    and [inputs[n] for n in f] == table["inputs"][:, j].tolist()):
                wrong.append((inputs, refused, per_cu, [(n, a, b, c) for n, a, b, c in zip(names, out, want, planned)
                                                        if not a == b == c]))
    assert not wrong, f"{len(wrong)} of {2 * len(picked)} rows differ, the first: {wrong[:3]}"
