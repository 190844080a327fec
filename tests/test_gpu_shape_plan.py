"""Live handles launch with the recorded plans, and with what the pure planner says (csrc/ccx_plan.hip).

On every 7th row of tests/golden/shape_plan/parent_plans.npz plus all of its settings rows: ``ccxi_handle_plan`` of a live
handle equals the table, the occupancy figure the runtime answers is the recorded one, and ``ccxi_plan`` fed with the
handle's own figure returns the same plan.  This pins what tests/test_shape_plan.py cannot see without a GPU: how
choose_shape applies a plan to the handle, and the occupancy query.

The same handles answer for the per-call planner, without a launch: ``ccxi_handle_call_plan`` of a handful of calls equals
``ccxi_plan_call`` fed with the handle's plan inputs and occupancy figures, and ``ccx_get_masks_fused`` /
``ccx_get_reset_obs_fused`` say what that plan says."""

import ctypes as C

import pytest

from _shape_plan import DRIVES, CALL_FIELDS, CallIn, bind_call, call, effective_inputs, gen, plan_call, setting_of

pytestmark = pytest.mark.gpu

# K = 1 / 16 / 17 / 64 from a tensor with rows, with masks bound and restarted rows to write; without rows; with a move
# order; mixed control
CALLS = ([call(K, masks=1, reset=1) for K in (1, 16, 17, 64)] + [call(K, rows=0, masks=1, reset=1) for K in (1, 64)]
         + [call(1, DRIVES[1], masks=1, reset=1)] + [call(K, DRIVES[4], masks=1, reset=1) for K in (1, 17)])


def call_plans_of(lib, nfields, handle):
    """What the live handle says about CALLS: ccxi_handle_call_plan of the first launch, and the two fused queries."""
    plans, queries = [], []
    for c in CALLS:
        out = (C.c_int64 * nfields)()
        rc = lib.ccxi_handle_call_plan(handle, C.byref(CallIn(*[int(c[n]) for n in CALL_FIELDS])), 0, out)
        assert rc == 0, lib.ccx_last_error()
        plans.append(list(out))
        fused = [C.c_int32(-1), C.c_int32(-1)]
        for fn, slot in zip((lib.ccx_get_masks_fused, lib.ccx_get_reset_obs_fused), fused):
            assert fn(handle, c["K"], c["order"], c["mixed"], C.byref(slot)) == 0, lib.ccx_last_error()
        queries.append([f.value for f in fused])
    return plans, queries


def test_live_handles_match_the_table_and_the_planner():
    import torch

    from collectivecrossing_amd import _lib

    lib = _lib.load()
    names = gen.bind(lib)
    call_names = bind_call(lib)
    table = gen.load_table()
    assert list(table["out_fields"]) == names
    f = gen.IN_FIELDS
    num_cus = torch.cuda.get_device_properties(0).multi_processor_count
    assert num_cus == int(table["inputs"][f.index("num_cus"), 0]), "the table was recorded on a device of another size"
    rows = table["inputs"].shape[1]
    picked = sorted({i - (i % 2) for i in range(0, rows, 7)} | {i for i in range(0, rows, 2) if setting_of(table, i)})
    wrong, wrong_calls = [], []
    for i in picked:                          # (rows i, i + 1: the two shapes of one handle)
        get = lambda name: int(table["inputs"][f.index(name), i])
        point = (get("width"), get("height"), get("N"), get("E"), *(setting_of(table, i) or (None, 0)))
        said = []
        live = gen.handle_rows(lib, len(names), point, num_cus,
                               probe=lambda handle: said.extend(call_plans_of(lib, len(call_names), handle)))
        for j, (inputs, refused, per_cu, out) in zip((i, i + 1), live):
            want = [int(v) for v in table["outputs"][:, j]]
            planned = want if refused == 2 else gen.plan_row(lib, len(names), effective_inputs(table, j), per_cu)
            if not (out == want == planned and refused == table["refused"][j] and per_cu == table["blocks_per_cu"][j]
                    and [inputs[n] for n in f] == table["inputs"][:, j].tolist()):
                wrong.append((inputs, refused, per_cu, [(n, a, b, c) for n, a, b, c in zip(names, out, want, planned)
                                                        if not a == b == c]))
        if said:                              # (a handle was created)
            plans, queries = said
            per_cu = [live[0][2], live[1][2]]
            for c, plan, query in zip(CALLS, plans, queries):
                want = plan_call(lib, len(call_names), effective_inputs(table, i), per_cu, c)
                fused = [want[call_names.index("masks_fused")], want[call_names.index("reset_obs_fused")]]
                if plan != want or query != fused:
                    wrong_calls.append((live[0][0], c, dict(zip(call_names, plan)), dict(zip(call_names, want)), query))
    assert not wrong, f"{len(wrong)} of {2 * len(picked)} rows differ, the first: {wrong[:3]}"
    assert not wrong_calls, f"{len(wrong_calls)} call plans differ, the first: {wrong_calls[:3]}"
