"""The shape catalogue of tests/_mlp_shape_classes.py against the library's own launch-shape functions -- ccx_mlp_grad::sub_rows
and grid_y (csrc/ccx_mlp_grad.h), ccx_mlp::lds_floats (csrc/ccx_mlp.h), the very functions csrc/ccx_mlp_backward.hip,
csrc/ccx_mlp.hip and csrc/ccx_sides.hip launch by, compiled for the host (tests/_mlp_host_rule.py): every figure of the
catalogue, and that its shapes cover every branch the shape selects.  No Python copy of the functions; no GPU."""

import pytest
from _mlp_host_rule import compiler, load_backward, load_forward, sub_rows
from _mlp_shape_classes import (BACKWARD, EVERY_G, EXACT_BUDGET, LDS_BUDGET, PICKED_PER_ROW, SIDES_BACKWARD, SIDES_FORWARD, by_dims)
from _mlp_spec import SHAPES


@pytest.fixture(scope="module")
def libs(tmp_path_factory):
    cxx = compiler()
    if cxx is None:
        pytest.skip("no host C++ compiler (c++, clang++ or ROCm's clang++)")
    d = tmp_path_factory.mktemp("mlp_shape_classes")
    return load_forward(cxx, d), load_backward(cxx, d)


def forward_bytes(fwd, L, H, O, draw=False):
    return fwd.host_lds_floats(L, H, O, int(draw)) * 4


@pytest.mark.parametrize("s", BACKWARD, ids=lambda s: f"{s.L}-{s.H}-{s.O}")
def test_the_catalogue_states_what_the_library_computes(libs, s):
    fwd, bwd = libs
    assert sub_rows(bwd, s.L, s.H, s.O) == (s.r_adjacent, s.bytes_adjacent), s.why
    assert sub_rows(bwd, s.L, s.H, s.O, PICKED_PER_ROW) == (s.r_picked, s.bytes_picked), s.why
    assert forward_bytes(fwd, s.L, s.H, s.O) == s.forward_bytes, s.why
    assert bwd.host_grad_grid_y(s.L, s.H, s.O) == s.grid_y, s.why
    assert max(s.bytes_adjacent, s.bytes_picked) <= LDS_BUDGET                # no backward launch asks for more


def test_no_catalogue_shape_has_left():
    assert [(s.L, s.H, s.O) for s in BACKWARD] == [(106, 64, 5), (110, 64, 5), (206, 64, 5), (255, 16, 1), (256, 16, 1), (257, 16, 1),
                                                   (368, 256, 8), (484, 256, 1), (372, 256, 8), (511, 240, 7), (512, 256, 8), (512, 16, 1)]
    assert [(L, H, O) for L, H, O, _ in EVERY_G] == [(7, H, 3) for H in range(16, 257, 16)]
    assert {s.act for s in BACKWARD} == {0, 1} == {act for *_, act in EVERY_G}     # both activations


def test_every_sub_tile_height_is_taken_in_both_kernels(libs):
    _, bwd = libs
    for per_row, kernel in ((0, "adjacent"), (PICKED_PER_ROW, "picked")):
        taken = {sub_rows(bwd, s.L, s.H, s.O, per_row)[0] for s in BACKWARD}
        assert taken == {64, 32, 16, 8}, kernel
    # the picked kernel is run on a subset of the shapes (64 and 16 rows are tests/test_gpu_sides_backward.py's)
    assert {sub_rows(bwd, *d, PICKED_PER_ROW)[0] for d in SIDES_BACKWARD} == {32, 8}
    # the boundary of the first drop, and the shapes the suite had: only 64 and 16
    assert sub_rows(bwd, 106, 64, 5)[0] == 64 and sub_rows(bwd, 110, 64, 5)[0] == 32
    assert {sub_rows(bwd, L, H, O)[0] for L, H, O, _ in SHAPES} == {64, 16}
    assert sub_rows(bwd, 262, 256, 8, PICKED_PER_ROW)[0] == 16


def test_both_exact_budget_shapes_ask_for_all_of_it(libs):
    _, bwd = libs
    for d in EXACT_BUDGET:
        assert sub_rows(bwd, *d) == (16, LDS_BUDGET), d
        R, b = sub_rows(bwd, *d, PICKED_PER_ROW)
        assert R == 8 and b < LDS_BUDGET, d
        assert by_dims(*d).bytes_adjacent == LDS_BUDGET
    assert EXACT_BUDGET[0] in SIDES_BACKWARD                                  # R = 8 against R = 16 on the same rows


def test_the_forward_tiles_straddle_the_opt_in(libs):
    fwd, _ = libs
    assert forward_bytes(fwd, 255, 16, 1) == 65280 <= LDS_BUDGET < 65792 == forward_bytes(fwd, 256, 16, 1) == forward_bytes(fwd, 257, 16, 1)
    assert {255, 256, 257} <= {s.L for s in BACKWARD}
    assert max(s.forward_bytes for s in BACKWARD) == forward_bytes(fwd, 512, 256, 8) == 131328   # the largest the ABI admits
    assert forward_bytes(fwd, 512, 256, 8, draw=True) == 131328                # the fused kernels' y fits behind the partials
    assert all(forward_bytes(fwd, *d) > LDS_BUDGET for d in SIDES_FORWARD)
    assert all(forward_bytes(fwd, L, H, O) < 16384 for L, H, O, _ in EVERY_G)


def test_every_wave_count_occurs():
    assert sorted(H // 16 for _, H, _, _ in EVERY_G) == list(range(1, 17))
    assert {s.H // 16 for s in BACKWARD} >= {1, 4, 15, 16}


def test_the_tile_grid_reaches_its_maximum(libs):
    _, bwd = libs
    assert max(s.grid_y for s in BACKWARD) == bwd.host_grad_grid_y(512, 256, 8) == 33
    assert any(s.O == 7 for s in BACKWARD)                                    # a padded grad_y quad, a partly live last tile row


def test_shapes_outside_the_limits_have_no_launch_shape(libs):
    fwd, bwd = libs
    for L, H, O in ((0, 16, 1), (513, 16, 1), (4, 24, 1), (4, 272, 1), (4, 16, 0), (4, 16, 9)):
        assert sub_rows(bwd, L, H, O)[0] == -1 and bwd.host_grad_grid_y(L, H, O) == 0 and fwd.host_lds_floats(L, H, O, 0) == -1, (L, H, O)
