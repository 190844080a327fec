"""The shape catalogue of tests/_mlp_wide_shape_classes.py against the library's own launch-shape functions
(csrc/ccx_mlp_wide.h: chunk_outputs, lds_floats, slab_outputs, first_rows, second_rows, grid_y -- the very functions
csrc/ccx_mlp_wide.hip launches by, compiled for the host, tests/_mlp_wide_host_rule.py): every figure of the catalogue, and
that its shapes cover every branch the shape selects.  No Python copy of the functions; no GPU."""

import ctypes as C

import pytest
from _mlp_wide_host_rule import compiler, launch_shape, load
from _mlp_wide_shape_classes import CATALOGUE, LDS_BUDGET, NARROW, by_dims


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    cxx = compiler()
    if cxx is None:
        pytest.skip("no host C++ compiler (c++, clang++ or ROCm's clang++)")
    return load(cxx, tmp_path_factory.mktemp("mlp_wide_shape_classes"))


@pytest.mark.parametrize("s", CATALOGUE, ids=lambda s: f"{s.L}-{s.H}-{s.O}")
def test_the_catalogue_states_what_the_library_computes(lib, s):
    g = launch_shape(lib, s.L, s.H, s.O)
    assert (g.chunk, g.chunks, g.forward_bytes) == (s.chunk, s.chunks, s.forward_bytes), s.why
    assert (g.slab, g.slabs, g.rows1, g.rows2, g.slices1, g.grid_y) == (s.slab, s.slabs, s.rows1, s.rows2, s.slices1, s.grid_y), s.why
    assert max(g.bytes1, g.bytes2) <= LDS_BUDGET                          # no backward launch asks for more
    assert g.forward_bytes <= 160 * 1024                                  # what a workgroup of gfx950 may have


def test_the_chunks_cover_their_classes(lib):
    assert {s.chunks for s in CATALOGUE} >= {1, 2, 3, 4, 8, 10}              # one chunk, a few, the customary head, the most
    assert {s.last_chunk_partial for s in CATALOGUE} == {False, True}
    assert any(s.chunks > 1 and not s.last_chunk_partial for s in CATALOGUE)   # several whole chunks
    assert any(s.O % s.chunk == 1 for s in CATALOGUE) and any(s.O % 4 for s in CATALOGUE if s.chunks > 1)
    assert max(launch_shape(lib, 7, H, 320).chunks for H in range(16, 257, 16)) == 10 == by_dims(512, 256, 320).chunks
    # the boundary of one chunk at G = 1, and of the chunk size at G = 3 -> 4
    assert launch_shape(lib, 7, 16, 224).chunks == 1 and launch_shape(lib, 7, 16, 225).chunks == 2
    assert launch_shape(lib, 7, 48, 320).chunk == 64 and launch_shape(lib, 7, 64, 320).chunk == 32
    assert all(launch_shape(lib, 7, H, 320).chunk % 32 == 0 for H in range(16, 257, 16))


def test_the_forward_straddles_the_opt_in_on_both_sides(lib):
    # the partials: G = 7 is the last without, G = 8 the first with
    assert by_dims(7, 112, 255).forward_bytes == 58240 <= LDS_BUDGET < 66560 == by_dims(7, 128, 32).forward_bytes
    # the x tile
    assert by_dims(255, 16, 9).forward_bytes == 65280 <= LDS_BUDGET < 65792 == by_dims(256, 16, 9).forward_bytes
    assert max(launch_shape(lib, L, H, 320).forward_bytes for L in (1, 512) for H in range(16, 257, 16)) == 133120
    assert {s.opt_in for s in CATALOGUE} == {False, True} and {s.act for s in CATALOGUE} == {0, 1}
    assert {s.H // 16 for s in CATALOGUE} >= {1, 3, 4, 7, 8, 16}


def test_the_backward_covers_its_classes(lib):
    assert {s.rows1 for s in CATALOGUE} == {64, 32, 16, 8}
    assert {s.rows2 for s in CATALOGUE} == {64, 32}                       # all the second part takes: 32 from H = 192 on
    assert {launch_shape(lib, 7, H, 320).rows2 for H in range(16, 257, 16)} == {64, 32}
    assert {s.slabs for s in CATALOGUE} >= {1, 2, 4, 8, 16, 20}
    assert any(s.slabs > 1 and s.O % s.slab == 1 for s in CATALOGUE)     # a last slab of one output
    assert any(s.slab % 4 for s in CATALOGUE if s.slabs > 1)             # a slab that is no whole number of quads
    assert by_dims(38, 64, 64).slabs == 1 and by_dims(38, 64, 65).slabs == 2   # the boundary
    assert {s.slices1 for s in CATALOGUE} >= {1, 2, 33}
    assert max(s.grid_y for s in CATALOGUE) == launch_shape(lib, 512, 256, 320).grid_y == 54   # the largest the ABI admits
    for s in CATALOGUE:
        assert s.grid_y > s.slices1 >= 1                                  # both parts have slices


def test_the_narrow_shapes_take_one_chunk_and_one_slab(lib):
    for L, H, O, _ in NARROW:
        g = launch_shape(lib, L, H, O)
        assert (g.chunk, g.chunks, g.slab, g.slabs) == (O, 1, O, 1)


def test_shapes_outside_the_limits_have_no_launch_shape(lib):
    out = (C.c_longlong * 11)()
    for L, H, O in ((0, 16, 1), (513, 16, 1), (4, 24, 1), (4, 272, 1), (4, 16, 0), (4, 16, 321)):
        assert lib.host_wide_shape(L, H, O, out) == -1, (L, H, O)
    assert lib.host_wide_shape(4, 16, 320, out) == 0 and lib.host_wide_shape(4, 16, 9, out) == 0
