"""The backward rule of csrc/ccx_mlp_grad.h -- the very source the kernels of ccx_mlp_backward.hip inline -- compiled for the
host (-O2 -ffp-contract=off) and run against the NumPy spec bit for bit: the four gradients and ga for the four shapes the
GPU tests use and for every shape of the catalogue (tests/_mlp_shape_classes.py), which is what lets
tests/test_gpu_mlp_shapes.py take the host rule as a reference where the spec's Python loop over the output elements is too
slow, and the workspace size against its formula and at its limits.  No GPU."""

import ctypes as C

import numpy as np
import pytest
from _mlp_backward_spec import NAMES, bits32, bits32c, make_mlp_backward_case, mlp_backward_spec
from _mlp_host_rule import compiler as _compiler
from _mlp_host_rule import host_backward, load_backward
from _mlp_host_rule import ptr as _p
from _mlp_shape_classes import BACKWARD, NUMPY_SPEC_BELOW
from _mlp_spec import SHAPES


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    cxx = _compiler()
    if cxx is None:
        pytest.skip("no host C++ compiler (c++, clang++ or ROCm's clang++)")
    return load_backward(cxx, tmp_path_factory.mktemp("mlp_backward_host_rule"))


@pytest.mark.parametrize("L, H, O, act", SHAPES)
def test_gradients_equal_the_spec(host, L, H, O, act):
    M = 70 if L > 200 else 300                                           # 300: two blocks, the second of 44 rows
    c = make_mlp_backward_case(M, L, H, O, act, seed=L + H)
    want = mlp_backward_spec(c["x"], c["hidden"], c["grad_y"], c["w2"], act)
    got = dict(w1t=np.full((L, H), np.nan, np.float32), b1=np.full(H, np.nan, np.float32), w2=np.full((O, H), np.nan, np.float32),
               b2=np.full(O, np.nan, np.float32), ga=np.full((M, H), np.nan, np.float32))
    rc = host.host_mlp_backward(C.c_longlong(M), L, H, O, act, _p(c["x"]), _p(c["hidden"]), _p(c["grad_y"]), _p(c["w2"]),
                                _p(got["w1t"]), _p(got["b1"]), _p(got["w2"]), _p(got["b2"]), _p(got["ga"]))
    assert rc == 0
    for name in NAMES + ("ga",):
        np.testing.assert_array_equal(bits32c(got[name]), bits32c(want[name]), err_msg=name)
        assert np.isfinite(want[name]).all() and want[name].any(), name


# every catalogue shape: two blocks (M = 258: the second of two rows) where the spec's loop over the output elements takes
# about a second, M = 9 above; and the two-block case for one large shape, the one with a padded grad_y quad (O = 7)
CATALOGUE = tuple((*s.dims, 258 if s.elements < NUMPY_SPEC_BELOW else 9) for s in BACKWARD) + ((511, 240, 7, 0, 258),)


@pytest.mark.parametrize("L, H, O, act, M", CATALOGUE)
def test_catalogue_gradients_equal_the_spec(host, L, H, O, act, M):
    c = make_mlp_backward_case(M, L, H, O, act, seed=L + H + M)
    want = mlp_backward_spec(c["x"], c["hidden"], c["grad_y"], c["w2"], act)
    got = host_backward(host, c["x"], c["hidden"], c["grad_y"], c["w2"], act)
    for name in NAMES + ("ga",):
        np.testing.assert_array_equal(bits32(got[name]), bits32(want[name]), err_msg=name)   # finite inputs: every bit, no NaN
        assert np.isfinite(want[name]).all() and want[name].any(), name


def test_workspace_bytes(host):
    ws = host.host_mlp_backward_workspace_bytes

    def formula(rows, L, H, O):
        return -(-rows // 256) * (L * H + H + O * H + O) * 8

    for rows in (1, 255, 256, 257, 131072, 524288, 2**40):
        for L, H, O in ((38, 64, 5), (1, 16, 1), (512, 256, 8), (262, 256, 8)):
            assert ws(C.c_longlong(rows), L, H, O) == formula(rows, L, H, O), (rows, L, H, O)
    assert ws(C.c_longlong(524288), 38, 64, 5) == 46219264              # the 46 MB the header states
    for rows, L, H, O in ((0, 38, 64, 5), (-1, 38, 64, 5), (8, 0, 64, 5), (8, 513, 64, 5), (8, 38, 8, 5), (8, 38, 24, 5),
                          (8, 38, 272, 5), (8, 38, 64, 0), (8, 38, 64, 9)):
        assert ws(C.c_longlong(rows), L, H, O) == 0, (rows, L, H, O)


def test_refusals(host):
    z = np.zeros(8, np.float32)
    for rows, L, H, O, act in ((0, 4, 16, 1, 0), (4, 0, 16, 1, 0), (4, 4, 24, 1, 0), (4, 4, 16, 9, 0), (4, 4, 16, 1, 2)):
        assert host.host_mlp_backward(C.c_longlong(rows), L, H, O, act, *([_p(z)] * 9)) == -1, (rows, L, H, O, act)
