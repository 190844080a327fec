"""The per-row rule of csrc/ccx_mlp.h -- the very source the kernels of ccx_mlp.hip inline -- compiled for the host
(-O2 -ffp-contract=off) and run against the NumPy spec bit for bit: y and hidden for the four shapes the GPU tests use and
for every shape of the catalogue (tests/_mlp_shape_classes.py), which is what lets tests/test_gpu_mlp_shapes.py take the
host rule as a reference, and the two activations on their edge values.  No GPU."""

import ctypes as C

import numpy as np
import pytest
from _mlp_host_rule import CSRC, host_forward, load_forward  # noqa: F401  (CSRC, _compiler and _p are imported by other tests)
from _mlp_host_rule import compiler as _compiler
from _mlp_host_rule import ptr as _p
from _mlp_shape_classes import BACKWARD, EVERY_G, NUMPY_SPEC_BELOW
from _mlp_spec import SHAPES, bits32, bits32c, make_mlp_case, mlp_spec, relu_spec, tanh_spec


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    cxx = _compiler()
    if cxx is None:
        pytest.skip("no host C++ compiler (c++, clang++ or ROCm's clang++)")
    return load_forward(cxx, tmp_path_factory.mktemp("mlp_host_rule"))


@pytest.mark.parametrize("L, H, O, act", SHAPES)
def test_rows_equal_the_spec(host, L, H, O, act):
    M = 66 if L > 200 else 150
    c = make_mlp_case(M, L, H, O, seed=L + H)
    want_y, want_h = mlp_spec(c["x"], c["w1t"], c["b1"], c["w2"], c["b2"], act)
    for with_hidden in (True, False):
        y = np.full((M, O), np.nan, np.float32)
        hid = np.full((M, H), np.nan, np.float32) if with_hidden else None
        rc = host.host_mlp(C.c_longlong(M), L, H, O, act, _p(c["x"]), _p(c["w1t"]), _p(c["b1"]), _p(c["w2"]), _p(c["b2"]), _p(y), _p(hid))
        assert rc == 0
        np.testing.assert_array_equal(bits32c(y), bits32c(want_y))
        if with_hidden:
            np.testing.assert_array_equal(bits32c(hid), bits32c(want_h))
    assert np.isnan(want_y).any() and np.isfinite(want_y).any()


# every catalogue shape at M = 258 below 20 000 output elements of the backward and at M = 9 above (the row counts of
# tests/test_mlp_backward_host_rule.py), and the largest shape at M = 258 too; rows with NaN and infinities included
CATALOGUE = tuple((*s.dims, 258 if s.elements < NUMPY_SPEC_BELOW else 9) for s in BACKWARD) + tuple((*d, 258) for d in EVERY_G) + ((512, 256, 8, 0, 258),)


@pytest.mark.parametrize("L, H, O, act, M", CATALOGUE)
def test_catalogue_rows_equal_the_spec(host, L, H, O, act, M):
    c = make_mlp_case(M, L, H, O, seed=L + H + M)
    want_y, want_h = mlp_spec(c["x"], c["w1t"], c["b1"], c["w2"], c["b2"], act)
    y, hid = host_forward(host, c["x"], c["w1t"], c["b1"], c["w2"], c["b2"], act)
    bare, none = host_forward(host, c["x"], c["w1t"], c["b1"], c["w2"], c["b2"], act, with_hidden=False)
    np.testing.assert_array_equal(bits32c(y), bits32c(want_y))
    np.testing.assert_array_equal(bits32c(hid), bits32c(want_h))
    np.testing.assert_array_equal(bits32c(bare), bits32c(want_y))
    assert none is None and np.isnan(want_y).any() and np.isfinite(want_y).any() and np.isfinite(want_h).any()


def test_limits(host):
    z = np.zeros(8, np.float32)
    for L, H, O, act in ((0, 16, 1, 0), (513, 16, 1, 0), (4, 24, 1, 0), (4, 8, 1, 0), (4, 272, 1, 0), (4, 16, 0, 0), (4, 16, 9, 0),
                         (4, 16, 1, 2)):
        assert host.host_mlp(C.c_longlong(0), L, H, O, act, _p(z), _p(z), _p(z), _p(z), _p(z), _p(z), None) == -1, (L, H, O, act)


def test_activations_equal_the_spec(host):
    rng = np.random.default_rng(2)
    a = np.concatenate([np.array([0.0, -0.0, np.inf, -np.inf, np.nan, 40.0, -40.0, 39.999996, 40.000004, 1e30, -1e-45, 1e-45, 3e-39],
                                 np.float32), rng.uniform(-45, 45, 20000).astype(np.float32),
                        (rng.standard_normal(20000) * 1e-3).astype(np.float32)])
    t, r = np.full(a.size, 7.0, np.float32), np.full(a.size, 7.0, np.float32)
    host.host_activations(C.c_longlong(a.size), _p(a), _p(t), _p(r))
    np.testing.assert_array_equal(bits32(t), bits32(tanh_spec(a)))
    np.testing.assert_array_equal(bits32(r), bits32(relu_spec(a)))
