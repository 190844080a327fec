"""The NumPy restatement of CCX_MLP's backward rule (tests/_mlp_backward_spec.py) against itself and against f64: the vector
form equals the literal scalar form, the generator reaches the edges it promises, the prefixes of one walk equal separate
walks, and the accuracy numbers the header quotes.  No GPU."""

import numpy as np
import pytest
from _mlp_backward_spec import (MLP_GRAD_BOUNDS, NAMES, RELU, TANH, bits32, make_mlp_backward_case, mlp_backward_scalar,
                                mlp_backward_spec, reference_f64)
from _mlp_spec import linear_init, mlp_spec

F32 = np.float32


@pytest.mark.parametrize("L, H, O, act, M", ((3, 16, 2, TANH, 70), (2, 16, 1, RELU, 300), (1, 16, 3, TANH, 513)))
def test_vector_form_equals_the_scalar_form(L, H, O, act, M):
    c = make_mlp_backward_case(M, L, H, O, act, seed=L + M)
    a = mlp_backward_spec(c["x"], c["hidden"], c["grad_y"], c["w2"], act)
    b = mlp_backward_scalar(c["x"], c["hidden"], c["grad_y"], c["w2"], act)
    for name in NAMES + ("ga",):
        assert a[name].shape == b[name].shape and a[name].dtype == F32, name
        np.testing.assert_array_equal(bits32(a[name]), bits32(b[name]), err_msg=name)
        assert np.isfinite(a[name]).all(), name


def test_the_generator_reaches_the_edges():
    c = make_mlp_backward_case(300, 38, 64, 5, TANH, seed=1)
    assert (np.abs(c["hidden"]) == 1.0).any()                            # pre-activations beyond the clamp: d = 0
    x = c["x"]
    assert (bits32(x) == 0x80000000).any() and ((x != 0) & (np.abs(x) < 1.1754944e-38)).any()   # -0.0 and subnormals
    gy = c["grad_y"]
    assert (bits32(gy[::5]) == 0).all() and (np.abs(gy) > 1e12).any() and (bits32(gy) == 0x80000000).any()
    r = make_mlp_backward_case(300, 18, 16, 1, RELU, seed=1)
    hb = bits32(r["hidden"])
    assert (hb[::7, 5] == 0).all() and (hb[::7, 6] == 0x80000000).all()
    ga = mlp_backward_spec(r["x"], r["hidden"], r["grad_y"], r["w2"], RELU)["ga"]
    assert not bits32(ga[::7, 5:7]).any()                                # h = +-0.0: the select gives +0.0
    nan_h = r["hidden"].copy()
    nan_h[3, 2] = np.nan
    assert bits32(mlp_backward_spec(r["x"], nan_h, r["grad_y"], r["w2"], RELU)["ga"])[3, 2] == 0   # a NaN h gives +0.0f


def test_prefixes_of_one_walk_equal_separate_walks():
    c = make_mlp_backward_case(600, 7, 48, 3, TANH, seed=4)
    rows = (1, 255, 256, 257, 600)
    many = mlp_backward_spec(c["x"], c["hidden"], c["grad_y"], c["w2"], TANH, rows=rows)
    for m in rows:
        one = mlp_backward_spec(c["x"][:m], c["hidden"][:m], c["grad_y"][:m], c["w2"], TANH)
        for name in NAMES + ("ga",):
            np.testing.assert_array_equal(bits32(many[m][name]), bits32(one[name]), err_msg=f"{name}, {m} rows")


def test_gradients_against_the_f64_composition():
    L, H, O, M = 38, 64, 5, 20_000
    worst = dict.fromkeys(NAMES, 0.0)
    for seed, act in ((0, TANH), (1, RELU)):
        w1t, b1, w2, b2 = linear_init(L, H, O, seed)
        rng = np.random.default_rng(200 + seed)
        x = rng.integers(0, 21, size=(M, L)).astype(F32)                 # observation-like rows: small whole numbers
        _, hidden = mlp_spec(x, w1t, b1, w2, b2, act)
        gy = rng.standard_normal((M, O)).astype(F32)
        got, want = mlp_backward_spec(x, hidden, gy, w2, act), reference_f64(x, hidden, gy, w2, act)
        for name in NAMES:
            err = np.abs(got[name].astype(np.float64) - want[name]) / np.maximum(1.0, np.abs(want[name]))
            worst[name] = max(worst[name], float(err.max()))
    for name in NAMES:
        print(f"grad_{name} (L = 38, H = 64, O = 5, M = 20000): max |err| / max(1, |f64|) = {worst[name]:.3e} "
              f"(bound {MLP_GRAD_BOUNDS[name]:.1e})")
    for name in NAMES:
        assert worst[name] <= MLP_GRAD_BOUNDS[name], name
        assert MLP_GRAD_BOUNDS[name] <= 2.0 * worst[name] * 1.05, name   # the recorded bound is the doubled maximum, no more
