"""The NumPy restatement of CCX_MLP (tests/_mlp_spec.py) against itself and against f64: the vector form equals the literal
scalar form, the accuracy numbers the header quotes, and a row's outputs do not depend on its neighbours.  No GPU."""

import numpy as np
import pytest
from _mlp_spec import (LOGIT_ABS_BOUND, RELU, TANH, TANH_ABS_BOUND, bits32, linear_init, make_mlp_case, mlp_scalar, mlp_spec,
                       reference_f64, relu_spec, tanh_spec)

F32 = np.float32


@pytest.mark.parametrize("L, H, O, act", ((7, 48, 3, TANH), (18, 16, 1, RELU), (38, 64, 5, TANH)))
def test_vector_form_equals_the_scalar_form(L, H, O, act):
    M = 240 if L < 38 else 60
    c = make_mlp_case(M, L, H, O, seed=L)
    y, hid = mlp_spec(c["x"], c["w1t"], c["b1"], c["w2"], c["b2"], act)
    ys, hs = mlp_scalar(c["x"], c["w1t"], c["b1"], c["w2"], c["b2"], act)
    np.testing.assert_array_equal(bits32(hid), bits32(hs))
    np.testing.assert_array_equal(bits32(y), bits32(ys))
    assert np.isnan(y).any() and np.isfinite(y).any()                    # the generator's poisoned rows reach the logits
    if act == TANH:
        assert (np.abs(hid) == 1.0).any()                                # pre-activations beyond the clamp


def test_activation_edge_values():
    a = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, 40.0, -40.0, 39.999996, 1e30, -1e-45, 1e-45, 20.0], F32)
    t = tanh_spec(a)
    np.testing.assert_array_equal(bits32(t[:4]), bits32(np.array([0.0, -0.0, 1.0, -1.0], F32)))
    assert np.isnan(t[4]) and bits32(t[4:5])[0] == bits32(a[4:5])[0]      # the NaN itself, selected
    np.testing.assert_array_equal(bits32(t[5:9]), bits32(np.array([1.0, -1.0, 1.0, 1.0], F32)))
    np.testing.assert_array_equal(bits32(t[9:11]), bits32(np.array([-0.0, 0.0], F32)))   # t rounds to 1: a signed zero
    assert t[11] == 1.0
    r = relu_spec(a)
    np.testing.assert_array_equal(bits32(r[:4]), bits32(np.array([0.0, -0.0, np.inf, 0.0], F32)))
    assert np.isnan(r[4]) and bits32(r[9:10])[0] == 0


def test_tanh_spec_against_f64():
    rng = np.random.default_rng(3)
    a = np.concatenate([rng.uniform(-12, 12, 2_000_000), rng.standard_normal(1_500_000),
                        np.exp(rng.uniform(np.log(1e-8), np.log(12.0), 1_000_000)) * rng.choice([-1.0, 1.0], 1_000_000)]).astype(F32)
    err = np.abs(tanh_spec(a).astype(np.float64) - np.tanh(a.astype(np.float64))).max()
    print(f"tanh_spec: max |err| against f64 tanh over {a.size} points = {err:.3e} (bound {TANH_ABS_BOUND:.1e})")
    assert err <= TANH_ABS_BOUND
    assert TANH_ABS_BOUND <= 2.0 * err * 1.05                            # the recorded bound is the doubled maximum, no more


def test_logits_against_the_f64_composition():
    L, H, O = 38, 64, 5
    worst = 0.0
    for seed in range(4):
        w1t, b1, w2, b2 = linear_init(L, H, O, seed)
        rng = np.random.default_rng(100 + seed)
        x = rng.integers(0, 21, size=(4096, L)).astype(F32)              # observation-like rows: small whole numbers
        y, _ = mlp_spec(x, w1t, b1, w2, b2, TANH)
        worst = max(worst, float(np.abs(y.astype(np.float64) - reference_f64(x, w1t, b1, w2, b2, TANH)).max()))
    print(f"logits (L = 38, H = 64, O = 5): max |err| against the f64 composition = {worst:.3e} (bound {LOGIT_ABS_BOUND:.1e})")
    assert worst <= LOGIT_ABS_BOUND
    assert LOGIT_ABS_BOUND <= 2.0 * worst * 1.05


@pytest.mark.parametrize("act", (TANH, RELU))
def test_a_row_does_not_depend_on_its_neighbours(act):
    c = make_mlp_case(97, 38, 64, 5, seed=9)
    p = (c["w1t"], c["b1"], c["w2"], c["b2"], act)
    y, hid = mlp_spec(c["x"], *p)
    for r in (0, 5, 41, 96):
        y1, h1 = mlp_spec(c["x"][r:r + 1], *p)
        np.testing.assert_array_equal(bits32(y1[0]), bits32(y[r]))
        np.testing.assert_array_equal(bits32(h1[0]), bits32(hid[r]))
    perm = np.random.default_rng(1).permutation(97)
    y2, h2 = mlp_spec(c["x"][perm], *p)
    np.testing.assert_array_equal(bits32(y2), bits32(y[perm]))
    np.testing.assert_array_equal(bits32(h2), bits32(hid[perm]))
