"""The NumPy statement of CCX_DUELING (tests/_dueling_spec.py) against an independent statement -- the textbook composition
``v + a - a.mean(-1)`` in torch f64 with autograd, on the same f32 inputs (accuracy, with the bounds the header quotes) -- and
the identities of the rule.  No GPU."""

import numpy as np
from _dueling_spec import DUELING_GRAD_BOUND, DUELING_Q_BOUND, dueling_backward_spec, dueling_spec, make_dueling_rows
from _sample_spec import bits32

F32 = np.float32
ROWS = 20_000


def test_against_torch_f64():
    """max |err| / max(1, |f64 value|) over 20 000 random rows: advantages ~ N(0, 1) * 10^U(-3, 3), a third of the rows with
    a common offset ten times their scale, so the subtraction of the mean cancels.  The bounds are the measured maxima
    doubled (the project's convention): the spec's error against f64, not a kernel's."""
    import torch

    va, g = make_dueling_rows(ROWS, seed=7)
    q = dueling_spec(va)
    gva = dueling_backward_spec(g)
    x = torch.from_numpy(va).double().requires_grad_()
    a, v = x[:, :5], x[:, 5:]
    q64 = v + a - a.mean(-1, keepdim=True)
    (g64,) = torch.autograd.grad(q64, x, torch.from_numpy(g).double())
    q64, g64 = q64.detach().numpy(), g64.numpy()
    err_q = float((np.abs(q.astype(np.float64) - q64) / np.maximum(1.0, np.abs(q64))).max())
    err_g = float((np.abs(gva.astype(np.float64) - g64) / np.maximum(1.0, np.abs(g64))).max())
    print(f"measured against torch f64: q {err_q:.3g}, grad_va {err_g:.3g} (the bounds are these doubled)")
    assert 0 < err_q <= DUELING_Q_BOUND and 0 < err_g <= DUELING_GRAD_BOUND
    assert np.isfinite(q).all() and np.isfinite(gva).all()


def test_the_bounds_are_the_ones_the_documents_quote():
    from pathlib import Path

    root = Path(__file__).resolve().parent.parent
    for text in ((root / "include" / "ccx.h").read_text(), (root / "README.md").read_text()):
        assert f"q within {DUELING_Q_BOUND:.1e}" in text and f"grad_va within {DUELING_GRAD_BOUND:.1e}" in text


def test_five_equal_advantages_give_the_value():
    # s / 5 is exact for these: 5 a is representable and the quotient is a itself
    a = np.array([0.0, 1.0, -2.5, 3.0, 1024.0, 0.375, -1e-3, 7e8], F32)
    exact = (a * F32(5.0)).astype(np.float64) == a.astype(np.float64) * 5.0
    assert exact.sum() >= 6
    a = a[exact]
    v = np.linspace(-3, 3, len(a)).astype(F32)
    va = np.concatenate([np.repeat(a[:, None], 5, 1), v[:, None]], -1)
    q = dueling_spec(va)
    np.testing.assert_array_equal(bits32(q), bits32(np.repeat((v + F32(0.0))[:, None], 5, 1)))


def test_zero_gradient_rows_get_positive_zeros():
    g = np.zeros((3, 5), F32)
    gva = dueling_backward_spec(g)
    assert gva.shape == (3, 6) and not bits32(gva).any()                 # +0.0f: no bit set, the sign bit included
    mixed = np.array([[1.0, 0, 0, 0, 0], [0, 0, 0, 0, 0]], F32)
    assert dueling_backward_spec(mixed)[0].any() and not bits32(dueling_backward_spec(mixed)[1]).any()


def test_the_backward_is_the_transpose_of_the_forward():
    """The combine is linear: <dueling(e_i), g> == <e_i, backward(g)> on small integers, where every operation is exact
    but the two divisions by five -- so compare against the exact matrix instead."""
    J = np.zeros((5, 6))
    J[:, :5] = np.eye(5) - 0.2
    J[:, 5] = 1.0
    rng = np.random.default_rng(0)
    g = rng.integers(-8, 9, (50, 5)).astype(F32)
    want = g.astype(np.float64) @ J
    np.testing.assert_allclose(dueling_backward_spec(g), want, rtol=0, atol=2e-6)
    va = rng.integers(-8, 9, (50, 6)).astype(F32)
    np.testing.assert_allclose(dueling_spec(va), va.astype(np.float64) @ J.T, rtol=0, atol=2e-6)


def test_a_nan_stays_in_its_row():
    va, _ = make_dueling_rows(8, seed=1)
    va[3, 2] = np.nan
    q = dueling_spec(va)
    assert np.isnan(q[3]).all() and np.isfinite(np.delete(q, 3, 0)).all()
    va[3, 2] = 1.0
    va[5, 5] = np.nan                                                     # the value reaches its row's five too
    q = dueling_spec(va)
    assert np.isnan(q[5]).all() and np.isfinite(np.delete(q, 5, 0)).all()


def test_the_mean_runs_over_all_five_actions():
    va = np.array([[1, 2, 3, 4, 100, 0.5]], F32)
    np.testing.assert_array_equal(dueling_spec(va), np.array([[-21 + 0.5, -20 + 0.5, -19 + 0.5, -18 + 0.5, 78 + 0.5]], F32))
