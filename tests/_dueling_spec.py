"""CCX_DUELING (include/ccx.h) in NumPy f32, one operation per line: the dueling combine of rows ``va`` f32 [..., 6] (five
advantages, then the state value) to Q-values f32 [..., 5], and its backward, a pure function of ``grad_q``.  Every line is
one f32 operation on f32 arrays, which NumPy rounds once: the order of the sums is the header's."""

import numpy as np

F32 = np.float32
# tests/test_dueling_spec.py measures the spec against torch f64 (q 4.8e-4, grad_va 6.1e-5: the cancellation in va_k - mean
# and in the sum where a row's entries are large against the result); the header and the README quote these, the maxima doubled
DUELING_Q_BOUND = 9.6e-4
DUELING_GRAD_BOUND = 1.3e-4


def dueling_spec(va):
    va = np.asarray(va)
    assert va.dtype == F32 and va.shape[-1] == 6
    with np.errstate(all="ignore"):
        s = va[..., 0] + va[..., 1]
        s = s + va[..., 2]
        s = s + va[..., 3]
        s = s + va[..., 4]
        mean = s / F32(5.0)
        q = np.empty(va.shape[:-1] + (5,), F32)
        for k in range(5):
            c = va[..., k] - mean
            q[..., k] = va[..., 5] + c
    return q


def dueling_backward_spec(grad_q):
    g = np.asarray(grad_q)
    assert g.dtype == F32 and g.shape[-1] == 5
    with np.errstate(all="ignore"):
        t = g[..., 0] + g[..., 1]
        t = t + g[..., 2]
        t = t + g[..., 3]
        t = t + g[..., 4]
        gm = t / F32(5.0)
        gva = np.empty(g.shape[:-1] + (6,), F32)
        for k in range(5):
            gva[..., k] = g[..., k] - gm
        gva[..., 5] = t
    return gva


def make_dueling_rows(M: int, seed: int = 0, special: bool = False):
    """``va`` f32 [M, 6] and a cotangent f32 [M, 5]: advantages ~ N(0, 1) * 10^U(-3, 3), in a third of the rows with a
    common offset of ten times the row's scale; values ~ N(0, 1) * 10^U(-2, 2).  ``special``: the first rows also hold +-0,
    +-inf, NaN and subnormals."""
    rng = np.random.default_rng(seed)
    scale = 10.0 ** rng.uniform(-3, 3, (M, 1))
    adv = rng.standard_normal((M, 5)) * scale
    adv += (rng.random((M, 1)) < 1 / 3) * rng.standard_normal((M, 1)) * scale * 10.0
    val = rng.standard_normal((M, 1)) * 10.0 ** rng.uniform(-2, 2, (M, 1))
    va = np.concatenate([adv, val], -1).astype(F32)
    g = (rng.standard_normal((M, 5)) * 10.0 ** rng.uniform(-3, 3, (M, 1))).astype(F32)
    if special:
        odd = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, 1e-45, -1e-45, 1e-39, 3e38, -3e38, 1.0], F32)
        n = min(M, 4 * len(odd))
        for i in range(n):
            va[i, rng.integers(0, 6)] = odd[i % len(odd)]
            g[i, rng.integers(0, 5)] = odd[(i + 3) % len(odd)]
        if M > n + 4:
            va[n] = 0.0
            va[n + 1] = -0.0
            g[n] = 0.0
            g[n + 1] = -0.0
            va[n + 2] = F32(1e-45)
            g[n + 2] = F32(-1e-45)
    return va, g
