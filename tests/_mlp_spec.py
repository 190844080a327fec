"""CCX_MLP as include/ccx.h states it, restated in NumPy on the CPU, plus a generator of cases.  TEST INFRASTRUCTURE ONLY:
what the perceptron kernels are compared with.

Written from the header paragraph, not from the kernel.  ``mlp_spec`` advances every row at once with elementwise
``np.float32`` operations (one IEEE binary32 rounding each: no reduction, no matrix product, nothing a library could
reassociate or fuse), a Python loop over ``k`` and over the 16 units of a group, and ``np.where`` for selects.
``mlp_scalar`` is the header's pseudo-code literally, one row and one unit at a time, with ``np.float32`` scalars.  Every
comparison against this module is on bit patterns."""

from __future__ import annotations

import numpy as np
from _sample_spec import bits32, exp_spec  # noqa: F401  (bits32 is re-exported for the tests)

F32 = np.float32
ZERO, ONE, CLAMP = F32(0.0), F32(1.0), F32(40.0)
GROUP = 16
TANH, RELU = 0, 1

# Accuracy against NumPy f64, measured on the CPU by tests/test_mlp_spec.py (the maxima it prints) and DOUBLED for the inputs
# its samples did not hit (measured: 9.07e-8 and 7.34e-7).  The header paragraph and DESIGN.md quote the same two numbers.
TANH_ABS_BOUND = 1.9e-7                # tanh_spec against f64 tanh, absolute
LOGIT_ABS_BOUND = 1.5e-6               # logits of L = 38, H = 64, O = 5, Linear-style weights, observation-like rows, absolute

# the shapes (L, H, O, activation) the host-rule and the GPU tests share
SHAPES = ((38, 64, 5, TANH), (18, 16, 1, RELU), (7, 48, 3, TANH), (262, 256, 8, TANH))


def bits32c(a) -> np.ndarray:
    """bits32 with every NaN mapped to one pattern: IEEE 754 leaves the sign and payload of a NaN an operation produces or
    passes on to the implementation (x86 makes inf * 0 a negative NaN, gfx950 a positive one), and so does CCX_MLP.  Where a
    NaN stands is compared exactly; so is every bit of everything else."""
    a = np.ascontiguousarray(a, F32)
    b = a.view(np.uint32).copy()
    b[np.isnan(a)] = 0x7FC00000
    return b


def relu_spec(a):
    return np.where(a < ZERO, ZERO, a).astype(F32)                       # NaN < 0 is false: NaN stays


def tanh_spec(a):
    a = np.asarray(a, F32)
    with np.errstate(all="ignore"):
        m0 = np.abs(a)
        m = np.where(m0 < CLAMP, m0, CLAMP).astype(F32)                  # (NaN: 40, selected away below)
        t = exp_spec(-(m + m))
        r = (ONE - t) / (ONE + t)
        return np.where(a != a, a, np.copysign(r, a)).astype(F32)


def mlp_spec(x, w1t, b1, w2, b2, activation=TANH):
    """(y f32 [M, O], hidden f32 [M, H]) of rows x f32 [M, L]; every row at once, one f32 operation per line."""
    x, w1t, b1, w2, b2 = (np.asarray(v, F32) for v in (x, w1t, b1, w2, b2))
    M, L = x.shape
    H, O = w1t.shape[1], w2.shape[0]
    assert w1t.shape == (L, H) and b1.shape == (H,) and w2.shape == (O, H) and b2.shape == (O,) and H % GROUP == 0
    with np.errstate(all="ignore"):
        a = np.broadcast_to(b1, (M, H)).astype(F32)
        for k in range(L):                                               # layer 1: the chain over k, every unit at once
            a = a + x[:, k:k + 1] * w1t[k][None, :]
        h = relu_spec(a) if activation == RELU else tanh_spec(a)
        y = np.broadcast_to(b2, (M, O)).astype(F32)
        for g in range(H // GROUP):                                      # layer 2: partial of group g, then added in group order
            p = h[:, GROUP * g, None] * w2[None, :, GROUP * g]
            for i in range(1, GROUP):
                p = p + h[:, GROUP * g + i, None] * w2[None, :, GROUP * g + i]
            y = y + p
    return y.astype(F32), h.astype(F32)


def mlp_scalar(x, w1t, b1, w2, b2, activation=TANH):
    """The header's pseudo-code, one row and one unit at a time."""
    x = np.asarray(x, F32)
    M, L = x.shape
    H, O = w1t.shape[1], w2.shape[0]
    y, hid = np.empty((M, O), F32), np.empty((M, H), F32)
    with np.errstate(all="ignore"):
        for r in range(M):
            for j in range(H):
                a = F32(b1[j])
                for k in range(L):
                    a = F32(a + F32(x[r, k] * w1t[k, j]))
                if activation == RELU:
                    hid[r, j] = ZERO if a < ZERO else a
                elif a != a:
                    hid[r, j] = a
                else:
                    m = abs(a) if abs(a) < CLAMP else CLAMP
                    t = F32(exp_spec(F32(-F32(m + m))))
                    hid[r, j] = np.copysign(F32(F32(ONE - t) / F32(ONE + t)), a)
            for o in range(O):
                acc = F32(b2[o])
                for g in range(H // GROUP):
                    p = F32(hid[r, GROUP * g] * w2[o, GROUP * g])
                    for i in range(1, GROUP):
                        p = F32(p + F32(hid[r, GROUP * g + i] * w2[o, GROUP * g + i]))
                    acc = F32(acc + p)
                y[r, o] = acc
    return y, hid


def linear_init(L, H, O, seed=0):
    """Parameters in the kernel's layout with torch.nn.Linear's initial distribution (uniform in +-1/sqrt(fan_in))."""
    rng = np.random.default_rng(seed)
    k1, k2 = 1.0 / np.sqrt(L), 1.0 / np.sqrt(H)
    return (rng.uniform(-k1, k1, (L, H)).astype(F32), rng.uniform(-k1, k1, H).astype(F32),
            rng.uniform(-k2, k2, (O, H)).astype(F32), rng.uniform(-k2, k2, O).astype(F32))


def make_mlp_case(M, L, H, O, seed=0, adversarial=True):
    """Rows and parameters for CCX_MLP.  Rows cycle through: integer-valued inputs up to 100 (as observation rows are),
    standard normal, rows scaled so that pre-activations pass +-40, tiny and signed-zero inputs, and (``adversarial``) rows
    holding a NaN, a +inf or a -inf.  Weights are Linear-style, with a few units made large, -0.0 and subnormal."""
    rng = np.random.default_rng(seed)
    w1t, b1, w2, b2 = linear_init(L, H, O, seed + 1)
    w1t[:, 1] *= F32(50.0)                                               # a unit whose pre-activation leaves +-40
    w1t[:, 2] = rng.choice(np.array([0.0, -0.0, 1e-40, -1e-42], F32), size=L)
    b1[2] = F32(-0.0)
    w2[:, 3] = F32(-0.0)
    x = np.empty((M, L), F32)
    for r in range(M):
        kind = r % 6
        if kind in (0, 1):
            x[r] = rng.integers(0, 101, size=L).astype(F32)
        elif kind == 2:
            x[r] = rng.standard_normal(L).astype(F32)
        elif kind == 3:
            x[r] = (rng.standard_normal(L) * 300.0).astype(F32)
        elif kind == 4:
            x[r] = rng.choice(np.array([0.0, -0.0, 1e-40, -1e-40, 1e-45, 3e-39], F32), size=L)
        else:
            x[r] = rng.integers(-3, 4, size=L).astype(F32)
            if adversarial:
                x[r, rng.integers(0, L)] = rng.choice(np.array([np.nan, np.inf, -np.inf], F32))
    return dict(x=x, w1t=w1t, b1=b1, w2=w2, b2=b2)


def reference_f64(x, w1t, b1, w2, b2, activation=TANH):
    """The f64 composition on the same f32 inputs."""
    a = np.asarray(x, np.float64) @ np.asarray(w1t, np.float64) + np.asarray(b1, np.float64)
    h = np.maximum(a, 0.0) if activation == RELU else np.tanh(a)
    return h @ np.asarray(w2, np.float64).T + np.asarray(b2, np.float64)
