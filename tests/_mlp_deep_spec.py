"""CCX_MLP_DEEP as include/ccx.h states it, in NumPy on the CPU, plus a generator of cases.  TEST INFRASTRUCTURE ONLY: what
the deep-head kernels and csrc/ccx_mlp_deep.h are compared with.

Composed from the specs of CCX_MLP (tests/_mlp_spec.py, tests/_mlp_backward_spec.py), which are not restated: the first
layer, the activations and the output layer are ``mlp_spec``'s, ga2 is ``ga_spec``'s, the block chains and the final step are
``block_chains`` / ``final_elements``.  What this module writes out itself is what the paragraph adds: the layer-2 chain
over ``k`` and the gh1 chain over ``j`` (with step 2's select / product on ``hidden1``), elementwise ``np.float32``
operations, one rounding each.  Every comparison against this module is on bit patterns."""

from __future__ import annotations

import numpy as np
from _mlp_backward_spec import block_chains, final_elements, ga_spec
from _mlp_spec import F32, ONE, RELU, TANH, ZERO, bits32c, linear_init, make_mlp_case, mlp_spec, relu_spec, tanh_spec  # noqa: F401

NAMES = ("w1t", "b1", "w2t", "b2", "w3", "b3")

# the catalogue (L, H1, H2, O) of the GPU tests and of the planner test
CATALOGUE = ((1, 16, 16, 1), (38, 64, 64, 5), (18, 16, 32, 5), (38, 48, 16, 6), (262, 256, 256, 8), (512, 16, 256, 1))

# Accuracy against IEEE f64 (torch f64 on the same f32 inputs, autograd for the gradients), measured on the CPU by
# tests/test_mlp_deep_spec.py (the maxima it prints) and DOUBLED for the inputs its samples did not hit: L = 38, O = 5,
# torch.nn.Linear's initial weights, observation-like rows, M = 20 000, the worse of tanh and relu.  The logits absolute; the
# gradients as max |err| / max(1, |f64 value|).  Keys: (H1, H2).  include/ccx.h and the README quote the same numbers.
# Measured, 64-64: logits 8.69e-7; w1t 9.28e-5, b1 3.02e-6, w2t 2.04e-5, b2 7.01e-7, w3 4.98e-5, b3 4.87e-8.
# Measured, 256-256: logits 1.32e-6; w1t 3.24e-3, b1 2.50e-4, w2t 7.14e-2, b2 4.07e-3, w3 7.87e-5, b3 4.87e-8.  The 256-256
# gradient figures of the first two layers are ONE relu unit of ONE row: its layer-2 pre-activation lies within f32 rounding
# of zero, so the f64 side (which forms its own masks) takes the other branch and that row's whole term moves the element.
# With tanh alone the same shape measures w1t 3.11e-5, b1 2.03e-6, w2t 8.82e-6, b2 3.75e-6, w3 5.06e-5.
DEEP_LOGIT_ABS_BOUNDS = {(64, 64): 1.74e-6, (256, 256): 2.6e-6}
DEEP_GRAD_BOUNDS = {(64, 64): dict(w1t=1.86e-4, b1=6.0e-6, w2t=4.1e-5, b2=1.4e-6, w3=1.0e-4, b3=9.7e-8),
                    (256, 256): dict(w1t=6.5e-3, b1=5.0e-4, w2t=1.43e-1, b2=8.1e-3, w3=1.57e-4, b3=9.7e-8)}


def layer2_spec(h1, w2t, b2, activation=TANH):
    """h2 f32 [M, H2]: a = b2[j]; for k = 0 .. H1-1 in order a = a + h1[k] * w2t[k][j]; act(a).  Every row and unit at once."""
    h1, w2t, b2 = (np.asarray(v, F32) for v in (h1, w2t, b2))
    with np.errstate(all="ignore"):
        a = np.broadcast_to(b2, (h1.shape[0], w2t.shape[1])).astype(F32)
        for k in range(w2t.shape[0]):
            a = a + h1[:, k:k + 1] * w2t[k][None, :]
        return relu_spec(a) if activation == RELU else tanh_spec(a)


def deep_spec(x, w1t, b1, w2t, b2, w3, b3, activation=TANH):
    """(y f32 [M, O], hidden1 f32 [M, H1], hidden2 f32 [M, H2]) of rows x f32 [M, L]."""
    w1t, w2t, w3 = (np.asarray(v, F32) for v in (w1t, w2t, w3))
    H1, O = w1t.shape[1], w3.shape[0]
    _, h1 = mlp_spec(x, w1t, b1, np.zeros((1, H1), F32), np.zeros(1, F32), activation)      # steps 1-2 of CCX_MLP
    h2 = layer2_spec(h1, w2t, b2, activation)
    y, h2_again = mlp_spec(h1, w2t, b2, w3, b3, activation)              # step 3 of CCX_MLP on h2: the rule's own identity
    assert np.array_equal(bits32c(h2), bits32c(h2_again)) and y.shape[1] == O
    return y, h1, h2


def ga1_spec(hidden1, ga2, w2t, activation=TANH):
    """ga1 f32 [M, H1]: gh1 = ga2[0] * w2t[i][0], then j = 1 .. H2-1 in order; then step 2's rule on hidden1."""
    h, ga2, w2t = (np.asarray(v, F32) for v in (hidden1, ga2, w2t))
    with np.errstate(all="ignore"):
        gh = ga2[:, 0, None] * w2t[None, :, 0]
        for j in range(1, w2t.shape[1]):
            gh = gh + ga2[:, j, None] * w2t[None, :, j]
        if activation == RELU:
            return np.where(h > ZERO, gh, ZERO).astype(F32)
        hh = h * h
        d = ONE - hh
        return (gh * d).astype(F32)


def deep_backward_spec(x, hidden1, hidden2, grad_y, w2t, w3, activation=TANH, rows=None):
    """dict(w1t, b1, w2t, b2, w3, b3, ga1, ga2) of the rule.  ``rows``: a list of row counts; then {M: that dict for the
    first M rows} (the chains are walked once)."""
    x, hidden1, hidden2, grad_y = (np.asarray(v, F32) for v in (x, hidden1, hidden2, grad_y))
    M = x.shape[0]
    ga2 = ga_spec(hidden2, grad_y, w3, activation)
    ga1 = ga1_spec(hidden1, ga2, w2t, activation)
    ones = np.ones((M, 1), F32)
    want = [M] if rows is None else list(rows)
    first = block_chains(np.concatenate([x, ones], 1), ga1, want)        # [B, L + 1, H1]
    second = block_chains(np.concatenate([hidden1, ones], 1), ga2, want)  # [B, H1 + 1, H2]
    third = block_chains(grad_y, np.concatenate([hidden2, ones], 1), want)    # [B, O, H2 + 1]
    out = {}
    for m in want:
        a, b, c = final_elements(first[m]), final_elements(second[m]), final_elements(third[m])
        out[m] = dict(w1t=a[:-1], b1=a[-1], w2t=b[:-1], b2=b[-1], w3=np.ascontiguousarray(c[:, :-1]),
                      b3=np.ascontiguousarray(c[:, -1]), ga1=ga1[:m], ga2=ga2[:m])
    return out if rows is not None else out[M]


def deep_init(L, H1, H2, O, seed=0):
    """The six parameters in the kernel's layout with torch.nn.Linear's initial distribution."""
    w1t, b1, _, _ = linear_init(L, H1, 1, seed)
    w2t, b2, w3, b3 = linear_init(H1, H2, O, seed + 1000)
    return dict(w1t=w1t, b1=b1, w2t=w2t, b2=b2, w3=w3, b3=b3)


def make_deep_case(M, L, H1, H2, O, seed=0, adversarial=True):
    """Rows and parameters: ``make_mlp_case``'s rows and first layer (NaN, +-inf, +-0, subnormals, pre-activations beyond
    +-40), a second layer with a large unit, a unit of signed zeros and subnormals and a -0.0 output column."""
    c = make_mlp_case(M, L, H1, 1, seed=seed, adversarial=adversarial)
    rng = np.random.default_rng(seed + 5)
    p = deep_init(L, H1, H2, O, seed + 2)
    p["w1t"], p["b1"] = c["w1t"], c["b1"]
    p["w2t"][:, 1] *= F32(60.0)
    p["w2t"][:, 2] = rng.choice(np.array([0.0, -0.0, 1e-40, -1e-42], F32), size=H1)
    p["b2"][2] = F32(-0.0)
    p["w3"][:, 3] = F32(-0.0)
    return dict(p, x=c["x"])


def make_deep_backward_case(M, L, H1, H2, O, activation=TANH, seed=0):
    """x, hidden1, hidden2 (what the forward writes), grad_y and the parameters; everything finite.  grad_y rows cycle as
    ``make_mlp_backward_case``'s do: exact zeros, tiny, standard normal, large, signed zeros with subnormals."""
    c = make_deep_case(M, L, H1, H2, O, seed=seed, adversarial=False)
    _, h1, h2 = deep_spec(c["x"], *(c[n] for n in NAMES), activation)
    if activation == RELU:
        h2[::7, 5 % H2], h2[::7, 6 % H2] = F32(0.0), F32(-0.0)
        h1[::5, 3 % H1], h1[::5, 4 % H1] = F32(0.0), F32(-0.0)
    rng = np.random.default_rng(seed + 77)
    gy = np.empty((M, O), F32)
    for r in range(M):
        kind = r % 5
        if kind == 0:
            gy[r] = ZERO
        elif kind == 1:
            gy[r] = (rng.standard_normal(O) * 1e-5).astype(F32)
        elif kind == 2:
            gy[r] = rng.standard_normal(O).astype(F32)
        elif kind == 3:
            gy[r] = (rng.standard_normal(O) * 1e12).astype(F32)
        else:
            gy[r] = rng.choice(np.array([0.0, -0.0, 1e-40, -1e-40, 1e-45, 2.5], F32), size=O)
    assert np.isfinite(h1).all() and np.isfinite(h2).all()
    return dict(c, hidden1=h1, hidden2=h2, grad_y=gy)
