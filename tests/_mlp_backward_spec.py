"""The backward rule of CCX_MLP as include/ccx.h states it, restated in NumPy on the CPU, plus a generator of cases.  TEST
INFRASTRUCTURE ONLY: what ``ccx_mlp_backward`` and csrc/ccx_mlp_grad.h are compared with.

Written from the header paragraph, not from the kernel.  ``mlp_backward_spec`` computes ``ga`` for every row at once with
elementwise ``np.float32`` operations (one rounding each, a Python loop over the outputs), accumulates every block's
partials as an f64 outer product per row -- one exact multiplication and ONE addition per element and row, a Python loop
over the rows, no ``@``, no ``sum``, nothing a library could reorder -- and applies ``_ppo_loss_spec.final_sum`` per output
element.  ``mlp_backward_scalar`` is the paragraph's pseudo-code, one addition at a time.  Every comparison against this
module is on bit patterns."""

from __future__ import annotations

import numpy as np
from _mlp_spec import F32, ONE, RELU, TANH, ZERO, bits32, bits32c, make_mlp_case, mlp_spec  # noqa: F401  (re-exported)
from _ppo_loss_spec import final_sum

F64 = np.float64
BLOCK = 256
NAMES = ("w1t", "b1", "w2", "b2")

# Accuracy against NumPy f64, measured on the CPU by tests/test_mlp_backward_spec.py (the maxima it prints) and DOUBLED for
# the inputs its samples did not hit, as max |err| / max(1, |f64 value|) against the textbook f64 composition on the same
# f32 x, hidden, grad_y and w2: L = 38, H = 64, O = 5, Linear-style weights, observation-like rows, M = 20 000, both
# activations.  Measured: grad_w1t 1.43e-5, grad_b1 1.81e-6, grad_w2 5.73e-8,
# grad_b2 4.56e-8 (grad_w1t and grad_b1 carry the f32 roundings of gh and ga through sums that cancel; grad_w2 and grad_b2 are
# f64 sums of exact terms, rounded once).  The header paragraph and DESIGN.md quote the same numbers.
MLP_GRAD_BOUNDS = dict(w1t=2.9e-5, b1=3.7e-6, w2=1.2e-7, b2=9.2e-8)


def ga_spec(hidden, grad_y, w2, activation=TANH):
    """ga f32 [M, H]: steps 1 and 2 of the rule for every row at once, one f32 operation per line."""
    h, gy, w2 = (np.asarray(v, F32) for v in (hidden, grad_y, w2))
    O = w2.shape[0]
    with np.errstate(all="ignore"):
        gh = gy[:, 0, None] * w2[None, 0, :]
        for o in range(1, O):
            gh = gh + gy[:, o, None] * w2[None, o, :]
        if activation == RELU:
            return np.where(h > ZERO, gh, ZERO).astype(F32)              # NaN > 0 is false: +0.0
        hh = h * h
        d = ONE - hh
        return (gh * d).astype(F32)


def block_chains(left, right, upto=None):
    """f64 [B, A, C]: for every block of 256 consecutive rows the chain of left[r][a] * right[r][c] over its rows in
    ascending order, from +0.0.  ``upto``: a sorted list of row counts; then a dict {M: [B_M, A, C]} of the partials of the
    first M rows for each (a chain's state after its first rows IS the partial of the shorter array)."""
    l64, r64 = np.asarray(left, F32).astype(F64), np.asarray(right, F32).astype(F64)
    M = l64.shape[0]
    want = sorted(set(upto)) if upto is not None else [M]
    assert want[-1] <= M and want[0] >= 1
    done, out = [], {}
    acc = np.zeros((l64.shape[1], r64.shape[1]), F64)
    with np.errstate(all="ignore"):
        for r in range(want[-1]):
            if r % BLOCK == 0 and r:
                done.append(acc)
                acc = np.zeros_like(acc)
            p = l64[r][:, None] * r64[r][None, :]                        # exact: 48 significant bits at most
            acc = acc + p                                                # the one addition
            if r + 1 in want:
                out[r + 1] = np.stack(done + [acc])
    return out if upto is not None else out[M]


def final_elements(P):
    """f32 [...]: ``final_sum`` over axis 0 of P f64 [B, ...] for every element, rounded to f32 once."""
    flat = P.reshape(P.shape[0], -1)
    with np.errstate(all="ignore"):
        s = np.array([final_sum(flat[:, e]) for e in range(flat.shape[1])], F64)
        return s.astype(F32).reshape(P.shape[1:])


def mlp_backward_spec(x, hidden, grad_y, w2, activation=TANH, rows=None):
    """dict(w1t, b1, w2, b2, ga) of the rule.  ``rows``: a list of row counts; then {M: that dict for the first M rows}
    (the chains are walked once)."""
    x, hidden, grad_y, w2 = (np.asarray(v, F32) for v in (x, hidden, grad_y, w2))
    M = x.shape[0]
    assert hidden.shape[0] == M and grad_y.shape == (M, w2.shape[0]) and w2.shape[1] == hidden.shape[1]
    ga = ga_spec(hidden, grad_y, w2, activation)
    ones = np.ones((M, 1), F32)
    want = [M] if rows is None else list(rows)
    first = block_chains(np.concatenate([x, ones], 1), ga, want)         # [B, L + 1, H]: grad_w1t, and grad_b1 as row L
    second = block_chains(grad_y, np.concatenate([hidden, ones], 1), want)   # [B, O, H + 1]: grad_w2, grad_b2 as column H
    out = {}
    for m in want:
        a, b = final_elements(first[m]), final_elements(second[m])
        out[m] = dict(w1t=a[:-1], b1=a[-1], w2=np.ascontiguousarray(b[:, :-1]), b2=np.ascontiguousarray(b[:, -1]), ga=ga[:m])
    return out if rows is not None else out[M]


def mlp_backward_scalar(x, hidden, grad_y, w2, activation=TANH):
    """The paragraph's pseudo-code, one row, one element and one addition at a time."""
    x, hidden, grad_y, w2 = (np.asarray(v, F32) for v in (x, hidden, grad_y, w2))
    M, L = x.shape
    H, O = hidden.shape[1], w2.shape[0]
    B = -(-M // BLOCK)
    ga = np.empty((M, H), F32)
    with np.errstate(all="ignore"):
        for r in range(M):
            for j in range(H):
                gh = F32(grad_y[r, 0] * w2[0, j])
                for o in range(1, O):
                    gh = F32(gh + F32(grad_y[r, o] * w2[o, j]))
                h = hidden[r, j]
                if activation == RELU:
                    ga[r, j] = gh if h > ZERO else ZERO
                else:
                    hh = F32(h * h)
                    d = F32(ONE - hh)
                    ga[r, j] = F32(gh * d)

        def halve(s):
            for o in (32, 16, 8, 4, 2, 1):
                s = [F64(s[j]) + F64(s[j ^ o]) for j in range(64)]
            return s[0]

        def reduce(term):
            P = []
            for b in range(B):
                acc = F64(0.0)
                for r in range(b * BLOCK, min(M, (b + 1) * BLOCK)):
                    acc = F64(acc + term(r))
                P.append(acc)
            places = []
            for j in range(64):
                a = F64(0.0)
                for i in range(j, B, 64):
                    a = F64(a + P[i])
                places.append(a)
            return F32(halve(places))

        gw1t = np.array([[reduce(lambda r: F64(F64(x[r, k]) * F64(ga[r, j]))) for j in range(H)] for k in range(L)], F32)
        gb1 = np.array([reduce(lambda r: F64(ga[r, j])) for j in range(H)], F32)
        gw2 = np.array([[reduce(lambda r: F64(F64(grad_y[r, o]) * F64(hidden[r, j]))) for j in range(H)] for o in range(O)], F32)
        gb2 = np.array([reduce(lambda r: F64(grad_y[r, o])) for o in range(O)], F32)
    return dict(w1t=gw1t, b1=gb1, w2=gw2, b2=gb2, ga=ga)


def make_mlp_backward_case(M, L, H, O, activation=TANH, seed=0):
    """x, hidden (what the forward writes for x), grad_y and the parameters.  Built on ``make_mlp_case(adversarial=False)``:
    its rows bring pre-activations beyond +-40 (tanh: h = +-1, so d = 0), signed zeros and subnormals; relu units get
    h = +0.0 and h = -0.0 on every seventh row.  grad_y rows cycle through: exact zeros (rows that do not count arrive from
    ``ppo_loss_backward`` that way), the scale of a mean over many rows, standard normal, large magnitudes, and signed zeros
    with subnormals.  Everything is finite."""
    c = make_mlp_case(M, L, H, O, seed=seed, adversarial=False)
    rng = np.random.default_rng(seed + 77)
    _, hidden = mlp_spec(c["x"], c["w1t"], c["b1"], c["w2"], c["b2"], activation)
    if activation == RELU:
        hidden[::7, 5 % H] = F32(0.0)
        hidden[::7, 6 % H] = F32(-0.0)
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
            gy[r] = (rng.standard_normal(O) * 1e15).astype(F32)
        else:
            gy[r] = rng.choice(np.array([0.0, -0.0, 1e-40, -1e-40, 1e-45, 2.5], F32), size=O)
    assert np.isfinite(hidden).all() and np.isfinite(c["x"]).all()
    return dict(c, hidden=hidden, grad_y=gy)


def reference_f64(x, hidden, grad_y, w2, activation=TANH):
    """The textbook composition in f64 on the same f32 inputs."""
    x, h, gy, w2 = (np.asarray(v, F64) for v in (x, hidden, grad_y, w2))
    gh = gy @ w2
    ga = gh * (h > 0) if activation == RELU else gh * (1.0 - h * h)
    return dict(w1t=x.T @ ga, b1=ga.sum(0), w2=gy.T @ h, b2=gy.sum(0))
