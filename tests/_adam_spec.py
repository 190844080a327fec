"""CCX_ADAM as include/ccx.h states it, restated in NumPy on the CPU.  TEST INFRASTRUCTURE ONLY: what the optimiser kernels
and the host build of csrc/ccx_adam.h are compared with.

f32 values are ``np.float32`` scalars and arrays, handled operation by operation (one rounding each); the f64 scalars of
steps 2 and 4 are ``np.float64``; selects are ``np.where`` or Python branches on per-call conditions, never a multiplication
by zero.  The tree is ``_ppo_loss_spec.tree_sum`` on the padded sequence.  Every comparison against this module is on bit
patterns."""

from __future__ import annotations

import numpy as np
from _ppo_loss_spec import tree_sum

F32 = np.float32
F64 = np.float64
MAX_TENSORS = 32
NORM_EPS = F32(1e-6)

# Accuracy against f64, measured on the CPU by tests/test_adam_spec.py (the maxima it prints) and DOUBLED, as
# max |err| / max(1, |f64 value|) against torch.optim.AdamW / Adam with clip_grad_norm_ in f64 on the same f32 gradients:
# 50 steps on the two-head set (lr 3e-4, max_grad_norm 0.5), 17 of them clipped.  Measured: parameters 3.89e-7 without
# weight decay and 2.37e-6 with weight_decay = 0.01 (the worst element sits near -1.1 with a small gradient: p - p * lrwd
# rounds the same way step after step while p hardly moves, 5e-8 a step; the root mean square error is 3.2e-7), m 1.38e-9,
# v 3.34e-11 (|m| and |v| are far below 1 here, so these two are absolute errors).  include/ccx.h, DESIGN.md and the README
# quote the doubled numbers.
ADAM_PARAM_BOUND = 7.8e-7
ADAM_PARAM_BOUND_DECAY = 4.8e-6
ADAM_M_BOUND = 2.8e-9
ADAM_V_BOUND = 6.7e-11

# the two heads of the examples: actor Linear(38, 64) -> Linear(64, 5), critic Linear(38, 64) -> Linear(64, 1)
TWO_HEADS = (38 * 64, 64, 320, 5, 38 * 64, 64, 64, 1)


def bits32(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


def new_state():
    """The 64 state bytes of a fresh optimiser, as a dict."""
    return dict(pow1=F64(1.0), pow2=F64(1.0), step=0, skipped=0)


def state_bytes(state):
    """The 64 bytes on the device: f64 pow1, f64 pow2, i64 step, i64 skipped, 32 zero bytes."""
    out = np.zeros(64, np.uint8)
    out[0:16] = np.array([state["pow1"], state["pow2"]], F64).view(np.uint8)
    out[16:32] = np.array([state["step"], state["skipped"]], np.int64).view(np.uint8)
    return out


def padded_squares(grads):
    """The virtual sequence: per tensor the exact f64 squares, padded with +0.0 to a multiple of 256 places."""
    parts = []
    for g in grads:
        d = np.asarray(g, F32).reshape(-1).astype(F64)
        sq = np.zeros(-(-d.size // 256) * 256, F64)
        sq[:d.size] = d * d
        parts.append(sq)
    return np.concatenate(parts)


def sum_of_squares(grads):
    with np.errstate(all="ignore"):
        return tree_sum(padded_squares(grads))


def adam_step_spec(params, grads, ms, vs, state, lr, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.0, max_grad_norm=0.0):
    """One step.  ``params`` / ``ms`` / ``vs``: lists of f32 arrays, updated IN PLACE; ``grads``: a list of f32 arrays, read;
    ``state``: :func:`new_state`'s dict, advanced in place; ``lr``: the rate in force (the by-value argument or the device
    scalar).  Returns ``stats`` f32 [4]."""
    assert 1 <= len(params) <= MAX_TENSORS and len(params) == len(grads) == len(ms) == len(vs)
    lr, beta1, beta2, eps, wd, mgn = F32(lr), F32(beta1), F32(beta2), F32(eps), F32(weight_decay), F32(max_grad_norm)
    with np.errstate(all="ignore"):
        # 1, 2
        S = sum_of_squares(grads)
        nd = np.sqrt(F64(S))
        gn = F32(nd)
        skip = bool(np.isnan(gn) or np.isinf(gn))
        # 3
        has_clip = bool(mgn > 0)
        scale = F32(1.0)
        if has_clip:
            den = gn + NORM_EPS
            c = mgn / den
            scale = c if c < F32(1.0) else F32(1.0)
        stats = np.array([gn, scale, F32(1.0) if skip else F32(0.0), lr], F32)
        if skip:
            state["skipped"] += 1
            return stats
        # 4
        state["pow1"] = F64(state["pow1"]) * F64(beta1)
        state["pow2"] = F64(state["pow2"]) * F64(beta2)
        state["step"] += 1
        bc1 = F32(F64(1.0) - state["pow1"])
        bc2 = F32(F64(1.0) - state["pow2"])
        omb1 = F32(F64(1.0) - F64(beta1))
        omb2 = F32(F64(1.0) - F64(beta2))
        lrwd = lr * wd
        # 5
        for p, g, m, v in zip(params, grads, ms, vs):
            assert p.dtype == F32 and m.dtype == F32 and v.dtype == F32
            g = np.asarray(g, F32).reshape(p.shape)
            gs = g * scale if has_clip else g
            pd = p - p * lrwd if wd != 0 else p
            mn = beta1 * m + omb1 * gs
            gg = gs * gs
            vn = beta2 * v + omb2 * gg
            mh = mn / bc1
            vh = vn / bc2
            dn = np.sqrt(vh) + eps
            u = mh / dn
            pn = pd - lr * u
            assert pn.dtype == F32 and mn.dtype == F32 and vn.dtype == F32
            p[...] = pn
            m[...] = mn
            v[...] = vn
    return stats


def make_adam_case(numels, seed, steps=3, grad_scale=1.0):
    """Parameters and ``steps`` gradient lists for tensors of the sizes ``numels``: magnitudes spread over several decades,
    a few exact zeros and subnormals among the gradients."""
    rng = np.random.default_rng(seed)
    params = [(rng.standard_normal(n) * 0.3).astype(F32) for n in numels]
    grads = []
    for _ in range(steps):
        gl = []
        for n in numels:
            g = (rng.standard_normal(n) * np.exp(rng.uniform(-6, 1, n)) * grad_scale).astype(F32)
            g[rng.random(n) < 0.05] = 0.0
            g[rng.random(n) < 0.02] = F32(1e-41)
            g[0] = F32(rng.uniform(0.05, 0.5) * grad_scale)               # (so that no tensor's gradient is all zero)
            gl.append(g)
        grads.append(gl)
    return params, grads


def run_spec(params, grad_steps, lrs, **hyper):
    """The spec over consecutive steps from a fresh state; returns per step (params, ms, vs, state bytes, stats) copies."""
    params = [p.copy() for p in params]
    ms = [np.zeros_like(p) for p in params]
    vs = [np.zeros_like(p) for p in params]
    state = new_state()
    out = []
    for grads, lr in zip(grad_steps, lrs):
        stats = adam_step_spec(params, grads, ms, vs, state, lr, **hyper)
        out.append(([p.copy() for p in params], [m.copy() for m in ms], [v.copy() for v in vs], state_bytes(state), stats))
    return out
