"""CCX_EVALUATE as include/ccx.h states it, restated in NumPy on the CPU, plus a generator of adversarial cases.  TEST
INFRASTRUCTURE ONLY: what the evaluate kernels are compared with.

Built on tests/_sample_spec.py: steps 2-6 of CCX_SAMPLE (legal set, maximum, degenerate, d, w, c, S) are taken from
``sample_spec(..., details=True)`` itself, so the two rules cannot drift apart; everything behind them is written from the
CCX_EVALUATE paragraph with elementwise ``np.float32`` operations (one rounding each), selects by ``np.where``, never a
multiplication by zero.  ``evaluate_scalar`` / ``evaluate_backward_scalar`` are the header's pseudo-code, one row at a time.
Every comparison against this module is on bit patterns."""

from __future__ import annotations

import numpy as np
from _sample_spec import (ACTION_ABSENT, D_MIN, F32, NEG_INF, ONE, POS_INF, ZERO, exp_spec, log_spec, make_sample_case,
                          sample_spec)

# Accuracy against f64, measured on the CPU by tests/test_evaluate_spec.py (the maxima it prints) and DOUBLED, over the
# generator's rows that are not absent, not degenerate and whose stored action is legal with w_a > 0 (about 0.6 of all
# rows).  Every figure is max |err| / max(1, |f64 value|): a stored action, unlike a sampled one, may sit at d near -80,
# where one rounding of l_a - mx is already 3.8e-6 absolute, so logp is measured relative to its own size.  Measured:
# 1.98e-7, 1.97e-7, 2.04e-7, 1.80e-7.  The header paragraph and DESIGN.md 3.13 quote the same four numbers.
EVAL_LOGP_BOUND = 4.0e-7               # logp
EVAL_ENTROPY_BOUND = 4.0e-7            # entropy
EVAL_JAC_LOGP_BOUND = 4.1e-7           # d logp / d logits (grad_logp = 1 alone)
EVAL_JAC_ENTROPY_BOUND = 3.7e-7        # d entropy / d logits (grad_entropy = 1 alone)


def _steps_2_to_6(logits, masks):
    """The intermediates of CCX_SAMPLE's steps 2-6 for flat rows, from sample_spec itself (no slot dead, no draw made)."""
    logits = np.asarray(logits, F32)
    M = logits.shape[0]
    zeros = np.zeros((M, 1), np.uint8)
    counters = np.zeros(M, np.int32)
    _, _, entropy, det = sample_spec(logits.reshape(M, 1, 5), None if masks is None else np.asarray(masks).reshape(M, 1), zeros,
                                     zeros, counters, counters, deterministic=True, details=True)
    out = {k: v.reshape((M,) + v.shape[2:]) for k, v in det.items()}
    out["entropy"] = entropy.reshape(M)                                  # step 10
    return out


def _stored(actions, legal):
    a = np.asarray(actions, np.uint8).astype(np.int64)
    absent = a == ACTION_ABSENT
    in_range = a <= 4
    ai = np.where(in_range, a, 4)
    a_legal = in_range & np.take_along_axis(legal, ai[:, None], -1)[:, 0]
    return a, absent, ai, a_legal


def evaluate_spec(logits, actions, masks=None, want_entropy=True):
    """(logp f32 [M], entropy f32 [M] or None) for logits f32 [M, 5], actions u8 [M], masks u8 [M] or None."""
    s = _steps_2_to_6(logits, masks)
    a, absent, ai, a_legal = _stored(actions, s["legal"])
    with np.errstate(all="ignore"):
        ls = log_spec(s["S"])
        d_a = np.take_along_axis(s["d"], ai[:, None], -1)[:, 0]
        logp = np.where(absent, ZERO, np.where(a_legal, d_a - ls, NEG_INF)).astype(F32)
    entropy = np.where(absent, ZERO, s["entropy"]).astype(F32) if want_entropy else None
    return logp, entropy


def evaluate_backward_spec(logits, actions, masks, grad_logp, grad_entropy):
    """grad_logits f32 [M, 5]; either gradient (f32 [M]) may be None, not both."""
    assert grad_logp is not None or grad_entropy is not None
    s = _steps_2_to_6(logits, masks)
    a, absent, ai, a_legal = _stored(actions, s["legal"])
    legal, w, d, S = s["legal"], s["w"], s["d"], s["S"]
    with np.errstate(all="ignore"):
        p = (w / S[:, None]).astype(F32)
        ls = log_spec(S)
        lp = (d - ls[:, None]).astype(F32)
        H = s["entropy"]
        A = B = None
        if grad_logp is not None:
            t1 = (np.where(np.arange(5)[None, :] == a[:, None], ONE, ZERO) - p).astype(F32)
            A = np.where(a_legal[:, None], np.asarray(grad_logp, F32)[:, None] * t1, ZERO).astype(F32)
        if grad_entropy is not None:
            t2 = np.where(w == ZERO, ZERO, p * (lp + H[:, None])).astype(F32)
            B = (np.asarray(grad_entropy, F32)[:, None] * t2).astype(F32)
        g = A - B if (A is not None and B is not None) else (A if B is None else ZERO - B)
    keep = legal & ~(absent | s["degenerate"])[:, None]
    return np.where(keep, g, ZERO).astype(F32)


# ---------------------------------------------------------------------------------------------------------------------
# the header's pseudo-code, row by row
# ---------------------------------------------------------------------------------------------------------------------
def _row(l, mask):
    """Steps 2-6 of CCX_SAMPLE for one row, as tests/_sample_spec.sample_scalar writes them."""
    m = ((0x1F if mask is None else int(mask)) & 0x1F) | 0x10
    ks = [k for k in range(5) if m >> k & 1]
    lk = {k: F32(l[k]) for k in ks}
    mx = NEG_INF
    for k in ks:
        if lk[k] > mx:
            mx = lk[k]
    degenerate = any(np.isnan(lk[k]) or lk[k] == POS_INF for k in ks) or mx == NEG_INF
    d = {k: (ZERO if degenerate else F32(lk[k] - mx)) for k in ks}
    w = [ZERO] * 5
    for k in ks:
        w[k] = ZERO if d[k] < D_MIN else F32(exp_spec(d[k]))
    c = [w[0]]
    for k in range(1, 5):
        c.append(F32(c[k - 1] + w[k]))
    S = c[4]
    ls = F32(log_spec(S))
    T = None
    for k in range(5):
        term = ZERO if w[k] == ZERO else F32(w[k] * d[k])
        T = term if T is None else F32(T + term)
    H = F32(ls - F32(T / S))
    return ks, degenerate, d, w, S, ls, H


def evaluate_scalar(logits, actions, masks=None):
    logits = np.asarray(logits, F32)
    M = len(logits)
    logp, entropy = np.full(M, np.nan, F32), np.full(M, np.nan, F32)
    with np.errstate(all="ignore"):
        for i in range(M):
            a = int(actions[i])
            if a == ACTION_ABSENT:
                logp[i], entropy[i] = ZERO, ZERO
                continue
            ks, _, d, _, _, ls, H = _row(logits[i], None if masks is None else masks[i])
            entropy[i] = H
            logp[i] = F32(d[a] - ls) if a in ks else NEG_INF
    return logp, entropy


def evaluate_backward_scalar(logits, actions, masks, grad_logp, grad_entropy):
    logits = np.asarray(logits, F32)
    M = len(logits)
    grad = np.full((M, 5), np.nan, F32)
    with np.errstate(all="ignore"):
        for i in range(M):
            a = int(actions[i])
            grad[i] = ZERO                                                   # illegal k, absent and degenerate rows
            if a == ACTION_ABSENT:
                continue
            ks, degenerate, d, w, S, ls, H = _row(logits[i], None if masks is None else masks[i])
            if degenerate:
                continue
            for k in ks:
                p = F32(w[k] / S)
                lp = F32(d[k] - ls)
                A = B = None
                if grad_logp is not None:
                    t1 = F32((ONE if k == a else ZERO) - p)
                    A = F32(F32(grad_logp[i]) * t1) if a in ks else ZERO
                if grad_entropy is not None:
                    t2 = ZERO if w[k] == ZERO else F32(p * F32(lp + H))
                    B = F32(F32(grad_entropy[i]) * t2)
                grad[i, k] = F32(A - B) if (A is not None and B is not None) else (A if B is None else F32(ZERO - B))
    return grad


# ---------------------------------------------------------------------------------------------------------------------
# adversarial cases
# ---------------------------------------------------------------------------------------------------------------------
def make_evaluate_case(E: int, N: int, seed: int = 0) -> dict:
    """make_sample_case(E, N) flattened to M = E N rows, with stored actions and incoming gradients.

    Stored actions: 255 at the case's dead slots; elsewhere about 70 % the action sample_spec draws under the masks, 10 %
    uniform over the legal set, 10 % uniform over 0..4 (may be illegal), 5 % 255, 5 % junk in 5..254.  ``actions_nomask`` is
    the same with the unmasked rule's draws (for calls without masks).  ``sampled`` / ``sampled_nomask`` mark the rows
    that hold the sampler's action, ``spec`` / ``spec_nomask`` the sampler's (actions, logp, entropy) on all rows.
    Gradients: N(0, 1) with some exact zeros; grad_logp also +-inf / NaN at a few absent rows and rows whose stored action is
    out of range or illegal, grad_entropy at a few absent rows (the places the rule selects away)."""
    case = make_sample_case(E, N, seed=seed)
    rng = np.random.default_rng(seed + 1_000_003)
    M = E * N
    out = dict(M=M, logits=case["logits"].reshape(M, 5), logits_masked=case["logits_masked"].reshape(M, 5),
               masks=case["masks"].reshape(M), classes=case["classes"].reshape(M))
    dead = ((case["terminated"] | case["truncated"]) != 0).reshape(M)
    kind = rng.choice(5, size=M, p=[0.70, 0.10, 0.10, 0.05, 0.05])
    for tag, masked in (("", True), ("_nomask", False)):
        spec = sample_spec(case["logits_masked"] if masked else case["logits"], case["masks"] if masked else None,
                           case["terminated"], case["truncated"], case["step_count"], case["episode"], env_offset=3, seed=seed + 17)
        spec = tuple(x.reshape(M) for x in spec)
        m = ((out["masks"] if masked else np.full(M, 0x1F, np.uint8)) & 0x1F) | 0x10
        legal = ((m[:, None] >> np.arange(5, dtype=np.uint8)) & 1).astype(bool)
        pick = (rng.random(M)[:, None] * legal.sum(-1, keepdims=True)).astype(np.int64)         # the pick-th legal action
        among_legal = (np.cumsum(legal, -1) > pick).argmax(-1)
        acts = np.select([kind == 0, kind == 1, kind == 2, kind == 3],
                         [spec[0], among_legal, rng.integers(0, 5, size=M), ACTION_ABSENT], rng.integers(5, 255, size=M))
        acts = np.where(dead, ACTION_ABSENT, acts).astype(np.uint8)
        out["actions" + tag] = acts
        out["sampled" + tag] = (kind == 0) & ~dead
        out["spec" + tag] = spec
        absent = acts == ACTION_ABSENT
        a_ok = (acts <= 4) & np.take_along_axis(legal, np.minimum(acts, 4).astype(np.int64)[:, None], -1)[:, 0]
        glp = rng.standard_normal(M).astype(F32)
        gent = rng.standard_normal(M).astype(F32)
        glp[rng.random(M) < 0.05] = ZERO
        gent[rng.random(M) < 0.05] = ZERO
        junk = np.array([np.inf, -np.inf, np.nan], F32)
        poison = rng.random(M) < 0.3
        glp = np.where((absent | ~a_ok) & poison, junk[rng.integers(0, 3, size=M)], glp).astype(F32)
        gent = np.where(absent & poison, junk[rng.integers(0, 3, size=M)], gent).astype(F32)
        out["grad_logp" + tag], out["grad_entropy" + tag] = glp, gent
    return out


def case_args(case, masked: bool):
    """(logits, actions, masks, grad_logp, grad_entropy) of a generator case for a call with or without masks."""
    tag = "" if masked else "_nomask"
    return (case["logits_masked"] if masked else case["logits"], case["actions" + tag], case["masks"] if masked else None,
            case["grad_logp" + tag], case["grad_entropy" + tag])
