"""CCX_PPO_LOSS as include/ccx.h states it, restated in NumPy on the CPU, plus a generator of adversarial cases.  TEST
INFRASTRUCTURE ONLY: what the loss kernels are compared with.

Built on tests/_evaluate_spec.py: step 1 (logp, H) is ``evaluate_spec`` itself and the logits gradient is
``evaluate_backward_spec`` itself, so the rules cannot drift apart; everything else is written from the CCX_PPO_LOSS paragraph
with elementwise ``np.float32`` operations (one rounding each), ``np.float64`` ones in the tree and the final values, selects
by ``np.where``, never a multiplication by zero.  ``ppo_loss_scalar`` / ``tree_sum_loop`` are the header's text one row and
one addition at a time.  Every comparison against this module is on bit patterns."""

from __future__ import annotations

import numpy as np
from _evaluate_spec import (evaluate_backward_scalar, evaluate_backward_spec, evaluate_scalar, evaluate_spec,
                            make_evaluate_case)
from _sample_spec import ACTION_ABSENT, F32, exp_spec

F64 = np.float64
X_MAX = F32(80.0)
ONE = F32(1.0)
ZERO = F32(0.0)

# Accuracy against f64, measured on the CPU by tests/test_ppo_loss_spec.py (the maxima it prints) and DOUBLED, as
# max |err| / max(1, |f64 value|) against the textbook composition in torch f64 on the same f32 inputs.  Measured:
# exp_spec on [-80, 80] 1.01e-7 relative; loss 4.91e-8, policy 1.05e-8, value 3.33e-8, entropy 2.47e-8, approx_kl 1.20e-8;
# n * grad_logits 3.05e-5 over all compared rows and 1.10e-6 over those with logp >= -10 (a stored action far down the tail
# has a logp of size 80 and more, whose rounding, 3.8e-6 absolute and up, the ratio exp(logp - logp_old) turns into a
# relative error of the row's gradient; the means average it away); n * grad_values 1.26e-7; mean 1.79e-8, std 4.13e-8.
# The header paragraph and DESIGN.md quote the same numbers.
EXP_REL_BOUND_80 = 2.1e-7
PPO_STAT_BOUNDS = dict(loss=9.9e-8, policy=2.2e-8, value=6.7e-8, entropy=5.0e-8, approx_kl=2.4e-8)
PPO_GRAD_LOGITS_BOUND = 6.1e-5         # n * grad_logits, all compared rows
PPO_GRAD_LOGITS_NEAR_BOUND = 2.2e-6    # n * grad_logits, rows with logp >= -10
PPO_GRAD_VALUES_BOUND = 2.6e-7         # n * grad_values
MOMENTS_MEAN_BOUND = 3.6e-8
MOMENTS_STD_BOUND = 8.3e-8
EXCLUDED_CAP = 0.10                    # of the counted rows


# ---------------------------------------------------------------------------------------------------------------------
# the tree
# ---------------------------------------------------------------------------------------------------------------------
_J = np.arange(64)


def _halve(s):
    """s f64 [..., 64]: for o = 32 .. 1, every place j takes s[j] + s[j ^ o]; returns place 0."""
    for o in (32, 16, 8, 4, 2, 1):
        s = s + s[..., _J ^ o]
    return s[..., 0]


def block_partials(terms):
    """f64 [B]: the partial of every block of 256 consecutive rows; rows >= M enter as +0.0."""
    terms = np.asarray(terms, F64)
    M = terms.shape[0]
    B = -(-M // 256)
    pad = np.zeros(B * 256, F64)
    pad[:M] = terms
    G = _halve(pad.reshape(B, 4, 64))
    return ((G[:, 0] + G[:, 1]) + G[:, 2]) + G[:, 3]


def final_sum(P):
    """Place j adds P[j], P[j + 64], ... in ascending order onto +0.0 (a missing one adds nothing: x + +0.0 is x for every x
    an accumulator that starts at +0.0 can hold), then the 64 places are halved."""
    P = np.asarray(P, F64)
    rounds = -(-P.shape[0] // 64)
    pad = np.zeros(rounds * 64, F64)
    pad[:P.shape[0]] = P
    acc = np.zeros(64, F64)
    for r in range(rounds):
        acc = acc + pad[r * 64:(r + 1) * 64]
    return F64(_halve(acc))


def tree_sum(terms):
    return final_sum(block_partials(terms))


def tree_sum_loop(terms):
    """The same tree, one addition at a time, from the header's sentences."""
    terms = [float(t) for t in np.asarray(terms, F64)]
    M = len(terms)
    B = -(-M // 256)

    def halve(s):
        s = list(s)
        for o in (32, 16, 8, 4, 2, 1):
            s = [F64(s[j]) + F64(s[j ^ o]) for j in range(64)]
        return s[0]

    P = []
    for b in range(B):
        G = []
        for g in range(4):
            base = b * 256 + g * 64
            G.append(halve([F64(terms[i]) if i < M else F64(0.0) for i in range(base, base + 64)]))
        P.append(((G[0] + G[1]) + G[2]) + G[3])
    acc = []
    for j in range(64):
        a = F64(0.0)
        for i in range(j, B, 64):
            a = a + P[i]
        acc.append(a)
    return F64(halve(acc))


# ---------------------------------------------------------------------------------------------------------------------
# the rule, every row at once
# ---------------------------------------------------------------------------------------------------------------------
def _hyper(clip, vf_coef, ent_coef, adv_eps):
    clip = F32(clip)
    return ONE - clip, ONE + clip, F32(vf_coef), F32(ent_coef), F32(adv_eps)


def counted(actions, valid):
    c = np.asarray(actions, np.uint8) != ACTION_ABSENT
    return c if valid is None else c & (np.asarray(valid) != 0)


def row_terms(logits, values, actions, logp_old, advantages, returns, masks=None, valid=None, norm=None, clip=0.2,
              adv_eps=1e-8):
    """Steps 1-6 for every row (what rows that do not count hold is junk; ``counts`` says which do)."""
    lo, hi, _, _, eps = _hyper(clip, 0, 0, adv_eps)
    counts = counted(actions, valid)
    logp, H = evaluate_spec(logits, actions, masks)
    adv = np.asarray(advantages, F32)
    with np.errstate(all="ignore"):
        x = (logp - np.asarray(logp_old, F32)).astype(F32)
        xc = np.where(x < -X_MAX, -X_MAX, np.where(x > X_MAX, X_MAX, x)).astype(F32)
        isnan = np.isnan(xc)
        e = exp_spec(np.where(isnan | ~counts, ZERO, xc).astype(F32))
        ratio = np.where(isnan, xc, e).astype(F32)
        if norm is None:
            an = adv
        else:
            den = F32(norm[1]) + eps
            an = ((adv - F32(norm[0])).astype(F32) / den).astype(F32)
        s1 = (ratio * an).astype(F32)
        rc = np.where(ratio < lo, lo, np.where(ratio > hi, hi, ratio)).astype(F32)
        s2 = (rc * an).astype(F32)
        surr = np.where(s2 < s1, s2, s1).astype(F32)
        ve = (np.asarray(values, F32) - np.asarray(returns, F32)).astype(F32)
        vl = (ve * ve).astype(F32)
        kl = ((ratio - ONE).astype(F32) - xc).astype(F32)
        clipped = (ratio < lo) | (ratio > hi)
        cf = np.where(clipped, ONE, ZERO).astype(F32)
    return dict(counts=counts, logp=logp, H=H, x=x, xc=xc, ratio=ratio, an=an, s1=s1, s2=s2, surr=surr, ve=ve, vl=vl, kl=kl,
                cf=cf, clipped=clipped)


def loss_finals(S, vf_coef, ent_coef):
    """stats f32 [8] from the six f64 sums."""
    n = F64(S[0])
    if n == 0:
        return np.zeros(8, F32)
    with np.errstate(all="ignore"):
        policy = -(F64(S[1]) / n)
        value = F64(S[2]) / n
        entropy = F64(S[3]) / n
        loss = (policy + F64(F32(vf_coef)) * value) - F64(F32(ent_coef)) * entropy
        return np.array([loss, policy, value, entropy, F64(S[4]) / n, F64(S[5]) / n, n, 0.0], F64).astype(F32)


def ppo_loss_spec(logits, values, actions, logp_old, advantages, returns, masks=None, valid=None, norm=None, clip=0.2,
                  vf_coef=0.5, ent_coef=0.01, adv_eps=1e-8, details=False):
    """stats f32 [8]."""
    t = row_terms(logits, values, actions, logp_old, advantages, returns, masks, valid, norm, clip, adv_eps)
    c = t["counts"]
    zero = F64(0.0)
    S = [tree_sum(np.where(c, F64(1.0), zero))]
    for name in ("surr", "vl", "H", "kl", "cf"):
        S.append(tree_sum(np.where(c, t[name].astype(F64), zero)))
    stats = loss_finals(S, vf_coef, ent_coef)
    return (stats, t, S) if details else stats


def ppo_loss_backward_spec(logits, values, actions, logp_old, advantages, returns, masks=None, valid=None, norm=None, clip=0.2,
                           vf_coef=0.5, ent_coef=0.01, adv_eps=1e-8, stats=None, grad_loss=None, want_logits=True,
                           want_values=True):
    """(grad_logits f32 [M, 5] or None, grad_values f32 [M] or None)."""
    _, _, vf, ent, _ = _hyper(clip, vf_coef, ent_coef, adv_eps)
    t = row_terms(logits, values, actions, logp_old, advantages, returns, masks, valid, norm, clip, adv_eps)
    M = t["counts"].shape[0]
    n = F32(stats[6])
    g = ONE if grad_loss is None else F32(grad_loss)
    with np.errstate(all="ignore"):
        sc = F32(g / n)
        counts = t["counts"] & bool(n != 0)
        gl = gv = None
        if want_logits:
            gent = F32(ZERO - F32(sc * ent))
            passes = ~t["clipped"] | (t["s1"] < t["s2"])
            prod = (sc * t["s1"]).astype(F32)
            glp = np.where(passes & (t["x"] == t["xc"]), (ZERO - prod).astype(F32), ZERO).astype(F32)
            rows = evaluate_backward_spec(logits, actions, masks, glp, np.full(M, gent, F32))
            gl = np.where(counts[:, None], rows, ZERO).astype(F32)
        if want_values:
            scv = F32(sc * vf)
            gv = np.where(counts, (scv * (t["ve"] + t["ve"]).astype(F32)).astype(F32), ZERO).astype(F32)
    return gl, gv


def masked_moments_spec(x, valid=None):
    """out f32 [4] = {n, mean, std, 0}."""
    x = np.asarray(x, F32).reshape(-1)
    c = np.ones(x.shape, bool) if valid is None else np.asarray(valid).reshape(-1) != 0
    zero = F64(0.0)
    xd = x.astype(F64)
    with np.errstate(all="ignore"):
        n = tree_sum(np.where(c, F64(1.0), zero))
        sx = tree_sum(np.where(c, xd, zero))
        sxx = tree_sum(np.where(c, xd * xd, zero))
        if n < 2:
            return np.array([n, 0.0, 1.0, 0.0], F32)
        mean = sx / n
        q = (sxx - sx * mean) / (n - F64(1.0))
        var = F64(0.0) if q < 0 else q
        return np.array([n, mean, np.sqrt(var), 0.0], F64).astype(F32)


# ---------------------------------------------------------------------------------------------------------------------
# the header's text, row by row
# ---------------------------------------------------------------------------------------------------------------------
def ppo_loss_scalar(logits, values, actions, logp_old, advantages, returns, masks=None, valid=None, norm=None, clip=0.2,
                    vf_coef=0.5, ent_coef=0.01, adv_eps=1e-8, grad_loss=None):
    """(stats, grad_logits, grad_values) with Python loops and np.float32 / np.float64 scalars."""
    M = len(actions)
    clip, vf, ent, eps = F32(clip), F32(vf_coef), F32(ent_coef), F32(adv_eps)
    lo, hi = F32(ONE - clip), F32(ONE + clip)
    logp, H = evaluate_scalar(logits, actions, masks)
    terms = [[F64(0.0)] * M for _ in range(6)]
    keep = {}
    with np.errstate(all="ignore"):
        den = None if norm is None else F32(F32(norm[1]) + eps)
        for i in range(M):
            if int(actions[i]) == ACTION_ABSENT or (valid is not None and int(valid[i]) == 0):
                continue
            x = F32(logp[i] - F32(logp_old[i]))
            xc = -X_MAX if x < -X_MAX else (X_MAX if x > X_MAX else x)
            ratio = xc if np.isnan(xc) else F32(exp_spec(F32(xc)))
            an = F32(advantages[i]) if norm is None else F32(F32(F32(advantages[i]) - F32(norm[0])) / den)
            s1 = F32(ratio * an)
            rc = lo if ratio < lo else (hi if ratio > hi else ratio)
            s2 = F32(rc * an)
            surr = s2 if s2 < s1 else s1
            ve = F32(F32(values[i]) - F32(returns[i]))
            vl = F32(ve * ve)
            kl = F32(F32(ratio - ONE) - xc)
            clipped = bool(ratio < lo or ratio > hi)
            for q, v in enumerate((ONE, surr, vl, H[i], kl, ONE if clipped else ZERO)):
                terms[q][i] = F64(v)
            keep[i] = (x, xc, s1, s2, ve, clipped)
        S = [tree_sum_loop(t) for t in terms]
        stats = loss_finals(S, vf, ent)
        gl, gv = np.zeros((M, 5), F32), np.zeros(M, F32)
        n = stats[6]
        if n != 0:
            g = ONE if grad_loss is None else F32(grad_loss)
            sc = F32(g / n)
            gent = F32(ZERO - F32(sc * ent))
            scv = F32(sc * vf)
            glp = np.zeros(M, F32)
            for i, (x, xc, s1, s2, ve, clipped) in keep.items():
                passes = (not clipped) or bool(s1 < s2)
                glp[i] = F32(ZERO - F32(sc * s1)) if (passes and x == xc) else ZERO
                gv[i] = F32(scv * F32(ve + ve))
            rows = evaluate_backward_scalar(logits, actions, masks, glp, np.full(M, gent, F32))
            for i in keep:
                gl[i] = rows[i]
    return stats, gl, gv


# ---------------------------------------------------------------------------------------------------------------------
# adversarial cases
# ---------------------------------------------------------------------------------------------------------------------
def make_ppo_case(M: int, seed: int = 0, density: float = 0.7) -> dict:
    """make_evaluate_case(M, 1) with everything a loss call reads.  Per call variant (tag "" with masks, "_nomask" without):

    actions      the evaluate generator's (sampler's draw, legal, possibly illegal, 255, junk 5..254; 255 at dead slots); of the
                 rows whose logp under them is -inf, 70 % take the sampler's draw instead, and three quarters of the rows of
                 class ``degenerate`` get plain logits, so that the rows an f64 comparison must leave out stay under a tenth
    logp_old     relative to the row's own logp: 25 % equal (ratio exactly 1), 35 % within +-0.15 (inside the clip range of
                 0.2), 38.5 % 0.25 .. 2 away on either side (outside it), 1.5 % +-100 away (|x| > 80); N(0, 1) where logp is -inf
    advantages   N(0, 1), both signs, some exact zeros;  returns, values  N(0, 2)
    valid        1 with probability ``density`` (0: all zero, 1: all one)
    Rows that do not count (valid = 0 or action 255) carry NaN / +-inf in every float input at about a third of them, and
    NaN logits wherever the evaluate generator puts them (illegal places, dead rows)."""
    case = make_evaluate_case(M, 1, seed=seed)
    rng = np.random.default_rng(seed + 2_000_003)
    plain = (rng.standard_normal((M, 5)) * 3.0).astype(F32)
    swap = (case["classes"] == 7) & (rng.random(M) < 0.75) & ~np.isnan(case["logits"]).all(-1)
    legal = ((((case["masks"] & 0x1F) | 0x10)[:, None] >> np.arange(5, dtype=np.uint8)) & 1).astype(bool)
    out = dict(M=M, masks=case["masks"], classes=case["classes"])
    out["logits"] = np.where(swap[:, None], plain, case["logits"]).astype(F32)
    out["logits_masked"] = np.where(swap[:, None], np.where(legal, plain, F32(np.nan)), case["logits_masked"]).astype(F32)
    valid = (rng.random(M) < density).astype(np.uint8)
    valid[valid != 0] = rng.choice(np.array([1, 1, 1, 2, 255], np.uint8), size=int((valid != 0).sum()))
    out["valid"] = valid
    adv = rng.standard_normal(M).astype(F32)
    adv[rng.random(M) < 0.03] = ZERO
    ret = (rng.standard_normal(M) * 2.0).astype(F32)
    val = (rng.standard_normal(M) * 2.0).astype(F32)
    junk = np.array([np.nan, np.inf, -np.inf], F32)
    for tag, masked in (("", True), ("_nomask", False)):
        logits = out["logits_masked"] if masked else out["logits"]
        masks = case["masks"] if masked else None
        acts = case["actions" + tag].copy()
        logp, _ = evaluate_spec(logits, acts, masks)
        redo = np.isneginf(logp) & (rng.random(M) < 0.7)
        acts = np.where(redo, case["spec" + tag][0], acts).astype(np.uint8)
        logp, _ = evaluate_spec(logits, acts, masks)
        kind = rng.choice(4, size=M, p=[0.25, 0.35, 0.385, 0.015])
        sign = np.where(rng.random(M) < 0.5, -1.0, 1.0)
        delta = np.select([kind == 0, kind == 1, kind == 2], [0.0, rng.uniform(-0.15, 0.15, M), sign * rng.uniform(0.25, 2.0, M)],
                          sign * 100.0)
        with np.errstate(all="ignore"):
            lpo = np.where(np.isfinite(logp), logp.astype(F64) - delta, rng.standard_normal(M)).astype(F32)
        c = counted(acts, valid)
        poison = ~c & (rng.random(M) < 0.35)
        fl = {}
        for name, a in (("logp_old", lpo), ("advantages", adv), ("returns", ret), ("values", val)):
            fl[name] = np.where(poison, junk[rng.integers(0, 3, size=M)], a).astype(F32)
        out["actions" + tag] = acts
        for name, a in fl.items():
            out[name + tag] = a
    return out


def case_args(case, masked: bool, with_valid: bool = True, M: int | None = None):
    """Keyword arguments (logits ... valid) of a generator case for a call with or without masks / valid, its first M rows."""
    tag = "" if masked else "_nomask"
    M = case["M"] if M is None else M
    kw = dict(logits=case["logits_masked"] if masked else case["logits"], values=case["values" + tag], actions=case["actions" + tag],
              logp_old=case["logp_old" + tag], advantages=case["advantages" + tag], returns=case["returns" + tag],
              masks=case["masks"] if masked else None, valid=case["valid"] if with_valid else None)
    return {k: (None if v is None else np.ascontiguousarray(v[:M])) for k, v in kw.items()}


def clean_case(case, masked: bool, M: int | None = None):
    """case_args for a call with valid = None.  The generator poisons the float inputs of rows whose `valid` byte is 0; without
    `valid` those rows count, so they get finite values here.  Rows with action 255 keep their NaN."""
    kw = case_args(case, masked, with_valid=False, M=M)
    rng = np.random.default_rng(5)
    bad = kw["actions"] != ACTION_ABSENT
    for name in ("logp_old", "advantages", "returns", "values"):
        a = kw[name].copy()
        fix = bad & ~np.isfinite(a)
        a[fix] = rng.standard_normal(int(fix.sum())).astype(F32)
        kw[name] = a
    return kw
