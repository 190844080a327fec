"""CCX_C51 as include/ccx.h states it, restated in NumPy on the CPU, plus generators of cases.  TEST INFRASTRUCTURE ONLY: what
the kernels of csrc/ccx_c51.hip and the host build of csrc/ccx_c51.h are compared with.

Written from the header paragraph.  ``exp_spec`` / ``log_spec`` are tests/_sample_spec.py's, the butterfly (``_halve``, run
here on f32 arrays of 64 places) and the f64 tree are tests/_ppo_loss_spec.py's, ``greedy_spec`` / ``legal_bits`` / the final
values are tests/_qlearn_spec.py's (imported, so the rules cannot drift apart); everything else is elementwise ``np.float32``
operations (one rounding each), selects by ``np.where``, never a multiplication by zero.  Every comparison against this
module is on bit patterns."""

from __future__ import annotations

import numpy as np
from _ppo_loss_spec import _halve, tree_sum
from _qlearn_spec import greedy_spec, legal_bits, td_finals, valid_ok
from _sample_spec import ACTION_ABSENT, D_MIN, F32, exp_spec, log_spec

F64 = np.float64
ZERO, ONE = F32(0.0), F32(1.0)
NEG_INF = F32(-np.inf)
_J = np.arange(64)
PLACE = _J.astype(F32)
ATOMS = (2, 3, 33, 51, 64, 8)             # 8 LAST: the atom count of the chain (tests/_c51_chain.py); the others keep their variants

# Accuracy against torch f64, measured on the CPU by tests/test_c51_spec.py (the maxima it prints) and DOUBLED, as
# max |err| / max(1, |f64 value|) against the textbook composition on the same f32 inputs, A in ATOMS, logits ~ N(0, 2^2),
# support [-10, 10].  Measured: proj 6.21e-6, loss 5.27e-8, row_loss 7.58e-6, q_values 1.04e-6, n * grad_logits 7.52e-6 (the first, third and
# last are ulp(b) at b near A - 1, a property of f32 positions on the support, times |log p|).  The
# header paragraph, the README and DESIGN.md quote the same numbers.
C51_PROJ_BOUND = 1.3e-5
C51_LOSS_BOUND = 1.1e-7
C51_ROW_LOSS_BOUND = 1.6e-5
C51_Q_BOUND = 2.1e-6
C51_GRAD_BOUND = 1.6e-5                # n * grad_logits
EXCLUDED_CAP = 0.005                   # rows whose two best legal expected next-values lie within 1e-4


def support(A, vmin, vmax):
    """(dz, z f32 [64], top)."""
    vmin, vmax = F32(vmin), F32(vmax)
    span = F32(vmax - vmin)
    dz = F32(span / F32(A - 1))
    z = (vmin + (PLACE * dz).astype(F32)).astype(F32)
    return dz, z, F32(A - 1)


def max2(a, b):
    m = np.fmax(a, b)
    return np.where(m == ZERO, ZERO, m).astype(F32)


def _max64(v):
    for o in (32, 16, 8, 4, 2, 1):
        v = max2(v, v[..., _J ^ o])
    return v[..., 0]


def dist(l, A):
    """l f32 [..., A] -> (d [..., 64], e [..., 64], S [...]): step 1."""
    l = np.asarray(l, F32)
    live = _J < A
    v = np.full(l.shape[:-1] + (64,), NEG_INF, F32)
    v[..., :A] = l
    with np.errstate(all="ignore"):
        mx = _max64(v)
        d = (v - mx[..., None]).astype(F32)
        u = (d - d).astype(F32)
        inn = d >= D_MIN
        ex = exp_spec(np.where(inn, d, ZERO).astype(F32))
        e = np.where(live, np.where(inn, ex, u), ZERO).astype(F32)
        S = _halve(e)
    return d, e, S.astype(F32)


def log_sum(S):
    nan = np.isnan(S)
    return np.where(nan, S, log_spec(np.where(nan, ONE, S).astype(F32))).astype(F32)


def expected(e, S, z, A):
    """Step 2: butterfly(e_j * z_j) / S."""
    with np.errstate(all="ignore"):
        T = _halve(np.where(_J < A, (e * z).astype(F32), ZERO).astype(F32))
        return (T / S).astype(F32)


def q_values_spec(logits, vmin=-10.0, vmax=10.0):
    """f32 [..., 5] from f32 [..., 5, A]."""
    logits = np.asarray(logits, F32)
    A = logits.shape[-1]
    _dz, z, _top = support(A, vmin, vmax)
    _d, e, S = dist(logits, A)
    return expected(e, S, z, A)


def c51_rows(logits, actions, reward, done, next_target, next_online=None, masks_next=None, valid=None, weights=None, gamma=0.99,
             discount=None, vmin=-10.0, vmax=10.0):
    """Steps 1-6 for every row (what rows that do not count hold is junk; ``counts`` says which do)."""
    logits = np.asarray(logits, F32)
    A = logits.shape[-1]
    logits = logits.reshape(-1, 5, A)
    M = logits.shape[0]
    live = _J < A
    dz, z, top = support(A, vmin, vmax)
    vmin = F32(vmin)
    a = np.asarray(actions, np.uint8).reshape(M).astype(np.int64)
    ok = valid_ok(valid, M)
    counts = ok & (a <= 4)
    bad = ok & (a > 4) & (a != ACTION_ABSENT)
    nt = np.asarray(next_target, F32).reshape(M, 5, A)
    sel = nt if next_online is None else np.asarray(next_online, F32).reshape(M, 5, A)
    rows = np.arange(M)
    with np.errstate(all="ignore"):
        _ds, es, Ss = dist(sel, A)
        qsel = expected(es, Ss, z, A)
        kstar = greedy_spec(qsel, legal_bits(masks_next, (M,)))
        _dp, ep, Sp = dist(nt[rows, kstar], A)
        r = np.asarray(reward, F64).reshape(M).astype(F32)                # one rounding
        disc = np.full(M, F32(gamma), F32) if discount is None else np.asarray(discount, F32).reshape(M)
        cut = (np.asarray(done).reshape(M) != 0) | (disc == ZERO)
        point = np.where(_J == 0, ONE, ZERO).astype(F32)
        p = np.where(cut[:, None], point[None, :], (ep / Sp[:, None]).astype(F32)).astype(F32)
        gz = (disc[:, None] * z[None, :]).astype(F32)
        tz = (r[:, None] + gz).astype(F32)
        t = np.where(cut[:, None], r[:, None], tz).astype(F32)
        u = (t - t).astype(F32)
        tv = (t - vmin).astype(F32)
        b0 = (tv / dz).astype(F32)
        b1 = np.where(b0 < ZERO, u, b0).astype(F32)
        tu = (top + u).astype(F32)
        b = np.where(b1 > top, tu, b1).astype(F32)
        m = np.zeros((M, 64), F32)
        for j in range(A):
            aa = (b[:, j, None] - PLACE[None, :]).astype(F32)
            om = (ONE - np.abs(aa)).astype(F32)
            w = np.where(om < ZERO, ZERO, om).astype(F32)
            m = (m + (p[:, j, None] * w).astype(F32)).astype(F32)
        d, e, S = dist(logits[rows, np.minimum(a, 4)], A)
        lS = log_sum(S)
        logp = (d - lS[:, None]).astype(F32)
        prod = (m * logp).astype(F32)
        c = np.where(live, np.where(m != ZERO, prod, ZERO), ZERO).astype(F32)
        ce = (ZERO - _halve(c)).astype(F32)
        term = ce if weights is None else (np.asarray(weights, F32).reshape(M) * ce).astype(F32)
        qa = expected(e, S, z, A)
        y = _halve(np.where(live, (m * z).astype(F32), ZERO).astype(F32)).astype(F32)
    return dict(M=M, A=A, a=a, counts=counts, bad=bad, kstar=kstar, cut=cut, p=p, b=b, m=m, d=d, e=e, S=S, ce=ce, term=term, qa=qa,
                y=y, qsel=qsel)


def c51_loss_spec(logits, actions, reward, done, next_target, next_online=None, masks_next=None, valid=None, weights=None,
                  gamma=0.99, discount=None, vmin=-10.0, vmax=10.0, details=False):
    """(stats f32 [8], row_loss f32 [M], proj f32 [M, A])."""
    t = c51_rows(logits, actions, reward, done, next_target, next_online, masks_next, valid, weights, gamma, discount, vmin, vmax)
    c, zero = t["counts"], F64(0.0)
    S = [tree_sum(np.where(c, F64(1.0), zero))]
    for name in ("term", "ce", "qa", "y"):
        S.append(tree_sum(np.where(c, t[name].astype(F64), zero)))
    S.append(tree_sum(np.where(t["bad"], F64(1.0), zero)))
    stats = td_finals(S)
    row_loss = np.where(c, t["ce"], ZERO).astype(F32)
    proj = np.where(c[:, None], t["m"][:, :t["A"]], ZERO).astype(F32)
    return (stats, row_loss, proj, t) if details else (stats, row_loss, proj)


def c51_loss_backward_spec(logits, actions, proj, valid=None, weights=None, stats=None, grad_loss=None):
    """grad_logits f32 [M, 5, A]."""
    logits = np.asarray(logits, F32)
    A = logits.shape[-1]
    logits = logits.reshape(-1, 5, A)
    M = logits.shape[0]
    a = np.asarray(actions, np.uint8).reshape(M).astype(np.int64)
    n = F32(stats[6])
    counts = valid_ok(valid, M) & (a <= 4) & bool(n != 0)
    g = ONE if grad_loss is None else F32(grad_loss)
    m = np.zeros((M, 64), F32)
    m[:, :A] = np.asarray(proj, F32).reshape(M, A)
    with np.errstate(all="ignore"):
        sc = F32(g / n)
        gw = np.full(M, sc, F32) if weights is None else (sc * np.asarray(weights, F32).reshape(M)).astype(F32)
        _d, e, S = dist(logits[np.arange(M), np.minimum(a, 4)], A)
        Msum = _halve(np.where(_J < A, m, ZERO).astype(F32)).astype(F32)
        pm = ((e / S[:, None]).astype(F32) * Msum[:, None]).astype(F32)
        ga = (gw[:, None] * (pm - m).astype(F32)).astype(F32)[:, :A]
    hit = counts[:, None] & (np.arange(5)[None, :] == a[:, None])
    return np.where(hit[:, :, None], ga[:, None, :], ZERO).astype(F32)


# ---------------------------------------------------------------------------------------------------------------------
# cases
# ---------------------------------------------------------------------------------------------------------------------
def make_c51_case(M: int, A: int, seed: int = 0, density: float = 0.75, special: bool = True) -> dict:
    """Everything a loss call reads, for calls with or without each optional input (``c51_args``).

    actions      0..4; 5 % 255 (absent), 3 % junk in 5..254
    valid        not zero (1, 2 or 255) with probability ``density``
    done         20 % (1, 4 or 255); half of the done rows hold NaN throughout their next-state logits
    logits       N(0, 2^2); with ``special``: a tenth of the rows hold an atom at -200 (d < -80: weight exactly +0.0), a few hold
                 +-0.0 and subnormals, and NaN / +-inf sit at actions other than the taken one in a tenth of the rows
    next_*       N(0, 2^2); with ``special``: ties between two actions' rows (equal expected values), NaN rows in the online
                 array (a NaN expected value never wins), NaN at every illegal action in the ``_masked`` arrays
    masks_next   bits 0-3 random, bit 4 mostly set, junk in bits 5-7
    reward       f64 N(0, 3): not f32 values, so the one rounding shows; 5 % beyond either end of the support
    weights      U(0.5, 1.5), exactly 0 at 5 %;  discount  0.99^k for k in 1..3, exactly 0 at 5 %
    Rows that never count (action 255 or junk) hold NaN in every float input; rows whose valid byte is 0 do so in the
    ``*_poisoned`` arrays, which calls with ``valid`` use."""
    rng = np.random.default_rng(seed + 51_000_017 * A)
    a = rng.integers(0, 5, size=M).astype(np.uint8)
    u = rng.random(M)
    a[u < 0.05] = ACTION_ABSENT
    junk = (u >= 0.05) & (u < 0.08)
    a[junk] = rng.choice(np.array([5, 7, 100, 254], np.uint8), size=int(junk.sum()))
    valid = (rng.random(M) < density).astype(np.uint8)
    valid[valid != 0] = rng.choice(np.array([1, 1, 1, 2, 255], np.uint8), size=int((valid != 0).sum()))
    done = (rng.random(M) < 0.2).astype(np.uint8)
    done[done != 0] = rng.choice(np.array([1, 1, 4, 255], np.uint8), size=int((done != 0).sum()))
    lg = (rng.standard_normal((M, 5, A)) * 2.0).astype(F32)
    nt = (rng.standard_normal((M, 5, A)) * 2.0).astype(F32)
    no = (rng.standard_normal((M, 5, A)) * 2.0).astype(F32)
    low = rng.integers(0, 16, size=M).astype(np.uint8)
    masks = low | np.where(rng.random(M) < 0.85, 0x10, 0).astype(np.uint8) | (rng.integers(0, 8, size=M).astype(np.uint8) << 5)
    legal = legal_bits(masks, (M,))
    reward = rng.standard_normal(M) * 3.0
    far = rng.random(M) < 0.05
    reward[far] = rng.choice(np.array([-37.5, 25.0, 1e30, -1e30]), size=int(far.sum()))
    weights = rng.uniform(0.5, 1.5, M).astype(F32)
    weights[rng.random(M) < 0.05] = ZERO
    discount = (F32(0.99) ** rng.integers(1, 4, size=M)).astype(F32)
    discount[rng.random(M) < 0.05] = ZERO
    if special:
        rows = np.flatnonzero(rng.random(M) < 0.1)
        lg[rows, :, rng.integers(0, A, size=len(rows))] = F32(-200.0)
        nt[rows, :, rng.integers(0, A, size=len(rows))] = F32(-200.0)
        rows = np.flatnonzero(rng.random(M) < 0.05)
        lg[rows, :, 0] = rng.choice(np.array([0.0, -0.0, 1e-40, -1e-42], F32), size=len(rows))[:, None]
        spoil = np.flatnonzero((rng.random(M) < 0.1) & (a <= 4))
        k = (a[spoil] + rng.integers(1, 5, size=len(spoil))) % 5
        lg[spoil, k, rng.integers(0, A, size=len(spoil))] = rng.choice(np.array([np.nan, np.inf, -np.inf], F32), size=len(spoil))
        tie = np.flatnonzero(rng.random(M) < 0.1)
        no[tie, 3], nt[tie, 2] = no[tie, 1], nt[tie, 0]
        rows = np.flatnonzero(rng.random(M) < 0.2)
        no[rows, rng.integers(0, 4, size=len(rows)), 0] = F32(np.nan)
    wipe = (done != 0) & (rng.random(M) < 0.5)
    nt[wipe], no[wipe] = np.nan, np.nan
    nt_m = np.where(legal[:, :, None], nt, F32(np.nan)).astype(F32)
    no_m = np.where(legal[:, :, None], no, F32(np.nan)).astype(F32)
    out = dict(M=M, A=A, actions=a, valid=valid, done=done, masks=masks)
    never = a > 4
    for poisoned in (False, True):
        gone = never | ((valid == 0) & poisoned)
        tag = "_poisoned" if poisoned else ""
        for name, arr in (("logits", lg), ("nt", nt), ("no", no), ("nt_masked", nt_m), ("no_masked", no_m)):
            out[name + tag] = np.where(gone[:, None, None], F32(np.nan), arr).astype(F32)
        out["reward" + tag] = np.where(gone, np.nan, reward)
        out["weights" + tag] = np.where(gone, F32(np.nan), weights).astype(F32)
        out["discount" + tag] = np.where(gone, F32(np.nan), discount).astype(F32)
    return out


def c51_args(case, masked=True, double=True, with_valid=True, with_weights=True, with_discount=False, M=None) -> dict:
    """Keyword arguments (logits ... discount) of a generator case for one NULL combination of the optional inputs."""
    M = case["M"] if M is None else M
    tag = "_poisoned" if with_valid else ""
    mk = "_masked" if masked else ""
    kw = dict(logits=case["logits" + tag], actions=case["actions"], reward=case["reward" + tag], done=case["done"],
              next_target=case["nt" + mk + tag], next_online=case["no" + mk + tag] if double else None,
              masks_next=case["masks"] if masked else None, valid=case["valid"] if with_valid else None,
              weights=case["weights" + tag] if with_weights else None, discount=case["discount" + tag] if with_discount else None)
    return {k: (None if v is None else np.ascontiguousarray(v[:M])) for k, v in kw.items()}


C51_VARIANTS = [(True, True, True, True, False), (False, False, False, False, False), (True, False, True, False, True),
                (False, True, False, True, True), (True, True, False, False, True), (False, False, True, True, False)]
