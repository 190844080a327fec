"""CCX_QLEARN as include/ccx.h states it, restated in NumPy on the CPU, plus generators of adversarial cases.  TEST
INFRASTRUCTURE ONLY: what the kernels of csrc/ccx_qlearn.hip and the host build of csrc/ccx_qlearn.h are compared with.

Written from the header paragraph.  The word function and ``bits32`` are tests/_sample_spec.py's, the tree is
tests/_ppo_loss_spec.py's (imported, so the rules cannot drift apart); everything else is elementwise ``np.float32``
operations (one rounding each), ``np.float64`` ones in the final values, selects by ``np.where``, never a multiplication by
zero.  Every comparison against this module is on bit patterns."""

from __future__ import annotations

import numpy as np
from _ppo_loss_spec import tree_sum
from _sample_spec import ACTION_ABSENT, F32, K_EPS_STREAM, K_SAMPLE_STREAM, R_SCALE, U32, bits32, make_sample_case, slot_words  # noqa: F401

F64 = np.float64
ZERO, HALF, ONE = F32(0.0), F32(0.5), F32(1.0)
NEG_INF = F32(-np.inf)
K_Q_EXPLORE_STREAM = 0x68E31DA4        # kQExploreStream / kQChoiceStream (csrc/ccx_kernels.h, include/ccx.h CCX_QLEARN)
K_Q_CHOICE_STREAM = 0xB5297A4D
assert len({0, K_EPS_STREAM, K_SAMPLE_STREAM, K_Q_EXPLORE_STREAM, K_Q_CHOICE_STREAM}) == 5

# Accuracy against torch f64, measured on the CPU by tests/test_qlearn_spec.py (the maxima it prints) and DOUBLED, as
# max |err| / max(1, |f64 value|) against the textbook composition on the same f32 inputs.  Measured: loss 5.11e-8, mean |td|
# 4.90e-8, n * grad_q 5.43e-7 (a rounding each of gamma * boot, r + nb, qa - y, g / n, sc * w and gw * dd on values of size up to 10).  The header
# paragraph, the README and DESIGN.md quote the same numbers.
TD_LOSS_BOUND = 1.1e-7
TD_MEAN_ABS_BOUND = 9.9e-8
TD_GRAD_BOUND = 1.1e-6                 # n * grad_q


def legal_bits(masks, shape):
    """bool [..., 5]: the legal set of CCX_SAMPLE step 2 (``masks`` None = everything legal); wait always is."""
    m = np.full(shape, 0x1F, np.uint8) if masks is None else np.asarray(masks, np.uint8).reshape(shape)
    m = (m & np.uint8(0x1F)) | np.uint8(0x10)
    return ((m[..., None] >> np.arange(5, dtype=np.uint8)) & 1).astype(bool)


def greedy_spec(v, legal):
    """int64 [...]: THE greedy action.  kg = the lowest legal k, mx = -inf; for legal k ascending, a strictly greater value
    takes over.  A NaN never wins; ties go to the lowest index."""
    v = np.asarray(v, F32)
    kg = legal.argmax(-1).astype(np.int64)
    mx = np.full(v.shape[:-1], NEG_INF, F32)
    with np.errstate(all="ignore"):
        for k in range(5):
            win = legal[..., k] & (v[..., k] > mx)
            mx = np.where(win, v[..., k], mx).astype(F32)
            kg = np.where(win, k, kg)
    return kg


# ---------------------------------------------------------------------------------------------------------------------
# ccx_q_actions
# ---------------------------------------------------------------------------------------------------------------------
def q_actions_spec(q, masks, terminated, truncated, step_count, episode, env_offset=0, seed=0, epsilon=None):
    """(actions u8 [E, N], explored u8 [E, N]).  ``epsilon`` None = greedy (nothing is drawn)."""
    q = np.asarray(q, F32)
    E, N, five = q.shape
    assert five == 5
    dead = (np.asarray(terminated).reshape(E, N) != 0) | (np.asarray(truncated).reshape(E, N) != 0)
    legal = legal_bits(masks, (E, N))
    action = greedy_spec(q, legal)
    explore = np.zeros((E, N), bool)
    if epsilon is not None:
        u1 = slot_words(seed, env_offset, E, N, step_count, episode, stream=K_Q_EXPLORE_STREAM)
        u2 = slot_words(seed, env_offset, E, N, step_count, episode, stream=K_Q_CHOICE_STREAM)
        r = (u1 >> U32(8)).astype(F32) * R_SCALE
        with np.errstate(all="ignore"):
            explore = r < F32(epsilon)                                   # (false for a NaN rate)
        n = legal.sum(-1).astype(np.uint64)
        idx = ((u2.astype(np.uint64) * n) >> np.uint64(32)).astype(np.int64)
        place = np.cumsum(legal, -1) - 1                                 # the rank of a legal k among the legal ones
        choice = (legal & (place == idx[..., None])).argmax(-1)
        action = np.where(explore, choice, action)
    actions = np.where(dead, ACTION_ABSENT, action).astype(np.uint8)
    return actions, (explore & ~dead).astype(np.uint8)


def q_actions_scalar(q, masks, terminated, truncated, step_count, episode, env_offset=0, seed=0, epsilon=None):
    """The header's steps literally, one slot at a time, with Python integers for the key."""
    from _sample_spec import random_word_int

    q = np.asarray(q, F32)
    E, N, _ = q.shape
    actions, explored = np.full((E, N), 77, np.uint8), np.full((E, N), 77, np.uint8)
    for e in range(E):
        for a in range(N):
            if terminated[e][a] or truncated[e][a]:
                actions[e, a], explored[e, a] = ACTION_ABSENT, 0
                continue
            m = ((0x1F if masks is None else int(masks[e][a])) & 0x1F) | 0x10
            ks = [k for k in range(5) if m >> k & 1]
            kg, mx = ks[0], NEG_INF
            for k in ks:
                if q[e, a, k] > mx:
                    mx, kg = q[e, a, k], k
            ex = False
            if epsilon is not None:
                key = (env_offset + e, int(episode[e]), int(step_count[e]), a)
                u1 = random_word_int(seed, K_Q_EXPLORE_STREAM, *key)
                u2 = random_word_int(seed, K_Q_CHOICE_STREAM, *key)
                ex = bool(F32(F32(u1 >> 8) * R_SCALE) < F32(epsilon))
                if ex:
                    kg = ks[(u2 * len(ks)) >> 32]
            actions[e, a], explored[e, a] = kg, int(ex)
    return actions, explored


def make_q_case(E: int, N: int, seed: int = 0, step_count=None, episode=None) -> dict:
    """make_sample_case (ties, NaN and +-inf at legal places, rows of -inf, NaN at dead slots and -- in ``q_masked`` -- at
    illegal places) with, in live slots too, rows that are NaN throughout and masks with one legal action."""
    case = make_sample_case(E, N, seed=seed, step_count=step_count, episode=episode)
    rng = np.random.default_rng(seed + 77)
    q, qm, masks = case["logits"].copy(), case["logits_masked"].copy(), case["masks"].copy()
    all_nan = rng.random((E, N)) < 0.05
    q[all_nan], qm[all_nan] = np.nan, np.nan
    one = rng.random((E, N)) < 0.08
    masks[one] &= 0xE0                                                    # junk in bits 5-7 stays; only wait is legal
    qm[one, :4] = np.nan
    inf_illegal = (rng.random((E, N)) < 0.1) & ((masks & 1) == 0)
    qm[inf_illegal, 0] = np.inf                                           # +inf at an illegal place never wins
    return dict(case, q=q, q_masked=qm, masks=masks)


# ---------------------------------------------------------------------------------------------------------------------
# ccx_td_loss / ccx_td_loss_backward
# ---------------------------------------------------------------------------------------------------------------------
def valid_ok(valid, M):
    return np.ones(M, bool) if valid is None else np.asarray(valid).reshape(M) != 0


def td_rows(q, actions, reward, done, q_next_target, q_next_online=None, masks_next=None, valid=None, weights=None, gamma=0.99,
            huber_delta=1.0, discount=None):
    """Steps 1-5 for every row (what rows that do not count hold is junk; ``counts`` says which do).  ``discount`` f32 [M]:
    include/ccx.h CCX_NSTEP's ``ccx_td_loss_discounted`` -- the same rule with ``discount[i]`` where it says gamma (step 4:
    ``nb = (done[i] || discount[i] == 0) ? +0.0 : discount[i] * boot``); ``gamma`` is then not read."""
    q = np.asarray(q, F32).reshape(-1, 5)
    M = q.shape[0]
    a = np.asarray(actions, np.uint8).reshape(M).astype(np.int64)
    ok = valid_ok(valid, M)
    counts = ok & (a <= 4)
    bad = ok & (a > 4) & (a != ACTION_ABSENT)
    qt = np.asarray(q_next_target, F32).reshape(M, 5)
    sel = qt if q_next_online is None else np.asarray(q_next_online, F32).reshape(M, 5)
    gamma, delta = F32(gamma) if discount is None else np.asarray(discount, F32).reshape(M), F32(huber_delta)
    with np.errstate(all="ignore"):
        c = F32(HALF * delta)
        qa = np.take_along_axis(q, np.minimum(a, 4)[:, None], -1)[:, 0]
        kstar = greedy_spec(sel, legal_bits(masks_next, (M,)))
        boot = np.take_along_axis(qt, kstar[:, None], -1)[:, 0]
        r = np.asarray(reward, F64).reshape(M).astype(F32)                # one rounding
        gb = (gamma * boot).astype(F32)
        nb = np.where((np.asarray(done).reshape(M) != 0) | (gamma == ZERO), ZERO, gb).astype(F32)
        y = (r + nb).astype(F32)
        d = (qa - y).astype(F32)
        ad = np.abs(d)
        h1 = (HALF * (d * d).astype(F32)).astype(F32)
        h2 = (delta * (ad - c).astype(F32)).astype(F32)
        h = np.where(ad <= delta, h1, h2).astype(F32)
        term = h if weights is None else (np.asarray(weights, F32).reshape(M) * h).astype(F32)
    return dict(M=M, a=a, counts=counts, bad=bad, qa=qa, kstar=kstar, boot=boot, y=y, d=d, ad=ad, h=h, term=term, delta=delta)


def td_finals(S):
    """stats f32 [8] from the six f64 sums (count, term, |d|, qa, y, bad)."""
    n = F64(S[0])
    out = np.zeros(8, F32)
    with np.errstate(all="ignore"):
        if n != 0:
            out[:4] = np.array([F64(S[k]) / n for k in (1, 2, 3, 4)], F64).astype(F32)
    out[6], out[7] = F32(n), F32(F64(S[5]))
    return out


def td_loss_spec(q, actions, reward, done, q_next_target, q_next_online=None, masks_next=None, valid=None, weights=None,
                 gamma=0.99, huber_delta=1.0, details=False, discount=None):
    """(stats f32 [8], td_error f32 [M])."""
    t = td_rows(q, actions, reward, done, q_next_target, q_next_online, masks_next, valid, weights, gamma, huber_delta, discount)
    c, zero = t["counts"], F64(0.0)
    S = [tree_sum(np.where(c, F64(1.0), zero))]
    for name in ("term", "ad", "qa", "y"):
        S.append(tree_sum(np.where(c, t[name].astype(F64), zero)))
    S.append(tree_sum(np.where(t["bad"], F64(1.0), zero)))
    stats = td_finals(S)
    td_error = np.where(c, t["d"], ZERO).astype(F32)
    return (stats, td_error, t) if details else (stats, td_error)


def td_loss_backward_spec(q, actions, reward, done, q_next_target, q_next_online=None, masks_next=None, valid=None, weights=None,
                          gamma=0.99, huber_delta=1.0, stats=None, grad_loss=None, discount=None):
    """grad_q f32 [M, 5]."""
    t = td_rows(q, actions, reward, done, q_next_target, q_next_online, masks_next, valid, weights, gamma, huber_delta, discount)
    M, delta = t["M"], t["delta"]
    n = F32(stats[6])
    g = ONE if grad_loss is None else F32(grad_loss)
    with np.errstate(all="ignore"):
        sc = F32(g / n)
        gw = np.full(M, sc, F32) if weights is None else (sc * np.asarray(weights, F32).reshape(M)).astype(F32)
        lim = np.where(t["d"] < ZERO, F32(ZERO - delta), delta).astype(F32)
        dd = np.where((t["ad"] <= delta) | np.isnan(t["d"]), t["d"], lim).astype(F32)
        ga = (gw * dd).astype(F32)
    counts = t["counts"] & bool(n != 0)
    hit = counts[:, None] & (np.arange(5)[None, :] == t["a"][:, None])
    return np.where(hit, ga[:, None], ZERO).astype(F32)


def make_td_case(M: int, seed: int = 0, density: float = 0.75, huber_delta: float = 1.0) -> dict:
    """Everything a TD-loss call reads, for calls with or without masks, double-Q, valid and weights (``td_args``).

    actions      0..4; 5 % 255 (absent), 3 % junk in 5..254 (7 among them)
    valid        not zero (1, 2 or 255) with probability ``density``
    done         20 %; half of the done rows have NaN throughout their next-state Q rows
    q            N(0, 2); NaN / +-inf at places other than the taken action in a tenth of the rows
    q_next_*     N(0, 2) with ties; in the online array NaN, -inf and +inf at legal places (a NaN never wins, +inf does: the
                 target array is finite there); in the target array NaN and -inf at places the bootstrap action cannot be (in
                 any variant), +inf only in done rows; the ``_masked`` arrays also hold NaN at every illegal place
    masks_next   bits 0-3 random, bit 4 mostly set, junk in bits 5-7; 8 % with wait the one legal action
    reward       f64 N(0, 1): not f32 values, so the one rounding shows
    |d| exactly huber_delta (and its two f32 neighbours) at 3 % of the rows: done rows with reward 0.5 and q[a] = 0.5 +- delta
    weights      U(0.5, 1.5), exactly 0 at 5 %
    Rows that never count (action 255 or junk) hold NaN in q, both next-state arrays, reward and weights; rows whose valid
    byte is 0 do so in the ``*_poisoned`` arrays, which calls with ``valid`` use."""
    rng = np.random.default_rng(seed + 9_000_011)
    delta = F32(huber_delta)
    a = rng.integers(0, 5, size=M).astype(np.uint8)
    u = rng.random(M)
    a[u < 0.05] = ACTION_ABSENT
    junk_rows = (u >= 0.05) & (u < 0.08)
    a[junk_rows] = rng.choice(np.array([5, 7, 7, 100, 254], np.uint8), size=int(junk_rows.sum()))
    valid = (rng.random(M) < density).astype(np.uint8)
    valid[valid != 0] = rng.choice(np.array([1, 1, 1, 2, 255], np.uint8), size=int((valid != 0).sum()))
    done = (rng.random(M) < 0.2).astype(np.uint8)
    done[done != 0] = rng.choice(np.array([1, 1, 4, 255], np.uint8), size=int((done != 0).sum()))
    q = (rng.standard_normal((M, 5)) * 2.0).astype(F32)
    qt = (rng.standard_normal((M, 5)) * 2.0).astype(F32)
    qo = (rng.standard_normal((M, 5)) * 2.0).astype(F32)
    tie = rng.random(M) < 0.1
    qo[tie, 1], qo[tie, 3] = qo[tie].max(-1), qo[tie].max(-1)
    qt[tie, 0], qt[tie, 2] = qt[tie].max(-1), qt[tie].max(-1)
    low = rng.integers(0, 16, size=M).astype(np.uint8)
    low[rng.random(M) < 0.08] = 0
    masks = low | np.where(rng.random(M) < 0.85, 0x10, 0).astype(np.uint8) | (rng.integers(0, 8, size=M).astype(np.uint8) << 5)
    legal = legal_bits(masks, (M,))
    reward = rng.standard_normal(M)
    weights = rng.uniform(0.5, 1.5, M).astype(F32)
    weights[rng.random(M) < 0.05] = ZERO
    # |d| = huber_delta exactly, and its neighbours
    edge = (rng.random(M) < 0.03) & (a <= 4)
    done[edge] = 1
    reward[edge] = 0.5
    idx = np.flatnonzero(edge)
    sign = np.where(rng.random(len(idx)) < 0.5, -1.0, 1.0).astype(F32)
    tgt = (F32(0.5) + sign * delta).astype(F32)
    nudge = rng.integers(0, 3, size=len(idx))
    tgt = np.where(nudge == 1, np.nextafter(tgt, F32(np.inf)), np.where(nudge == 2, np.nextafter(tgt, NEG_INF), tgt)).astype(F32)
    q[idx, a[idx]] = tgt
    # junk in q beside the taken action
    spoil = np.flatnonzero((rng.random(M) < 0.1) & (a <= 4))
    k = (a[spoil] + rng.integers(1, 5, size=len(spoil))) % 5
    q[spoil, k] = rng.choice(np.array([np.nan, np.inf, -np.inf], F32), size=len(spoil))
    # the online array: NaN / -inf / +inf at legal places
    rows = np.flatnonzero(rng.random(M) < 0.3)
    qo[rows, rng.integers(0, 4, size=len(rows))] = rng.choice(np.array([np.nan, -np.inf, np.inf], F32), size=len(rows))
    qo_m = np.where(legal, qo, F32(np.nan)).astype(F32)
    # the target array: NaN / -inf where no variant's bootstrap action can be
    everything = np.ones((M, 5), bool)
    taken = np.zeros((M, 5), bool)
    for sel, lg in ((qo, everything), (qo_m, legal), (qt, everything), (qt, legal)):
        taken[np.arange(M), greedy_spec(sel, lg)] = True
    rows = np.flatnonzero(rng.random(M) < 0.3)
    k = rng.integers(0, 4, size=len(rows))
    free = ~taken[rows, k]
    qt[rows[free], k[free]] = rng.choice(np.array([np.nan, -np.inf], F32), size=int(free.sum()))
    for sel, lg in ((qt, everything), (qt, legal)):                      # (a NaN or -inf never wins: the single-Q actions stay)
        assert not np.isnan(qt[np.arange(M), greedy_spec(sel, lg)]).any()
    dn = done != 0
    qt[dn & (rng.random(M) < 0.3), 4] = np.inf
    wipe = dn & (rng.random(M) < 0.5)
    qt[wipe], qo[wipe] = np.nan, np.nan
    qo_m = np.where(legal, qo, F32(np.nan)).astype(F32)
    qt_m = np.where(legal, qt, F32(np.nan)).astype(F32)
    out = dict(M=M, actions=a, valid=valid, done=done, masks=masks, huber_delta=float(delta))
    never = a > 4
    for poisoned in (False, True):
        gone = never | ((valid == 0) & poisoned)
        tag = "_poisoned" if poisoned else ""
        for name, arr in (("q", q), ("qt", qt), ("qo", qo), ("qt_masked", qt_m), ("qo_masked", qo_m)):
            out[name + tag] = np.where(gone[:, None], F32(np.nan), arr).astype(F32)
        out["reward" + tag] = np.where(gone, np.nan, reward)
        out["weights" + tag] = np.where(gone, F32(np.nan), weights).astype(F32)
    return out


def td_args(case, masked: bool = True, double: bool = True, with_valid: bool = True, with_weights: bool = True,
            M: int | None = None) -> dict:
    """Keyword arguments (q ... weights) of a generator case for one NULL combination of the optional inputs, its first M rows."""
    M = case["M"] if M is None else M
    tag = "_poisoned" if with_valid else ""
    mk = "_masked" if masked else ""
    kw = dict(q=case["q" + tag], actions=case["actions"], reward=case["reward" + tag], done=case["done"],
              q_next_target=case["qt" + mk + tag], q_next_online=case["qo" + mk + tag] if double else None,
              masks_next=case["masks"] if masked else None, valid=case["valid"] if with_valid else None,
              weights=case["weights" + tag] if with_weights else None)
    return {k: (None if v is None else np.ascontiguousarray(v[:M])) for k, v in kw.items()}


TD_VARIANTS = [(masked, double, with_valid, with_weights) for masked in (True, False) for double in (True, False)
               for with_valid in (True, False) for with_weights in (True, False)]
