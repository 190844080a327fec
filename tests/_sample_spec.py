"""CCX_SAMPLE as include/ccx.h states it, restated in NumPy on the CPU, plus a generator of adversarial cases.  TEST
INFRASTRUCTURE ONLY: what the sampling kernel is compared with.

Written from the header paragraph, not from the kernel.  ``sample_spec`` advances every slot at once with elementwise
``np.float32`` operations (one IEEE binary32 rounding each: no reduction, nothing a library could reassociate or fuse) and
``np.uint32`` arithmetic for the key; what the rule does not read is selected away with ``np.where`` (a select: the
unselected operand never reaches the result), never multiplied by zero.  ``sample_scalar`` is the header's pseudo-code
literally, one slot at a time, with ``np.float32`` scalars and Python integers for the key.  Every comparison against this
module is on bit patterns."""

from __future__ import annotations

import numpy as np

F32 = np.float32
U32 = np.uint32
ACTION_ABSENT = 255
K_SAMPLE_STREAM = 0x2545F491           # kSampleStream (include/ccx.h CCX_SAMPLE); 0 = CCX_POLICY_RANDOM, 0x5BD1E995 = epsilon
K_EPS_STREAM = 0x5BD1E995


def _h(text: str) -> np.float32:
    v = float.fromhex(text)
    assert float(F32(v)) == v, text      # every constant of the header is an f32 value
    return F32(v)


# the header's constants, as it writes them
LOG2E = _h("0x1.715476p+0")
LN2_HI = _h("0x1.62e4p-1")             # 15 significant bits: n * LN2_HI is exact for |n| < 2^9
LN2_LO = _h("0x1.7f7d1cp-20")
EXP_C = tuple(_h(t) for t in ("0x1.a01a02p-13", "0x1.6c16c2p-10", "0x1.111112p-7", "0x1.555556p-5", "0x1.555556p-3",
                              "0x1p-1", "0x1p+0", "0x1p+0"))       # 1/7!, 1/6!, ..., 1/2!, 1, 1: Horner, highest first
SQRT_HALF = _h("0x1.6a09e6p-1")
LOG_C = tuple(_h(t) for t in ("0x1.c71c72p-4", "0x1.24924ap-3", "0x1.99999ap-3", "0x1.555556p-2"))   # 1/9, 1/7, 1/5, 1/3
D_MIN = F32(-80.0)
ONE, TWO, ZERO = F32(1.0), F32(2.0), F32(0.0)
R_SCALE = _h("0x1p-24")
NEG_INF, POS_INF = F32(-np.inf), F32(np.inf)

# Accuracy against NumPy f64, measured on the CPU by tests/test_sample_spec.py (the maxima it prints) and DOUBLED for the
# inputs its samples did not hit (measured: 9.88e-8, 4.58e-7, 2.11e-7).  The header paragraph and DESIGN.md 3.12 quote the same three numbers.
EXP_REL_BOUND = 2.0e-7                 # exp_spec on [-80, 0], relative
LOGP_ABS_BOUND = 9.2e-7                # logp, absolute, over the generator's non-degenerate slots
ENTROPY_ABS_BOUND = 4.3e-7             # entropy, absolute, likewise


def bits32(a) -> np.ndarray:
    """f32 as u32 bit patterns for exact comparison (the sign of zero and NaN payloads included)."""
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


# ---------------------------------------------------------------------------------------------------------------------
# exp_spec / log_spec: work on arrays and on np.float32 scalars alike (every operation is an elementwise f32 one)
# ---------------------------------------------------------------------------------------------------------------------
def exp_spec(x):
    """x f32 in [-80, 0] (anything else must have been selected away by the caller)."""
    n = np.rint(x * LOG2E)
    r = (x - n * LN2_HI) - n * LN2_LO
    p = EXP_C[0]
    for c in EXP_C[1:]:
        p = p * r + c                                   # one multiply, one add
    return np.ldexp(p, np.asarray(n).astype(np.int32)).astype(F32)      # exact: the result is a normal number


def log_spec(s):
    """s f32 in [1, 5]."""
    m, e = np.frexp(s)                                  # s = m * 2^e exactly, m in [0.5, 1)
    small = m < SQRT_HALF
    f = np.where(small, m + m, m).astype(F32)           # m + m is exact
    ef = np.where(small, e - 1, e).astype(F32)
    t = f - ONE                                         # exact
    q = t / (TWO + t)
    z = q * q
    p = LOG_C[0]
    for c in LOG_C[1:]:
        p = p * z + c
    u = q + q                                           # exact
    lf = u + u * (z * p)
    return (ef * LN2_HI + (lf + ef * LN2_LO)).astype(F32)


# ---------------------------------------------------------------------------------------------------------------------
# the key
# ---------------------------------------------------------------------------------------------------------------------
def _mix(k):
    k = k ^ (k >> U32(16))
    k = k * U32(0x7FEB352D)
    k = k ^ (k >> U32(15))
    k = k * U32(0x846CA68B)
    return k ^ (k >> U32(16))


def _u32(v) -> np.ndarray:
    return np.atleast_1d((np.asarray(v, np.int64) & 0xFFFFFFFF).astype(U32))


def random_word(seed: int, stream: int, g, j, t, a) -> np.ndarray:
    """The word of ccx_set_rng_seed's formula with seed_hi ^ stream, in np.uint32 array arithmetic (wraps mod 2^32).
    g, j, t, a: integer arrays (64-bit at most; reduced to u32 here), broadcast against each other."""
    lo, hi = U32(seed & 0xFFFFFFFF), U32(((seed >> 32) & 0xFFFFFFFF) ^ stream)
    g, j, t, a = _u32(g), _u32(j), _u32(t), _u32(a)
    k = g * U32(0x9E3779B1) + j * U32(0x85EBCA77) + t * U32(0xC2B2AE3D) + a * U32(0x27D4EB2F) + lo
    return _mix(_mix(k) ^ hi)


def slot_words(seed: int, env_offset: int, E: int, N: int, step_count, episode, stream: int = K_SAMPLE_STREAM) -> np.ndarray:
    """u32 [E, N]: the draw of every slot of a batch (g = env_offset + e, j = episode[e], t = step_count[e], a)."""
    g = int(env_offset) + np.arange(E, dtype=np.int64)
    return random_word(seed, stream, g[:, None], np.asarray(episode)[:, None], np.asarray(step_count)[:, None],
                       np.arange(N)[None, :])


# ---------------------------------------------------------------------------------------------------------------------
# the rule, every slot at once
# ---------------------------------------------------------------------------------------------------------------------
def sample_spec(logits, masks, terminated, truncated, step_count, episode, env_offset=0, seed=0, deterministic=False,
                details=False):
    """(actions u8 [E, N], logp f32 [E, N], entropy f32 [E, N]); with ``details`` also a dict of the intermediates (dead,
    legal, degenerate, w, c, S) for the identity tests."""
    logits = np.asarray(logits, F32)
    E, N, five = logits.shape
    assert five == 5
    dead = (np.asarray(terminated).reshape(E, N) != 0) | (np.asarray(truncated).reshape(E, N) != 0)
    m = np.full((E, N), 0x1F, np.uint8) if masks is None else np.asarray(masks, np.uint8).reshape(E, N)
    m = (m & np.uint8(0x1F)) | np.uint8(0x10)
    legal = ((m[..., None] >> np.arange(5, dtype=np.uint8)) & 1).astype(bool)          # [E, N, 5]
    with np.errstate(all="ignore"):
        lg = np.where(legal, logits, NEG_INF)                                        # illegal logits selected away
        mx = np.full((E, N), NEG_INF, F32)
        for k in range(5):
            mx = np.where(legal[..., k] & (lg[..., k] > mx), lg[..., k], mx)         # by comparisons, ascending k
        bad = legal & (np.isnan(lg) | (lg == POS_INF))
        degenerate = bad.any(-1) | (mx == NEG_INF)
        safe = np.where(legal & ~degenerate[..., None], lg, ZERO)
        d = np.where(legal & ~degenerate[..., None], safe - np.where(degenerate, ZERO, mx)[..., None], ZERO)
        cut = d < D_MIN                                                              # (-inf included)
        w = np.where(legal & ~cut, exp_spec(np.where(cut, ZERO, d)), ZERO)
        c = np.empty((E, N, 5), F32)
        c[..., 0] = w[..., 0]
        for k in range(1, 5):
            c[..., k] = c[..., k - 1] + w[..., k]
        S = c[..., 4]
        if deterministic:
            hit = legal & (degenerate[..., None] | (lg == mx[..., None]))
        else:
            u = slot_words(seed, env_offset, E, N, step_count, episode)
            r = (u >> U32(8)).astype(F32) * R_SCALE
            thr = r * S
            hit = legal & (c > thr[..., None])
        action = np.where(hit.any(-1), hit.argmax(-1), 4)                            # lowest such k, else wait
        ls = log_spec(S)
        d_a = np.take_along_axis(d, action[..., None], -1)[..., 0]
        logp = d_a - ls
        term = np.where(w == ZERO, ZERO, w * np.where(w == ZERO, ZERO, d))           # selected, never multiplied
        T = term[..., 0]
        for k in range(1, 5):
            T = T + term[..., k]
        entropy = ls - T / S
    actions = np.where(dead, ACTION_ABSENT, action).astype(np.uint8)
    logp = np.where(dead, ZERO, logp).astype(F32)
    entropy = np.where(dead, ZERO, entropy).astype(F32)
    if details:
        return actions, logp, entropy, dict(dead=dead, legal=legal, degenerate=degenerate, w=w, c=c, S=S, d=d)
    return actions, logp, entropy


# ---------------------------------------------------------------------------------------------------------------------
# the header's pseudo-code, slot by slot
# ---------------------------------------------------------------------------------------------------------------------
def _mix_int(k: int) -> int:
    k ^= k >> 16
    k = (k * 0x7FEB352D) & 0xFFFFFFFF
    k ^= k >> 15
    k = (k * 0x846CA68B) & 0xFFFFFFFF
    return k ^ (k >> 16)


def random_word_int(seed: int, stream: int, g: int, j: int, t: int, a: int) -> int:
    lo, hi = seed & 0xFFFFFFFF, ((seed >> 32) & 0xFFFFFFFF) ^ stream
    M = 0xFFFFFFFF
    k = ((g & M) * 0x9E3779B1 + (j & M) * 0x85EBCA77 + (t & M) * 0xC2B2AE3D + (a & M) * 0x27D4EB2F + lo) & M
    return _mix_int(_mix_int(k) ^ hi)


def sample_scalar(logits, masks, terminated, truncated, step_count, episode, env_offset=0, seed=0, deterministic=False):
    logits = np.asarray(logits, F32)
    E, N, _ = logits.shape
    actions = np.full((E, N), 77, np.uint8)
    logp = np.full((E, N), np.nan, F32)
    entropy = np.full((E, N), np.nan, F32)
    with np.errstate(all="ignore"):
        for e in range(E):
            for a in range(N):
                if terminated[e][a] or truncated[e][a]:                              # 1. dead slots
                    actions[e, a], logp[e, a], entropy[e, a] = ACTION_ABSENT, ZERO, ZERO
                    continue
                m = ((0x1F if masks is None else int(masks[e][a])) & 0x1F) | 0x10    # 2. legal set
                ks = [k for k in range(5) if m >> k & 1]
                lk = {k: F32(logits[e, a, k]) for k in ks}
                mx = NEG_INF                                                         # 3. max
                for k in ks:
                    if lk[k] > mx:
                        mx = lk[k]
                degenerate = any(np.isnan(lk[k]) or lk[k] == POS_INF for k in ks) or mx == NEG_INF     # 4.
                d = {k: (ZERO if degenerate else F32(lk[k] - mx)) for k in ks}       # 5. weights
                w = [ZERO] * 5
                for k in ks:
                    w[k] = ZERO if d[k] < D_MIN else F32(exp_spec(d[k]))
                c = [w[0]]                                                           # 6. prefix sums
                for k in range(1, 5):
                    c.append(F32(c[k - 1] + w[k]))
                S = c[4]
                if deterministic:                                                    # 8. action
                    action = next(k for k in ks if degenerate or lk[k] == mx)
                else:
                    u = random_word_int(seed, K_SAMPLE_STREAM, env_offset + e, int(episode[e]), int(step_count[e]), a)   # 7.
                    r = F32(F32(u >> 8) * R_SCALE)
                    thr = F32(r * S)
                    action = next((k for k in ks if c[k] > thr), 4)
                ls = F32(log_spec(S))
                T = None                                                             # 10. entropy
                for k in range(5):
                    term = ZERO if w[k] == ZERO else F32(w[k] * d[k])
                    T = term if T is None else F32(T + term)
                actions[e, a] = action
                logp[e, a] = F32(d[action] - ls)                                     # 9. log-prob
                entropy[e, a] = F32(ls - F32(T / S))
    return actions, logp, entropy


# ---------------------------------------------------------------------------------------------------------------------
# adversarial cases
# ---------------------------------------------------------------------------------------------------------------------
SLOT_CLASSES = ("plain", "plain", "plain", "wide", "ties", "neg_inf", "huge_pair", "degenerate", "cutoff", "tiny")


def make_sample_case(E: int, N: int, seed: int = 0, step_count=None, episode=None) -> dict:
    """A batch for CCX_SAMPLE.  Per slot one of SLOT_CLASSES:
      plain       logits ~ N(0, 3)
      wide        N(0, 3) x 40: spreads beyond 80, the cutoff bites
      ties        the maximum repeated at one or two more places
      neg_inf     -inf at some legal places, not all
      huge_pair   +3e38 and -3e38 in one slot: their difference overflows
      degenerate  every legal logit -inf / a legal NaN / a legal +inf
      cutoff      differences of exactly -80 and its two f32 neighbours
      tiny        differences that are subnormal, signed zeros
    Masks: bits 0-3 random, bit 4 mostly set (the rule sets it anyway), junk in bits 5-7.  ``logits`` has NaN at every dead
    slot (terminated / truncated, 10 % each); ``logits_masked`` also at every k the mask rules out -- use it with the
    masks, ``logits`` without.  step_count / episode default to random values up to 2^31 - 1."""
    rng = np.random.default_rng(seed)
    logits = (rng.standard_normal((E, N, 5)) * 3.0).astype(F32)
    low = rng.integers(0, 16, size=(E, N)).astype(np.uint8)
    bit4 = np.where(rng.random((E, N)) < 0.85, 0x10, 0).astype(np.uint8)
    masks = low | bit4 | (rng.integers(0, 8, size=(E, N)).astype(np.uint8) << 5)
    legal = (((masks[..., None] | 0x10) >> np.arange(5, dtype=np.uint8)) & 1).astype(bool)
    cls = rng.integers(0, len(SLOT_CLASSES), size=(E, N))
    for e in range(E):
        for a in range(N):
            name = SLOT_CLASSES[cls[e, a]]
            l = logits[e, a]
            ks = np.flatnonzero(legal[e, a])
            if name == "wide":
                l *= F32(40.0)
            elif name == "ties":
                top = l[ks].max()
                for k in rng.choice(5, size=rng.integers(1, 3), replace=False):
                    l[k] = top
            elif name == "neg_inf":
                for k in rng.choice(5, size=rng.integers(1, 4), replace=False):
                    l[k] = -np.inf
                if np.all(np.isneginf(l[ks])) and rng.random() < 0.7:
                    l[4] = F32(0.25)
            elif name == "huge_pair":
                i, j = rng.choice(5, size=2, replace=False)
                l[i], l[j] = F32(3e38), F32(-3e38)
            elif name == "degenerate":
                kind = rng.integers(0, 3)
                if kind == 0:
                    l[:] = -np.inf
                else:
                    l[rng.choice(ks)] = np.nan if kind == 1 else np.inf
            elif name == "cutoff":
                base = F32(rng.choice([0.0, 1.5, -3.25, 100.0]))
                lo = F32(base + D_MIN)
                l[:] = [base, lo, np.nextafter(lo, NEG_INF), np.nextafter(lo, POS_INF), F32(base - F32(79.5))]
                l[:] = l[rng.permutation(5)]
            elif name == "tiny":
                l[:] = rng.choice(np.array([0.0, -0.0, 1e-40, -1e-40, 1e-45, -3e-39], F32), size=5)
    terminated = (rng.random((E, N)) < 0.1).astype(np.uint8)
    truncated = (rng.random((E, N)) < 0.1).astype(np.uint8)
    dead = (terminated | truncated) != 0
    logits[dead] = np.nan
    masked = logits.copy()
    masked[~legal] = np.nan
    if step_count is None:
        step_count = rng.integers(0, 1 << 31, size=E).astype(np.int32)
        step_count[: max(1, E // 4)] = rng.integers(0, 50, size=max(1, E // 4))
    if episode is None:
        episode = rng.integers(0, 1 << 31, size=E).astype(np.int32)
        episode[::3] = rng.integers(0, 20, size=len(episode[::3]))
    return dict(logits=logits, logits_masked=masked, masks=masks, terminated=terminated, truncated=truncated,
                step_count=np.asarray(step_count, np.int32), episode=np.asarray(episode, np.int32), classes=cls)


def reference_f64(logits, masks):
    """(log-softmax f64 [E, N, 5] with -inf at illegal k, entropy f64 [E, N]) of the masked logits, in NumPy f64."""
    x = np.asarray(logits, np.float64)
    E, N, _ = x.shape
    m = np.full((E, N), 0x1F, np.uint8) if masks is None else np.asarray(masks, np.uint8)
    legal = (((m[..., None] | 0x10) >> np.arange(5, dtype=np.uint8)) & 1).astype(bool)
    with np.errstate(all="ignore"):
        x = np.where(legal, x, -np.inf)
        mx = x.max(-1, keepdims=True)
        dd = x - mx
        lse = np.log(np.exp(dd).sum(-1, keepdims=True))
        lp = dd - lse
        p = np.exp(lp)
        ent = -np.where(p > 0, p * lp, 0.0).sum(-1)
    return lp, ent
