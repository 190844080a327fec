"""CCX_PRIO (include/ccx.h) restated in NumPy f32 and Python integers, independent of the library.  TEST INFRASTRUCTURE ONLY.

The draw never mentions a tree: the leaves are summed with ``np.cumsum`` over Python integers (``dtype=object``: exact, no
width to overflow) and searched with ``bisect_right``.  ``exp_spec`` / ``log_spec`` are restated here line by line (they are
CCX_SAMPLE's; this section uses them on a wider domain: log on [2^-31, 2^15], exp on [-22, 11]).  The word is
tests/_sample_spec.py's."""

from bisect import bisect_right

import numpy as np
from _sample_spec import random_word

F32 = np.float32
K_PRIO_STREAM = 0x7F4A7C15
ONE_FIXED = 65536
LEAF_MAX = (1 << 31) - 1
MAX_TD = 8

# Accuracy of p = exp_spec(alpha * log_spec(x)) against f64 pow, relative, over x in [2^-31, 2^15] and alpha in {0.3, 0.6, 1}:
# measured on the CPU by tests/test_prio_spec.py (the maximum it prints: 1.09e-6) and DOUBLED.  include/ccx.h and the README
# quote the same number.
POW_REL_BOUND = 2.2e-6


def _h(text: str) -> np.float32:
    v = float.fromhex(text)
    assert float(F32(v)) == v, text
    return F32(v)


LOG2E, LN2_HI, LN2_LO = _h("0x1.715476p+0"), _h("0x1.62e4p-1"), _h("0x1.7f7d1cp-20")
EXP_C = tuple(_h(t) for t in ("0x1.a01a02p-13", "0x1.6c16c2p-10", "0x1.111112p-7", "0x1.555556p-5", "0x1.555556p-3", "0x1p-1",
                              "0x1p+0", "0x1p+0"))
SQRT_HALF = _h("0x1.6a09e6p-1")
LOG_C = tuple(_h(t) for t in ("0x1.c71c72p-4", "0x1.24924ap-3", "0x1.99999ap-3", "0x1.555556p-2"))
ONE, TWO = F32(1.0), F32(2.0)
X_LO, X_HI = _h("0x1p-16"), _h("0x1p+15")
F_TOP = _h("0x1.fffffep+30")


def exp_spec(x):
    """x f32, |x| <= 80: every line one f32 operation."""
    x = np.asarray(x, F32)
    n = np.rint(x * LOG2E)
    r = (x - n * LN2_HI) - n * LN2_LO
    p = EXP_C[0]
    for c in EXP_C[1:]:
        p = p * r + c
    return np.ldexp(p, n.astype(np.int32)).astype(F32)                    # exact: a normal number


def log_spec(s):
    """s f32, a positive normal number."""
    s = np.asarray(s, F32)
    m, e = np.frexp(s)                                                    # s = m * 2^e exactly, m in [0.5, 1)
    small = m < SQRT_HALF
    f = np.where(small, m + m, m).astype(F32)
    ef = np.where(small, e - 1, e).astype(F32)
    t = f - ONE
    q = t / (TWO + t)
    z = q * q
    p = LOG_C[0]
    for c in LOG_C[1:]:
        p = p * z + c
    u = q + q
    lf = u + u * (z * p)
    return (ef * LN2_HI + (lf + ef * LN2_LO)).astype(F32)


# ------------------------------------------------------------------------------------------------------------ update
def quantise_spec(m, alpha, eps) -> np.ndarray:
    """int64 array: the leaf of records whose largest |td| is m (f32 array, no NaN: they have been selected away)."""
    with np.errstate(over="ignore", invalid="ignore"):
        m, alpha, eps = np.asarray(m, F32), F32(alpha), F32(eps)
        s = m + eps
        x = np.where(s < X_LO, X_LO, np.where(s > X_HI, X_HI, s)).astype(F32)
        pw = exp_spec(alpha * log_spec(x))
        p = np.where(alpha == F32(0.0), ONE, pw).astype(F32)
        f = np.floor(p * F32(65536.0))
        c = np.where(f > F_TOP, F_TOP, f).astype(F32)
        return np.maximum(c.astype(np.int64), 1)


def td_max_spec(tds) -> np.ndarray:
    """f32 [B]: the maximum of |td| over all arrays [B, N] and agents, from +0.0; a NaN never wins."""
    B = tds[0].shape[0]
    m = np.zeros(B, F32)
    for td in tds:
        for n in range(td.shape[1]):
            a = np.abs(np.asarray(td[:, n], F32))
            with np.errstate(invalid="ignore"):
                m = np.where(a > m, a, m).astype(F32)
    return m


def update_spec(leaf: np.ndarray, pstate: np.ndarray, index, tds, alpha, eps) -> None:
    """In place, b by b: the maximum over duplicates is a maximum over a list."""
    tds = [tds] if isinstance(tds, np.ndarray) else list(tds)
    assert 1 <= len(tds) <= MAX_TD
    new = quantise_spec(td_max_spec(tds), alpha, eps)
    R = leaf.shape[0]
    named = {}
    for b, i in enumerate(np.asarray(index, np.int64).tolist()):
        if 0 <= i < R and leaf[i] != 0:
            named.setdefault(i, []).append(int(new[b]))
    for i, values in named.items():
        leaf[i] = max(values)
        pstate[0] = max(int(pstate[0]), max(values))


# ------------------------------------------------------------------------------------------------------------ push
def push_leaf_spec(leaf: np.ndarray, pstate: np.ndarray, head: int, K: int, S: int, E: int) -> None:
    """leaf = max_leaf at the K * E slots of a block pushed at ``head`` (the head BEFORE the push)."""
    for s in range(K):
        for e in range(E):
            leaf[((head + s) % S) * E + e] = int(pstate[0])


# ------------------------------------------------------------------------------------------------------------ draw
def point_spec(w0: int, w1: int, b: int, B: int, stratified: bool) -> int:
    x = (w0 << 32) | w1
    return ((b << 64) + x) // B if stratified else x


def words_spec(seed: int, d: int, B: int):
    b = np.arange(B, dtype=np.int64)
    key = (b, d & 0xFFFFFFFF, (d >> 32) & 0xFFFFFFFF)
    return random_word(seed, K_PRIO_STREAM, *key, 0), random_word(seed, K_PRIO_STREAM, *key, 1)


def index_of_point(cum: list, x: int) -> int:
    """The record a point x in [0, 2^64) picks: the smallest i with cum[i] > u, u = (x T) >> 64."""
    T = cum[-1] if cum else 0
    if T == 0:
        return -1
    return bisect_right(cum, (x * T) >> 64)


def cumsum_spec(leaf) -> list:
    return np.cumsum(np.array([int(v) for v in leaf], dtype=object)).tolist() if len(leaf) else []


def draw_spec(leaf, seed: int, d: int, B: int, stratified: bool) -> np.ndarray:
    cum = cumsum_spec(leaf)
    w0, w1 = words_spec(seed, d, B)
    return np.array([index_of_point(cum, point_spec(int(h), int(l), b, B, stratified)) for b, (h, l) in enumerate(zip(w0, w1))],
                    np.int64)


def weight_spec(min_leaf: int, leaf_drawn, beta) -> np.ndarray:
    """f32 [B]: (min_leaf / leaf)^beta; +0.0 where leaf_drawn is 0 (nothing drawn)."""
    ld = np.asarray(leaf_drawn, np.int64)
    drawn = ld > 0
    beta = F32(beta)
    bt = F32(0.0) if beta < 0 else (F32(1.0) if beta > 1 else beta)
    r = (np.float64(min_leaf) / np.where(drawn, ld, 1).astype(np.float64)).astype(F32)
    w = exp_spec(bt * log_spec(np.where(drawn, r, ONE).astype(F32)))
    return np.where(drawn, w, F32(0.0)).astype(F32)


def sample_spec(leaf: np.ndarray, pstate: np.ndarray, seed: int, B: int, N: int, beta, stratified: bool) -> dict:
    """One sample launch: index, weights [B, N], leaf_drawn; writes T and min_leaf and advances draws in ``pstate``."""
    ints = [int(v) for v in leaf]
    nz = [v for v in ints if v != 0]
    pstate[2], pstate[3] = sum(ints), (min(nz) if nz else 0)
    index = draw_spec(leaf, seed, int(pstate[1]), B, stratified)
    ld = np.where(index >= 0, np.asarray(leaf, np.int64)[np.maximum(index, 0)], 0).astype(np.int32)
    w = weight_spec(int(pstate[3]), ld, beta)
    pstate[1] += 1
    return dict(index=index, weights=np.repeat(w[:, None], N, axis=1), leaf_drawn=ld)


def new_pstate() -> np.ndarray:
    return np.array([ONE_FIXED, 0, 0, 0], np.int64)
