"""CCX_MINIBATCH (include/ccx.h) restated in NumPy and Python integers, independent of the library: the keyed permutation
(``perm_spec``: all positions at once in uint32 arrays, a masked cycle walk), the draw of one launch (``draw_spec``), the state
(``advance_spec``) and the gather (``gather_spec``: records to a minibatch, rows of the compact form built by
tests/_replay_spec.py's plain restatement of the DefaultObservation layout).  The word is tests/_sample_spec.py's."""

import numpy as np
from _replay_spec import rows_spec
from _sample_spec import random_word

K_MINIBATCH_STREAM = 0x1B873593
ROUNDS = 6
EMPTY_ACTION, EMPTY_MASKS, MASKS_ALL, VALID_LIVE = 255, 0x10, 0x1F, 4
M_LIST = (1, 2, 3, 4, 5, 6, 7, 8, 9, 15, 16, 17, 33, 63, 64, 65, 129, 255, 256, 257, 513, 1000, 1023, 1025, 2049, 4097, 65537,
          131073, 262145)
U32 = np.uint32


def split_spec(M: int):
    """(w, a, b): the smallest w >= 2 with 2^w >= M, a = w // 2 bits of L, b = w - a bits of R."""
    w = 2
    while (1 << w) < M:
        w += 1
    return w, w // 2, w - w // 2


def rounds_spec(x, M: int, seed: int, epoch: int, rounds: int = ROUNDS):
    """The six rounds on a uint32 array of values below 2^w."""
    w, a, b = split_spec(M)
    x = np.asarray(x, U32)
    L, R, wl = x >> U32(b), x & U32((1 << b) - 1), a
    for r in range(rounds):
        f = random_word(seed, K_MINIBATCH_STREAM, R, epoch & 0xFFFFFFFF, (epoch >> 32) & 0xFFFFFFFF, r) & U32((1 << wl) - 1)
        L, R = R, L ^ f
        wl = w - wl
    assert wl == (a if rounds % 2 == 0 else b)
    return (L << U32(w - wl)) | R


def perm_spec(M: int, seed: int, epoch: int, positions=None, rounds: int = ROUNDS, want_steps: bool = False):
    """int64: pi_epoch(p) for every p of ``positions`` (default 0 .. M - 1); with ``want_steps`` also the walk lengths."""
    p = np.arange(M, dtype=np.int64) if positions is None else np.asarray(positions, np.int64).reshape(-1)
    assert ((p >= 0) & (p < M)).all() and 1 <= M < 1 << 31
    x = p.astype(U32)
    steps = np.zeros(len(x), np.int64)
    walking = np.ones(len(x), bool)
    while walking.any():
        x[walking] = rounds_spec(x[walking], M, seed, epoch, rounds)
        steps[walking] += 1
        walking &= x >= M
    out = x.astype(np.int64)
    return (out, steps) if want_steps else out


def draw_spec(M: int, B: int, seed: int, state) -> np.ndarray:
    """index int64 [B] of a draw at ``state`` = (epoch, cursor, ...); the state is not changed."""
    epoch, cursor = int(state[0]), int(state[1])
    index = np.full(B, -1, np.int64)
    if cursor >= 0:
        n = max(0, min(B, M - cursor))
        if n:
            index[:n] = perm_spec(M, seed, epoch & (2**64 - 1), cursor + np.arange(n))
    return index


def advance_spec(state, B: int, M: int) -> None:
    """The state behind a draw of B rows, in place (Python integers; the epoch wraps as u64 -> i64)."""
    epoch, cursor = int(state[0]), int(state[1])
    if cursor < 0 or cursor + B >= M:
        epoch = (epoch + 1) & (2**64 - 1)
        epoch, cursor = (epoch - 2**64 if epoch >= 2**63 else epoch), 0
    else:
        cursor += B
    state[0], state[1] = epoch, cursor


def next_spec(M: int, B: int, seed: int, state) -> np.ndarray:
    """One ``next``: the indices, and the state advanced in place."""
    index = draw_spec(M, B, seed, state)
    advance_spec(state, B, M)
    return index


def gather_spec(src: dict, index, E: int, consts) -> dict:
    """The minibatch of record indices ``index``.  ``src``: obs (rows [K, E, N, L], compact [K, E, N, 4] or None), obs0 (same
    form, [E, N, .], or None), actions, logp, advantages, returns, masks (or None), valid (or None), each [K, E, N]."""
    index = np.asarray(index, np.int64)
    K, _, N = src["actions"].shape
    M, B = K * E, len(index)
    inside = (index >= 0) & (index < M)
    at = np.where(inside, index, 0)
    s, e = at // E, at % E
    out = {}
    for k, empty in (("actions", EMPTY_ACTION), ("logp", 0.0), ("advantages", 0.0), ("returns", 0.0)):
        got = src[k][s, e].copy()
        got[~inside] = empty
        out[k] = got
    for k, absent, empty in (("masks", MASKS_ALL, EMPTY_MASKS), ("valid", VALID_LIVE, 0)):
        got = np.full((B, N), absent, np.uint8) if src.get(k) is None else src[k][s, e].copy()
        got[~inside] = empty
        out[k] = got
    obs = src.get("obs")
    if obs is not None:
        compact = obs.shape[-1] == 4
        obs0 = src.get("obs0")
        if obs0 is None:
            got = obs[s, e].copy()
        else:
            got = np.where((s == 0)[:, None, None], obs0[e], obs[np.maximum(s - 1, 0), e])
        if compact:
            got[~inside] = 0.0
            got = rows_spec(got, consts)
        else:
            got[~inside] = rows_spec(np.zeros((N, 4), np.float32), consts)
        out["obs"] = got
    else:
        out["obs"] = None
    out["index"] = index.copy()
    return out
