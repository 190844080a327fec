"""CCX_REPLAY (include/ccx.h) restated in NumPy and Python integers, independent of the library: the ring as a dict of arrays,
``push_spec`` (rollout arrays to records), ``draw_spec`` (the record indices of one sample launch; the 128-bit product in
Python integers) and ``fetch_spec`` (records to a minibatch, rows built from the compact records by a plain restatement of
the DefaultObservation layout).  The word is tests/_sample_spec.py's."""

import numpy as np
from _sample_spec import random_word, random_word_int

K_REPLAY_STREAM = 0x3C6EF372
AF_TERMINATED, AF_LIVE, EF_RESET = 0x01, 0x04, 0x04
EMPTY_ACTION, EMPTY_MASKS, MASKS_ALL = 255, 0x10, 0x1F
ARRAYS = ("obs_c", "next_c", "actions", "reward", "done", "valid", "masks_next")


def new_ring(S: int, E: int, N: int) -> dict:
    """S * E copies of the EMPTY record, head = draws = 0."""
    R = S * E
    return dict(S=S, E=E, N=N, obs_c=np.zeros((R, N, 4), np.float32), next_c=np.zeros((R, N, 4), np.float32),
                actions=np.full((R, N), EMPTY_ACTION, np.uint8), reward=np.zeros((R, N), np.float64),
                done=np.zeros((R, N), np.uint8), valid=np.zeros((R, N), np.uint8),
                masks_next=np.full((R, N), EMPTY_MASKS, np.uint8), state=np.zeros(4, np.int64))


def slot_spec(head: int, s: int, S: int, E: int, e: int) -> int:
    return ((head + s) % S) * E + e


def filled_spec(head: int, S: int, E: int) -> int:
    return min(head, S) * E


def push_spec(ring: dict, obs0_compact, actions, reward, agent_flags, env_flags, obs_compact, final_compact=None,
              masks_next=None) -> None:
    """One block of K steps, step by step and env by env, in place."""
    S, E = ring["S"], ring["E"]
    K = actions.shape[0]
    assert 1 <= K <= S
    head = int(ring["state"][0])
    for s in range(K):
        for e in range(E):
            at = slot_spec(head, s, S, E, e)
            reset = final_compact is not None and bool(env_flags[s, e] & EF_RESET)
            ring["obs_c"][at] = obs0_compact[e] if s == 0 else obs_compact[s - 1, e]
            ring["next_c"][at] = final_compact[s, e] if reset else obs_compact[s, e]
            ring["actions"][at] = actions[s, e]
            ring["reward"][at] = reward[s, e]
            ring["done"][at] = agent_flags[s, e] & AF_TERMINATED
            ring["valid"][at] = agent_flags[s, e] & AF_LIVE
            ring["masks_next"][at] = MASKS_ALL if (reset or masks_next is None) else masks_next[s, e]
    ring["state"][0] = head + K


def draw_one(seed: int, F: int, d: int, b: int) -> int:
    """index[b] of launch d over F records, in Python integers throughout."""
    if F == 0:
        return -1
    key = (b & 0xFFFFFFFF, d & 0xFFFFFFFF, (d >> 32) & 0xFFFFFFFF)
    w0 = random_word_int(seed, K_REPLAY_STREAM, *key, 0)
    w1 = random_word_int(seed, K_REPLAY_STREAM, *key, 1)
    return (((w0 << 32) | w1) * F) >> 64


def draw_spec(seed: int, F: int, d: int, B: int) -> np.ndarray:
    """int64 [B]: the words as uint32 arrays, the 128-bit product one draw at a time in Python integers."""
    if F == 0:
        return np.full(B, -1, np.int64)
    b = np.arange(B, dtype=np.int64)
    w0 = random_word(seed, K_REPLAY_STREAM, b, d & 0xFFFFFFFF, (d >> 32) & 0xFFFFFFFF, 0)
    w1 = random_word(seed, K_REPLAY_STREAM, b, d & 0xFFFFFFFF, (d >> 32) & 0xFFFFFFFF, 1)
    return np.array([(((int(h) << 32) | int(l)) * F) >> 64 for h, l in zip(w0, w1)], np.int64)


def sample_index_spec(ring: dict, seed: int, B: int) -> np.ndarray:
    """The indices of the next sample launch; advances ``draws``."""
    head, d = int(ring["state"][0]), int(ring["state"][1])
    index = draw_spec(seed, filled_spec(head, ring["S"], ring["E"]), d, B)
    ring["state"][1] = d + 1
    return index


def rows_spec(compact: np.ndarray, consts) -> np.ndarray:
    """DefaultObservation rows f32 [..., N, 6 + 4 N] of compact records f32 [..., N, 4]; consts = (door centre, division
    row, door left, door right).  Row i: (x_i, y_i, consts) and then the four numbers of every slot j, -1 four times at
    j == i."""
    compact = np.asarray(compact, np.float32)
    N = compact.shape[-2]
    lead = compact.shape[:-2]
    rows = np.empty(lead + (N, 6 + 4 * N), np.float32)
    for i in range(N):
        rows[..., i, 0:2] = compact[..., i, 0:2]
        rows[..., i, 2:6] = np.asarray(consts, np.float32)
        for j in range(N):
            rows[..., i, 6 + 4 * j:10 + 4 * j] = np.float32(-1.0) if j == i else compact[..., j, :]
    return rows


def fetch_spec(ring: dict, index, consts) -> dict:
    """The minibatch of record indices ``index``: copies of the records' fields, the EMPTY record outside [0, R)."""
    index = np.asarray(index, np.int64)
    R = ring["S"] * ring["E"]
    empty = new_ring(1, 1, ring["N"])
    out = {}
    inside = (index >= 0) & (index < R)
    at = np.where(inside, index, 0)
    for k in ARRAYS:
        got = ring[k][at].copy()
        got[~inside] = empty[k][0]
        out[k] = got
    out["obs"], out["next_obs"] = rows_spec(out.pop("obs_c"), consts), rows_spec(out.pop("next_c"), consts)
    out["index"] = index.copy()
    return out
