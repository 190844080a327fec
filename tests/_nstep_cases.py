"""What the tests of CCX_NSTEP share: the geometry of the rollout case (the shapes of tests/test_gpu_replay.py with a ring of
6 steps), the count of what ends the windows of a fetch, and the SYNTHETIC ring -- arrays written directly -- that holds every
edge of the rule at a known record."""

import numpy as np
from _nstep_spec import new_cut, window_spec
from _replay_spec import new_ring
from _reset_obs_spec import make_config

E, S = 24, 6
MAX_STEPS = 8
BLOCKS = (1, 3, 2, 4)                              # heads 1, 4, 6, 10: partly filled, full, wrapped and rewritten
POOL = dict(seed0=7, size=64)
EPSILON = 0.1                                      # of the scripted greedy policy: agents arrive at different steps
NS = (1, 2, 3, 5, 6)
GAMMAS = (0.99, 1.0, 0.0)
CAUSES = ("n", "cut", "avail", "agent_early", "wrap", "rewritten")


def stagger(E: int) -> np.ndarray:
    """Step counters at the start: episodes end at different steps in different envs."""
    return (np.arange(E) % MAX_STEPS).astype(np.int32)


def config(N: int):
    return make_config(N, max_steps=MAX_STEPS, individual=True)


def count_causes(ring: dict, cut: np.ndarray, index, n: int, gamma=0.99) -> dict:
    """How often each ending occurs among the windows of ``index`` (n >= 2: a window of one step ends by n only)."""
    R, S_ = ring["S"] * ring["E"], ring["S"]
    head = int(ring["state"][0])
    c = dict.fromkeys(CAUSES, 0)
    for i in np.asarray(index).tolist():
        if not 0 <= i < R:
            continue
        w = window_spec(ring, cut, i, n, gamma)
        if not ring["valid"][i].any():
            continue                                                     # (an empty slot)
        c[w["why"]] += 1
        c["agent_early"] += int(((w["span"] < w["m_env"]) & (w["done"] != 0)).any())
        c["wrap"] += int(w["wraps"] and w["m_env"] > 1)
        c["rewritten"] += int(head > S_ and w["m_env"] > 1)
    return c


def synthetic(N: int = 3):
    """A ring of S = 5 steps, E = 2 envs, written directly, with ``head`` = 7 (rewritten: steps 0 and 1 hold the newest
    records, step 1 is the newest), and the records at which each edge of the rule sits for n = 3.  Returns (ring, cut,
    where): ``where[name]`` is a record index."""
    S_, E_ = 5, 2
    ring = new_ring(S_, E_, N)
    cut = new_cut(S_, E_)
    rng = np.random.default_rng(11)
    R = S_ * E_
    ring["reward"][:] = rng.standard_normal((R, N))
    ring["actions"][:] = rng.integers(0, 5, (R, N), dtype=np.uint8)
    ring["valid"][:] = 4
    ring["masks_next"][:] = rng.integers(0, 16, (R, N), dtype=np.uint8) | 0x10
    ring["obs_c"][:] = rng.standard_normal((R, N, 4)).astype(np.float32)
    ring["next_c"][:] = rng.standard_normal((R, N, 4)).astype(np.float32)
    ring["state"][0] = 7                                                  # ring steps in age order: 2, 3, 4, 0, 1
    at = lambda p, e: p * E_ + e                                          # noqa: E731
    where = {}
    # env 0: no cut anywhere.  step 2 -> 2, 3, 4 (by n); step 3 -> 3, 4, 0 (by n, wraps); step 0 -> 0, 1 (availability);
    # step 1 -> 1 alone (the newest record)
    where["by_n"], where["wraps"], where["by_avail"], where["newest"] = at(2, 0), at(3, 0), at(0, 0), at(1, 0)
    # env 1: a cut at step 3; agent 0 terminates at step 4 (before the window of step 4 ends); agent 1 stops being live at
    # step 0 without terminating (dropped in the windows that reach it); a NaN reward at step 0 for agent 2
    cut[at(3, 1)] = 1
    where["by_cut"] = at(2, 1)                                            # 2, 3 | cut
    ring["done"][at(4, 1), 0] = 1
    ring["valid"][at(0, 1), 0] = 0
    ring["valid"][at(1, 1), 0] = 0
    where["agent_early"] = at(4, 1)                                       # env window 4, 0, 1; agent 0 stops at 4 with done
    ring["valid"][at(0, 1), 1] = 0                                        # not live at step 0, not terminated at step 4
    ring["valid"][at(1, 1), 1] = 0
    where["dropped"] = at(4, 1)                                           # the same record: agent 1's row is dropped
    ring["reward"][at(0, 1), 2] = np.nan
    where["nan_inside"] = at(4, 1)                                        # agent 2: the NaN is the window's second reward
    ring["reward"][at(2, 0), 2] = np.nan
    where["nan_just_beyond"] = at(0, 0)                                   # env 0, window 0, 1 (availability): slot_2 = step 2 holds a NaN for agent 2
    return ring, cut, where


def synthetic_states():
    """(head, what it shows) for the synthetic arrays: rewritten, empty, partly filled."""
    return ((7, "head > S"), (0, "head == 0"), (3, "head < S"), (5, "head == S"), (12, "head > 2 S"))
