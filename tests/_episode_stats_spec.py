"""CCX_EPISODE_STATS as include/ccx.h states it, restated in plain Python / NumPy on the CPU, plus a generator of adversarial
trajectories.  TEST INFRASTRUCTURE ONLY: what the episode-statistics kernels are compared with.

Written from the header paragraph, not from the kernels: one pass over the steps in order, one record list per update in
env-major order.  The running return is advanced with ONE IEEE f64 add per live agent and step (an elementwise NumPy add
over the selected (env, agent) entries: no reduction, nothing a library could reassociate); rewards of agents that are not
live are never touched.  Every comparison against this module is on bit patterns."""

from __future__ import annotations

import numpy as np

AF_LIVE = 0x04
EF_ALL_TERMINATED, EF_ALL_TRUNCATED, EF_RESET = 0x01, 0x02, 0x04
ACC_KEYS = ("ret", "live_steps", "steps", "closed", "finished", "last_ret", "last_live_steps", "last_steps", "last_end")
LOG_KEYS = ("env", "episode", "steps", "end", "ret", "live_steps")


class StatsSpec:
    """The accumulators of one handle and its finished-episode log (capacity 0 = no log)."""

    def __init__(self, E: int, N: int, log_capacity: int = 0, env_offset: int = 0):
        self.E, self.N, self.capacity, self.env_offset = E, N, int(log_capacity), int(env_offset)
        self.ret = np.zeros((E, N), np.float64)
        self.live_steps = np.zeros((E, N), np.int32)
        self.steps = np.zeros(E, np.int32)
        self.closed = np.zeros(E, np.uint8)
        self.finished = np.zeros(E, np.int32)
        self.last_ret = np.zeros((E, N), np.float64)
        self.last_live_steps = np.zeros((E, N), np.int32)
        self.last_steps = np.zeros(E, np.int32)
        self.last_end = np.zeros(E, np.uint8)
        self.records: list[tuple] = []       # stored records, in log order
        self.dropped = 0
        self.emitted = 0                     # records emitted since construction, stored or not

    def update(self, reward, agent_flags, env_flags) -> None:
        """The steps in order; within a step every env at once (the envs are independent, the operations elementwise: the
        same IEEE add per (env, agent) as a loop over the envs).  Records are collected with their (env, step) and put into
        the update's env-major order at the end."""
        reward = np.asarray(reward, np.float64)
        agent_flags = np.asarray(agent_flags, np.uint8)
        env_flags = np.asarray(env_flags, np.uint8)
        K = env_flags.shape[0]
        assert reward.shape == agent_flags.shape == (K, self.E, self.N) and env_flags.shape == (K, self.E)
        emitted = []                                              # (e, s, record)
        for s in range(K):
            ef = env_flags[s]
            open_ = self.closed == 0
            self.steps[open_] += 1
            add = open_[:, None] & ((agent_flags[s] & AF_LIVE) != 0)
            self.ret[add] = self.ret[add] + reward[s][add]        # one add per live agent of an open episode; nothing else is read
            self.live_steps[add] += 1
            fin = ((ef & (EF_ALL_TERMINATED | EF_ALL_TRUNCATED)) != 0) & open_
            if fin.any():
                self.emitted += int(fin.sum())
                if self.capacity:
                    for e in np.nonzero(fin)[0]:
                        emitted.append((int(e), s, (self.env_offset + int(e), int(self.finished[e]), int(self.steps[e]),
                                                    int(ef[e]) & 3, self.ret[e].copy(), self.live_steps[e].copy())))
                self.last_ret[fin] = self.ret[fin]
                self.last_live_steps[fin] = self.live_steps[fin]
                self.last_steps[fin] = self.steps[fin]
                self.last_end[fin] = ef[fin] & 3
                self.finished[fin] += 1
                self.closed[fin] = 1
            rst = (ef & EF_RESET) != 0
            if rst.any():
                self.ret[rst] = 0.0
                self.live_steps[rst] = 0
                self.steps[rst] = 0
                self.closed[rst] = 0
        emitted.sort(key=lambda r: (r[0], r[1]))                  # env-major: ascending e, then ascending s
        room = max(self.capacity - len(self.records), 0)
        self.records += [r[2] for r in emitted[:room]]
        self.dropped += len(emitted) - min(room, len(emitted))

    def reset(self, env_mask=None) -> None:
        m = np.ones(self.E, bool) if env_mask is None else np.asarray(env_mask) != 0
        self.ret[m] = 0.0
        self.live_steps[m] = 0
        self.steps[m] = 0
        self.closed[m] = 0

    def clear_log(self) -> None:
        self.records, self.dropped = [], 0

    def accumulators(self) -> dict:
        return {k: getattr(self, k) for k in ACC_KEYS}

    def log(self) -> dict:
        """The stored records as arrays, in log order."""
        R, N = len(self.records), self.N
        cols = list(zip(*self.records)) if R else [[]] * 6
        return dict(env=np.asarray(cols[0], np.int64).reshape(R), episode=np.asarray(cols[1], np.int32).reshape(R),
                    steps=np.asarray(cols[2], np.int32).reshape(R), end=np.asarray(cols[3], np.uint8).reshape(R),
                    ret=np.asarray(cols[4], np.float64).reshape(R, N), live_steps=np.asarray(cols[5], np.int32).reshape(R, N))


def bits(a) -> np.ndarray:
    """An array for exact comparison: f64 as its u64 bit patterns, everything else as it is."""
    a = np.ascontiguousarray(a)
    return a.view(np.uint64) if a.dtype == np.float64 else a


def sort_log(log: dict) -> dict:
    """Records ordered by (env, episode): the order that does not depend on how a trajectory was cut into updates."""
    order = np.lexsort((log["episode"], log["env"]))
    return {k: log[k][order] for k in LOG_KEYS}


# ----------------------------------------------------------------------------------------------------------------------
# adversarial trajectories (no env involved)
# ----------------------------------------------------------------------------------------------------------------------
N_LAYOUTS = 7


def make_trajectory(K: int, E: int, N: int, seed: int = 0):
    """(reward f64 [K, E, N], agent_flags u8 [K, E, N], env_flags u8 [K, E]).

    Rewards by column (e * N + a) % 4: 0 the pattern 1e16, 1.0, -1e16 step after step (any reassociation of the sum changes
    its bits), 1 values from {-0.0, +0.0, 0.1, -0.3, 1e-300} (sign of zero, inexact adds, subnormal range), 2 and 3 random
    normals of mixed magnitude.  Where an agent is NOT live the reward is NaN: one read of it into a sum shows.
    agent_flags: LIVE set with probability 0.8 under random other bits.
    env_flags by e % 7:
      0  never finishes (and never resets);
      1  finishes on step 0 and on step K - 1, each with RESET;
      2  an episode of length 1 on every step: finish + RESET throughout;
      3  finishes at K // 4 without RESET, keeps its flags raised, RESET alone many steps later at 3K // 4: no second record;
      4  random raises (terminated, truncated or both), RESET on half of them, a few RESETs without a raise;
      5  finishes without RESET and is never restarted: every later raise is latched away;
      6  alternates raised / not raised without any RESET: one record."""
    rng = np.random.default_rng(seed)
    col = (np.arange(E)[:, None] * N + np.arange(N)[None, :]) % 4
    s = np.arange(K)[:, None, None]
    pattern = np.array([1e16, 1.0, -1e16])[s % 3] + np.zeros((K, E, N))
    small = rng.choice(np.array([-0.0, 0.0, 0.1, -0.3, 1e-300]), size=(K, E, N))
    normal = rng.standard_normal((K, E, N)) * 10.0 ** rng.integers(-3, 4, size=(K, E, N))
    reward = np.where(col == 0, pattern, np.where(col == 1, small, normal))
    live = rng.random((K, E, N)) < 0.8
    agent_flags = (rng.integers(0, 256, size=(K, E, N)) & ~AF_LIVE | np.where(live, AF_LIVE, 0)).astype(np.uint8)
    reward = np.where(live, reward, np.nan)
    ef = np.zeros((K, E), np.uint8)
    for e in range(E):
        kind = e % N_LAYOUTS
        if kind == 1:
            ef[0, e] = EF_ALL_TERMINATED | EF_RESET
            ef[K - 1, e] |= EF_ALL_TRUNCATED | EF_RESET
        elif kind == 2:
            ef[:, e] = rng.choice(np.array([1, 2, 3], np.uint8), size=K) | EF_RESET
        elif kind == 3:
            ef[K // 4:3 * K // 4, e] = EF_ALL_TERMINATED
            ef[3 * K // 4, e] = EF_RESET
        elif kind == 4:
            raised = rng.random(K) < 0.15
            ef[:, e] = np.where(raised, rng.integers(1, 4, size=K), 0)
            ef[:, e] |= np.where(raised & (rng.random(K) < 0.5), EF_RESET, 0).astype(np.uint8)
            ef[:, e] |= np.where(~raised & (rng.random(K) < 0.05), EF_RESET, 0).astype(np.uint8)
        elif kind == 5:
            ef[K // 3:, e] = EF_ALL_TRUNCATED
            ef[K // 3::2, e] |= EF_ALL_TERMINATED
        elif kind == 6:
            ef[K // 5::2, e] = EF_ALL_TERMINATED
    return np.ascontiguousarray(reward), agent_flags, ef
