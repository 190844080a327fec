"""Far shards and late episodes: the cases, the wrong-width models of the reset-pool cursor and the oracle's reference runs
that tests/test_far_shard_spec.py (CPU) and tests/test_gpu_far_shards.py share.  TEST INFRASTRUCTURE ONLY.

The cursor of include/ccx.h (ccx_set_reset_pool) is ``entry (g + j * stride) mod P``, ``g = env_offset + e``, ``stride =
total_envs mod P, or 1``.  ``env_offset`` and ``total_envs`` are 64-bit in the ABI; the kernels narrow them by hand.  The
spec is ``_split_step_spec.pool_cursor`` (Python integers of unlimited width).  Every case below is small (E <= 130, a pool
of at most 1.6 MB); what is large are the NUMBERS the cursor and the RNG key are computed from."""

from __future__ import annotations

import functools
from dataclasses import dataclass

import numpy as np
from _reset_obs_spec import SENTINEL, compact_of, make_config, next_mode
from _split_step_spec import pool_cursor

N, MAX_STEPS, K = 8, 5, 38         # C1's geometry with 8 agents, episodes of at most 5 steps: 7+ restarts of every env in K steps
RESTARTS = K // MAX_STEPS          # restarts of an env the adequacy condition looks at (a run has at least that many)
POOL_SEED = 7
P_BIG = 100_003                    # prime, above 92 682 = floor(sqrt(2^32 - 1)): a product of two residues can pass 2^32
M32, M64 = (1 << 32) - 1, (1 << 64) - 1

# total_envs >= 2^32 in the three forms of stride (P = P_BIG)
T_STRIDE_70001 = (1 << 33) + 93_100        # = 70 001 mod P_BIG: a stride above 65 536
T_STRIDE_99991 = (1 << 41) + 13_155        # = 99 991 mod P_BIG
T_DIVIDES = P_BIG * 50_000                 # P divides total_envs: the stride is 1
T_STRIDE_PM1 = P_BIG * 50_000 - 1          # the stride is P - 1
# start episodes (set_state(episode=...)); an env adds e % 5 and at most K restarts: no counter passes INT32_MAX
EP_LATE = (1 << 31) - 300
EP_ABOVE_2_16 = (1 << 16) + 7              # its residue mod P_BIG, 65 543, times a stride of P - 1 is 6.5e9 > 2^32
EP_BIG_RESIDUE = 9_000 * P_BIG + 95_000    # residue 95 000: times 99 991 (or 70 001) it exceeds 2^32


@dataclass(frozen=True)
class FarCase:
    name: str
    env_offset: int
    total_envs: int
    P: int
    episode0: int
    E: int

    @property
    def stride(self) -> int:
        return self.total_envs % self.P or 1

    def episodes(self) -> np.ndarray:
        """i32 [E]: the episode counters the run starts from (staggered, so that envs of one tile sit in different episodes)."""
        return (self.episode0 + np.arange(self.E) % 5).astype(np.int32)

    def step_counts(self) -> np.ndarray:
        """i32 [E]: staggered over the episode length by GLOBAL index (what the call-path harness sets)."""
        return ((self.env_offset + np.arange(self.E)) % MAX_STEPS).astype(np.int32)


CASES = {c.name: c for c in (
    # crosses 2^31 inside the batch (env 30 is global env 2^31)
    FarCase("cross31", (1 << 31) - 30, T_STRIDE_70001, P_BIG, EP_LATE, 67),
    # crosses 2^32 inside the batch AND inside one tile: env 29 is global env 2^32, and 29 is no multiple of a tile's 2..64 envs
    FarCase("cross32", (1 << 32) - 29, T_STRIDE_PM1, P_BIG, EP_ABOVE_2_16, 130),
    FarCase("far40", (1 << 40) + 12_345, T_STRIDE_99991, P_BIG, EP_BIG_RESIDUE, 67),
    # two shards whose boundary is exactly 2^32: the last env of the first is 2^32 - 1, env 0 of the second is 2^32
    FarCase("edge32_below", (1 << 32) - 67, T_DIVIDES, P_BIG, EP_BIG_RESIDUE, 67),
    FarCase("edge32_above", 1 << 32, T_DIVIDES, P_BIG, EP_LATE, 130),
    FarCase("pool_of_1", (1 << 40) + 12_345, T_STRIDE_99991, 1, EP_ABOVE_2_16, 67),
    FarCase("pool_of_37", (1 << 32) - 29, T_STRIDE_70001, 37, EP_LATE, 67),
)}


# ---------------------------------------------------------------------------------------------------------------------
# wrong-width models of the cursor: what a copy computes that narrows ONE quantity.  (A fifth candidate, the rollout
# kernel's incremental walk `idx += stride; if (idx >= P) idx -= P` overflowing its u32, needs idx + stride >= 2^32 with
# both below P, i.e. P > 2^31: ccx_set_reset_pool refuses pools of 2^31 entries and more, so it is not reachable and has no
# model here.)
# ---------------------------------------------------------------------------------------------------------------------
def model_u32_product(env_offset, total_envs, P, env, episode):
    """(ep % P) * stride taken mod 2^32."""
    stride = total_envs % P or 1
    return ((env_offset + env) % P + (((episode % P) * stride) & M32)) % P


def model_u32_global(env_offset, total_envs, P, env, episode):
    """env_offset + e taken mod 2^32."""
    return pool_cursor((env_offset + env) & M32, total_envs, P, 0, episode)


def model_i32_global(env_offset, total_envs, P, env, episode):
    """env_offset + e taken through a signed 32-bit int, then widened to u64 the way the kernels widen it (sign extension)."""
    g = (env_offset + env) & M32
    g = (g - (1 << 32) if g >> 31 else g) & M64
    return pool_cursor(g, total_envs, P, 0, episode)


def model_u32_total(env_offset, total_envs, P, env, episode):
    """total_envs taken mod 2^32 before `% P`."""
    return pool_cursor(env_offset, total_envs & M32, P, env, episode)


MODELS = dict(u32_product=model_u32_product, u32_global=model_u32_global, i32_global=model_i32_global,
              u32_total=model_u32_total)


def cursor_pairs(case: FarCase):
    """The (env, episode) pairs of a case the adequacy condition counts: the start and RESTARTS restarts of every env."""
    ep = case.episodes()
    return [(e, int(ep[e]) + r) for e in range(case.E) for r in range(RESTARTS + 1)]


# ---------------------------------------------------------------------------------------------------------------------
# config, pool, inputs, and the oracle's runs
# ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def config():
    return make_config(N, MAX_STEPS)


@functools.lru_cache(maxsize=None)
def params():
    from collectivecrossing_amd.params import lower_config
    return lower_config(config())


@functools.lru_cache(maxsize=None)
def pool(P: int) -> np.ndarray:
    """u8 [P, N, 2]: the placements of reset(seed=POOL_SEED + p), from the oracle's C restatement of numpy's stream (the
    Python loop of `build_reset_pool` takes ~12 s for 100 003 seeds; test_far_shard_spec.py checks the two agree on a prefix,
    the GPU tests that `make_reset_pool` builds the same bytes).  Read-only: shared by every test of a session."""
    from oracle import oracle
    a = oracle.seeded_placements(params(), np.arange(POOL_SEED, POOL_SEED + P, dtype=np.uint64))
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def inputs(name: str):
    """(actions u8 [K, E, N], orders u8 [K, E, N]) of a case, read-only."""
    case = CASES[name]
    rng = np.random.default_rng(sum(map(ord, name)))
    acts = rng.integers(0, 5, size=(K, case.E, N), dtype=np.uint8)
    orders = np.argsort(rng.random((K, case.E, N)), axis=-1).astype(np.uint8)
    acts.setflags(write=False)
    orders.setflags(write=False)
    return acts, orders


def new_oracle(case: FarCase):
    """An OracleBatch of the case in its start state: episode counters set, placed from the pool, step counters staggered."""
    from oracle import oracle
    ob = oracle.OracleBatch(params(), case.E, case.env_offset, case.total_envs)
    ob.set_reset_pool(pool(case.P))
    ob.set_state(episode=case.episodes())
    ob.reset_from_pool()
    ob.set_state(step_count=case.step_counts())
    return ob


@dataclass
class Reference:
    """What one auto-reset run of K steps leaves, from the oracle: the NEXT-mode arrays (tests/_reset_obs_spec.next_mode on
    the oracle's TERMINAL-mode trajectory; side buffers start as SENTINEL bytes), the trajectory, the state and the counters."""
    actions: np.ndarray            # u8 [K, E, N]: the actions the steps took (the policy's, the merged ones, or the tensor)
    obs: np.ndarray
    obs_compact: np.ndarray
    final_obs: np.ndarray
    final_compact: np.ndarray
    reward: np.ndarray
    agent_flags: np.ndarray
    env_flags: np.ndarray
    state: dict
    counters: dict

    def freeze(self):
        for v in list(self.__dict__.values()) + list(self.state.values()):
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        return self


def _reference(case, ob, acts, obs, rew, af, ef, ep_before):
    nb = params().num_boarding
    cmp_ = compact_of(obs, af, nb)
    fo = np.frombuffer(bytes([SENTINEL]) * obs.nbytes, np.float32).reshape(obs.shape)
    fc = np.frombuffer(bytes([SENTINEL]) * cmp_.nbytes, np.float32).reshape(cmp_.shape)
    n_obs, n_cmp, f_obs, f_cmp, ep_after = next_mode(obs, cmp_, ef, pool(case.P), case.env_offset, case.total_envs, ep_before,
                                                     params(), fo, fc)
    state = {k: getattr(ob, k).copy() for k in ("x", "y", "active", "terminated", "truncated", "step_count", "episode")}
    assert np.array_equal(state["episode"], ep_after)
    return Reference(acts, n_obs, n_cmp, f_obs, f_cmp, rew, af, ef, state, ob.counters.as_dict()).freeze()


@functools.lru_cache(maxsize=None)
def tensor_reference(name: str, with_order: bool = False) -> Reference:
    """The case driven by its action tensor (and its move orders)."""
    case = CASES[name]
    acts, orders = inputs(name)
    ob = new_oracle(case)
    ep0 = ob.episode.copy()
    obs, rew, af, ef = ob.rollout(acts, orders if with_order else None, auto_reset=True)
    return _reference(case, ob, acts, obs, rew, af, ef, ep0)


RNG_SEED, EPSILON = 2024, 0.3


@functools.lru_cache(maxsize=None)
def policy_reference(name: str, policy: str, epsilon: float = EPSILON) -> Reference:
    """The case driven by the scripted policy with the counter-based exploration draws (keyed by the low word of the
    global env index, include/ccx.h: ccx_set_policy_epsilon)."""
    from oracle import oracle
    case = CASES[name]
    ob = new_oracle(case)
    ep0 = ob.episode.copy()
    try:
        oracle.OracleBatch.set_rng_seed(RNG_SEED)
        oracle.OracleBatch.set_policy_epsilon(epsilon)
        acts, obs, rew, af, ef = ob.rollout_greedy(K, auto_reset=True, policy=policy)
    finally:
        oracle.OracleBatch.set_policy_epsilon(0.0)
    return _reference(case, ob, acts, obs, rew, af, ef, ep0)


@functools.lru_cache(maxsize=None)
def mixed_reference(name: str, policy: str, epsilon: float = EPSILON) -> Reference:
    """The case with its exiting slots scripted: per step the oracle's policy actions of the state before the step (with
    the exploration draws), merged under the slot mask with the tensor, then the ordinary step (ccx_rollout_mixed)."""
    from oracle import oracle
    case = CASES[name]
    acts, _ = inputs(name)
    sel = np.arange(N) >= params().num_boarding
    ob = new_oracle(case)
    ep0 = ob.episode.copy()
    merged, parts = np.empty_like(acts), []
    try:
        oracle.OracleBatch.set_rng_seed(RNG_SEED)
        oracle.OracleBatch.set_policy_epsilon(epsilon)
        for s in range(K):
            pa = ob.policy_actions(policy, with_epsilon=True)
            merged[s] = np.where(sel[None, :], pa, acts[s])
            parts.append(ob.rollout(merged[s][None], auto_reset=True))
    finally:
        oracle.OracleBatch.set_policy_epsilon(0.0)
    obs, rew, af, ef = (np.concatenate([p[i] for p in parts], 0) for i in range(4))
    return _reference(case, ob, merged, obs, rew, af, ef, ep0)
