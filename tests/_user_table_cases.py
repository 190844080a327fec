"""Position-only user tables (ccx_set_reward_table / ccx_set_terminated_table) under every feature that reads the bits they
change: seeded table families, the cases the CPU adequacy test (tests/test_user_tables_spec.py) and the GPU test
(tests/test_gpu_user_tables.py) share, and the oracle's trajectory of a case.

NumPy only: nothing here touches a GPU or libccx.  The CPU oracle is handed in by the caller (``oracle_mod``), as in
tests/_reset_obs_spec.py, whose configs, pool size and NEXT-mode spec are reused."""

from __future__ import annotations

import numpy as np
from _fixtures import config_from_dict
from _reset_obs_spec import POOL_SIZE, SENTINEL, compact_of, make_config, next_mode

AF_TERMINATED, AF_TRUNCATED, AF_LIVE, AF_ACTIVE = 0x01, 0x02, 0x04, 0x40
EF_ALL_TERMINATED, EF_ALL_TRUNCATED, EF_RESET = 0x01, 0x02, 0x04
FAMILIES = ("sparse", "no_term_at_destination", "dense", "reward_only", "term_only")
SUBNORMAL, HUGE = 5e-324, 1e300     # rewards are copied, never computed: both must come back bit for bit
RNG_SEED = 2024                     # counter-based exploration draws (mixed control with epsilon > 0)
STATE_KEYS = ("x", "y", "active", "terminated", "truncated", "step_count", "episode")

# Two grids with the same agent count on both sides of a boundary of the CPU planner (csrc/ccx_plan.hip, through the
# ccxi_plan binding of tests/golden/gen_shape_plan_golden.py): with reward_table = 1 the smaller keeps step_ok = 1, the
# larger falls back to the rollout kernel (step_ok = 0), and without the table both take the step kernel.
# tests/test_user_tables_spec.py asks the planner again, so a change of its rules that moves the boundary shows there.
PLANNER_PAIR = ((56, 40), (64, 48))
PLANNER_PAIR_N = 8
SWITCHES = ("sparse", None, "dense", "reward_only")      # the tables of section f, each for one [1, 5] pair of launches
# A handle on which a reward table fits with the default launch shape and is refused after set_launch_shape(0, 2): two sim
# waves per workgroup double the per-tile LDS next to the table (the planner's lds_bytes crosses 150 KB).  From the planner
# too; tests/test_user_tables_spec.py asks it again.
DROP_GRID, DROP_N, DROP_WAVES = (84, 62), 33, 2


def grid_config(width, height, N, max_steps):
    """A valid env of a given grid: the tram spans most of the width, the door sits in its middle."""
    nb = {1: 1, 3: 2, 5: 3, 8: 5}.get(N, N // 2)
    length = width - 4
    return config_from_dict(dict(
        width=width, height=height, division_y=height // 2, tram_door_left=length // 2 - 2, tram_door_right=length // 2 + 2,
        tram_length=length, boarding_destination_area_y=height, exiting_destination_area_y=0, num_boarding_agents=nb,
        num_exiting_agents=N - nb, truncated_config=dict(truncated_function="max_steps", max_steps=max_steps),
        terminated_config=dict(terminated_function="individual_at_destination")))


def make_tables(family, config, seed=0):
    """``((reward_boarding, reward_exiting) | None, (term_boarding, term_exiting) | None)`` of a family: f64 / bool
    ``[height + 1, width + 1]``, the two agent types drawn separately."""
    assert family in FAMILIES, family
    W, H = config.width, config.height
    shape = (H + 1, W + 1)
    rng = np.random.default_rng([seed, FAMILIES.index(family), W, H])
    reward = term = None
    if family != "term_only":
        reward = []
        for t in range(2):
            tab = rng.normal(size=shape)
            flat = tab.reshape(-1)
            zeros = rng.permutation(flat.size)[:max(8, flat.size // 10)]
            flat[zeros[0::2]] = -0.0
            flat[zeros[1::2]] = 0.0
            # on the row the agents cross on their way (the division line and the one next to it), around the middle
            y = H // 2 + (0 if t == 0 else 1)
            tab[y, W // 2] = SUBNORMAL
            tab[y, W // 2 + 1] = HUGE
            tab[y, W // 2 - 1] = -0.0
            reward.append(tab)
        reward = tuple(reward)
    if family != "reward_only":
        density = 0.7 if family == "dense" else 0.15
        term = tuple(rng.random(shape) < density for _ in range(2))
        if family == "no_term_at_destination":       # arrived agents deactivate and stay not terminated
            for tab in term:
                tab[config.boarding_destination_area_y, :] = False
                tab[config.exiting_destination_area_y, :] = False
    return reward, term


# name -> what differs from the defaults of TableCase.  `section` = the part of tests/test_gpu_user_tables.py that runs it.
def _cases():
    c = {}
    # (a) fused one-step extras: table families x agent counts (odd counts, the PAIR path, a padded lane group)
    for family, counts in (("sparse", (1, 5, 8, 33)), ("no_term_at_destination", (5, 8)), ("dense", (1, 3)),
                           ("reward_only", (5, 33)), ("term_only", (8, 33))):
        for n in counts:
            c[f"a_{family}_n{n}"] = dict(section="a", family=family, N=n, chunks=[1] * 14)
    # (b) the same through the unfused kernels
    c["b_unfused_sparse_n8"] = dict(section="b", family="sparse", N=8, chunks=[1] * 8, unfused=True)
    c["b_unfused_dense_n3"] = dict(section="b", family="dense", N=3, chunks=[1] * 8, unfused=True)
    c["b_order_sparse_n8"] = dict(section="b", family="sparse", N=8, chunks=[1, 1, 4, 1], order=True)
    c["b_order_no_term_n5"] = dict(section="b", family="no_term_at_destination", N=5, chunks=[1, 16], order=True)
    c["b_k16_sparse_n5"] = dict(section="b", family="sparse", N=5, chunks=[16, 16])
    c["b_k16_dense_n3"] = dict(section="b", family="dense", N=3, chunks=[16, 3])
    c["b_k40_sparse_n33"] = dict(section="b", family="sparse", N=33, chunks=[40])
    c["b_k40_no_term_n8"] = dict(section="b", family="no_term_at_destination", N=8, chunks=[40, 16])
    c["b_k40_dense_n1"] = dict(section="b", family="dense", N=1, chunks=[40, 40])
    c["b_big_term_only_n3"] = dict(section="b", family="term_only", N=3, E=5, big=True, chunks=[1, 1, 16], max_steps=6,
                                   crowded=True, input_seed=1)
    c["b_shard_sparse_n5"] = dict(section="b", family="sparse", N=5, chunks=[1, 16, 40], env_offset=1000, total_envs=5000)
    # (c) scripted and mixed control
    for family, n in (("no_term_at_destination", 8), ("no_term_at_destination", 5), ("sparse", 8)):
        short = "no_term" if family.startswith("no_term") else family
        for policy in ("greedy", "waiting"):
            for eps in (0.0, 0.3):
                for drive in ("greedy", "mixed", "mixed_unfused"):
                    if (family, n) != ("no_term_at_destination", 8) and (policy == "waiting") != (eps > 0):
                        continue                    # the full matrix on the important family, the diagonal elsewhere
                    c[f"c_{drive}_{policy}_eps{int(eps * 10)}_{short}_n{n}"] = dict(
                        section="c", family=family, N=n, chunks=[1, 16, 23], drive="greedy" if drive == "greedy" else "mixed",
                        unfused=drive == "mixed_unfused", policy=policy, eps=eps, max_steps=20)
    # (d) episode statistics: f64 sums of arbitrary normals, whole and cut into launches of 7 steps
    for family, n in (("sparse", 5), ("dense", 3)):
        for cut in (0, 7):
            c[f"d_{family}_n{n}_cut{cut}"] = dict(section="d", family=family, N=n, chunks=[40, 23], cut=cut, log=4096, input_seed=1 + cut)
    # (e) the three-way comparison of tests/test_gpu_call_paths.py (its E, K, MAX_STEPS and input seeds) with tables
    for n in (5, 8):
        for i, drive in ((0, "tensor"), (1, "order"), (3, "mixed"), (5, "mt")):
            c[f"e_{drive}_n{n}"] = dict(section="e", family="sparse", N=n, chunks=[38], max_steps=5, input_seed=1000 * n + i,
                                        order=drive == "order", drive={"mt": "greedy", "order": "tensor"}.get(drive, drive),
                                        eps=0.3 if drive == "mt" else 0.0)
    # (f) tables switched on a live handle, on both sides of the planner pair; a refused reward table on 100 x 100
    for w, h in PLANNER_PAIR:
        c[f"f_switch_{w}x{h}"] = dict(section="f", family="sparse", N=PLANNER_PAIR_N, grid=(w, h), max_steps=6,
                                      chunks=[1, 5] * len(SWITCHES), switches=SWITCHES)
    c["f_refused_big_n3"] = dict(section="f", family="term_only", N=3, E=5, big=True, chunks=[1, 16], max_steps=6, crowded=True,
                                 input_seed=1)
    c["f_dropped_84x62_n33"] = dict(section="f", family="sparse", N=DROP_N, grid=DROP_GRID, max_steps=6, chunks=[1, 5] * 2,
                                    switches=("sparse", "reward_dropped"))
    return c


CASES = _cases()


def names(section):
    return [n for n, c in CASES.items() if c["section"] == section]


class TableCase:
    """One case on the CPU: config, pool, staggered start state, tables and the inputs of every launch."""

    def __init__(self, name):
        from collectivecrossing_amd.params import lower_config
        from collectivecrossing_amd.reset import build_reset_pool
        c = dict(E=67, max_steps=12, big=False, order=False, env_offset=0, total_envs=None, drive="tensor", unfused=False,
                 policy="greedy", eps=0.0, cut=0, log=0, grid=None, input_seed=None, crowded=False, switches=None, section="")
        given = CASES[name]
        unknown = set(given) - set(c) - {"family", "N", "chunks"}
        assert not unknown, (name, unknown)
        c.update(given)
        for key, value in c.items():
            setattr(self, key, value)
        self.name = name
        self.total_envs = self.total_envs or self.E
        self.config = (grid_config(*self.grid, self.N, self.max_steps) if self.grid
                       else make_config(self.N, self.max_steps, self.big))
        self.params = lower_config(self.config)
        self.pool = build_reset_pool(self.config, 7, POOL_SIZE)
        if self.crowded:
            # A grid on which random placements never meet: the boarding agents start side by side, so that one that
            # terminates stands in its neighbour's way (the pool is the caller's: any in-grid placement is a valid entry).
            for j in range(1, self.params.num_boarding):
                x0 = self.pool[:, 0, 0].astype(np.int32)
                self.pool[:, j, 0] = np.where(x0 + j <= self.config.width, x0 + j, x0 - j).astype(np.uint8)
                self.pool[:, j, 1] = self.pool[:, 0, 1]
            cells = self.pool[:, :, 0].astype(np.int32) * 256 + self.pool[:, :, 1]
            assert all(len(set(row)) == self.N for row in cells.tolist()), "two agents of a pool entry share a cell"
        self.tables = make_tables(self.family, self.config)
        E, N = self.E, self.N
        rng = np.random.default_rng(sum(map(ord, self.name)) if self.input_seed is None else self.input_seed)
        # step counters staggered over the episode length: restarts fall on first, middle and last steps of a launch
        self.step_count0 = ((self.env_offset + np.arange(E)) % self.max_steps).astype(np.int32)
        self.actions = [rng.integers(0, 5, size=(k, E, N), dtype=np.uint8) for k in self.chunks]
        drawn = [np.argsort(rng.random((k, E, N)), axis=-1).astype(np.uint8) for k in self.chunks]
        self.drawn_orders = drawn
        self.orders = drawn if self.order else [None] * len(self.chunks)
        self.mt_seeds = (np.arange(E) + 11).astype(np.uint32)
        self.scripted = np.arange(N) >= self.params.num_boarding          # mixed control: the exiting slots

    def tables_of_launch(self, q):
        """The tables launch q runs under: the case's own, or those of its `switches` entry (one per pair of launches)."""
        if not self.switches:
            return self.tables
        family = self.switches[q // 2]
        if family == "reward_dropped":                      # the case's terminated table stays, the built-in reward is back
            return None, self.tables[1]
        return (None, None) if family is None else make_tables(family, self.config)

    def run_oracle(self, oracle_mod):
        if self.switches:
            ob = new_oracle(oracle_mod, self.params, self.E, self.pool, self.step_count0, self.tables)
            out = []
            for q, k in enumerate(self.chunks):
                ob.set_user_tables(*self.tables_of_launch(q))
                out.append(oracle_launch(ob, "tensor", k, self.actions[q]))
            return out
        return oracle_trajectory(oracle_mod, self.params, self.E, self.pool, self.step_count0, self.tables, self.drive,
                                 self.chunks, self.actions, self.orders, self.policy, self.eps, self.mt_seeds, self.scripted,
                                 self.env_offset, self.total_envs)

    def spec(self, chunk):
        """NEXT-mode arrays (obs, compact, final_obs, final_compact, episode after) of a launch from its TERMINAL-mode
        trajectory; the side buffers start as SENTINEL bytes."""
        obs = chunk["obs"]
        compact = compact_of(obs, chunk["agent_flags"], self.params.num_boarding)
        fo = np.frombuffer(bytes([SENTINEL]) * obs.nbytes, np.float32).reshape(obs.shape)
        fc = np.frombuffer(bytes([SENTINEL]) * compact.nbytes, np.float32).reshape(compact.shape)
        return next_mode(obs, compact, chunk["env_flags"], self.pool, self.env_offset, self.total_envs,
                         chunk["episode_before"], self.params, fo, fc)


def new_oracle(oracle_mod, params, E, pool, step_count0, tables, env_offset=0, total_envs=None):
    ob = oracle_mod.OracleBatch(params, E, env_offset, total_envs or E)
    ob.set_reset_pool(pool)
    ob.reset_from_pool()
    ob.set_state(step_count=step_count0)
    ob.set_user_tables(*tables)
    return ob


def oracle_launch(ob, drive, k, actions=None, order=None, policy="greedy", scripted=None, with_epsilon=False):
    """One auto-reset launch of k steps on the oracle -> its TERMINAL-mode trajectory, the actions the steps took, the
    episode counters before and the state and counters behind it.  ``mixed``: per step the oracle's policy actions of the
    state before the step in the scripted slots, the tensor's bytes elsewhere, then the ordinary step."""
    ep0 = ob.episode.copy()
    if drive == "greedy":
        acts, obs, rew, af, ef = ob.rollout_greedy(k, auto_reset=True, policy=policy)
    elif drive == "mixed":
        acts, parts = np.empty_like(actions), []
        for s in range(k):
            pa = ob.policy_actions(policy, with_epsilon=with_epsilon)
            acts[s] = np.where(scripted[None, :], pa, actions[s])
            parts.append(ob.rollout(acts[s][None], None if order is None else order[s][None], auto_reset=True))
        obs, rew, af, ef = (np.concatenate([p[i] for p in parts], 0) for i in range(4))
    else:
        acts = actions
        obs, rew, af, ef = ob.rollout(actions, order, auto_reset=True)
    return dict(actions=acts, obs=obs, reward=rew, agent_flags=af, env_flags=ef, episode_before=ep0,
                state={f: getattr(ob, f).copy() for f in STATE_KEYS}, counters=ob.counters.as_dict())


def oracle_trajectory(oracle_mod, params, E, pool, step_count0, tables, drive, chunks, actions, orders=None, policy="greedy",
                      eps=0.0, mt_seeds=None, scripted=None, env_offset=0, total_envs=None):
    """The launches of a case on the oracle, one dict per launch (oracle_launch).  Exploration: the scripted policy alone
    draws from the per-env MT19937 streams, mixed control from the counter-based draws (the library refuses MT19937 there);
    both settings are process-wide in the oracle and are put back."""
    ob = new_oracle(oracle_mod, params, E, pool, step_count0, tables, env_offset, total_envs)
    out = []
    try:
        if drive == "greedy" and eps > 0:
            ob.set_policy_stream_mt19937(mt_seeds, eps)
        if drive == "mixed":
            oracle_mod.OracleBatch.set_rng_seed(RNG_SEED)
            oracle_mod.OracleBatch.set_policy_epsilon(eps)
        for q, k in enumerate(chunks):
            out.append(oracle_launch(ob, drive, k, None if actions is None else actions[q],
                                     None if orders is None else orders[q], policy, scripted, eps > 0))
    finally:
        oracle_mod.OracleBatch.set_policy_epsilon(0.0)
        ob.set_policy_stream_mt19937(None, 0.0)
        ob.policy_actions(policy, with_epsilon=True)        # (rebinds the process-wide stream pointer: none)
    return out


# ---------------------------------------------------------------------------------------------------- state predicates
def blocked_by_terminated(oracle_mod, params, st):
    """bool [E, N]: live, active agents with a move that only an ACTIVE TERMINATED agent's cell forbids."""
    from _action_masks import spec_masks
    ghost = (st["active"] != 0) & (st["terminated"] != 0)
    with_all = spec_masks(oracle_mod, params, st["x"], st["y"], st["active"], st["terminated"], st["truncated"])
    without = spec_masks(oracle_mod, params, st["x"], st["y"], np.where(ghost, 0, st["active"]), st["terminated"], st["truncated"])
    live = (st["terminated"] == 0) & (st["truncated"] == 0) & (st["active"] != 0)
    return live & (with_all != without)


def terminated_with_a_free_neighbour(oracle_mod, params, st):
    """bool [E, N]: active terminated agents whose geometry-and-occupancy mask (their done bits ignored) has a move."""
    from _action_masks import WAIT_ONLY, spec_masks
    zero = np.zeros_like(st["terminated"])
    geo = spec_masks(oracle_mod, params, st["x"], st["y"], st["active"], zero, zero)
    return (st["active"] != 0) & (st["terminated"] != 0) & (geo != WAIT_ONLY)
