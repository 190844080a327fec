"""The three implementations of one env-step hand out the same bits for the same trajectory: the rollout kernel (one launch
of K = 20), the short-launch kernel (20 launches of K = 1 with auto-reset) and the split step (20 x begin + finish with no
caller arrays).  They share the step rule of csrc/ccx_step_rule.h; this is the test that they still agree after a change to
it.  E = 5 envs on the smallest grid of the split-step cases leave a ragged last wave; N = 3 is odd (8-byte row units, a
partial lane group), N = 8 fills its group.

The actions are recorded ONCE on the CPU (the oracle steps the same state; the greedy policy drives envs 0 and 3, fixed-seed
random bytes the rest) and replayed on all three paths.  The reset pool of 3 entries places every agent one or two rows
from its destination and max_steps is 6, so that inside 20 steps greedy envs arrive (ALL_TERMINATED) and the others
truncate (ALL_TRUNCATED), both restart (RESET), and env 4 starts with an agent that was truncated earlier (a non-live
agent-step under either termination mode).  `test_recorded_trajectories_reach_every_event` holds that on the CPU."""

import _split_step_cases as cases
import _split_step_spec as spec
import numpy as np
import pytest

from collectivecrossing_amd._abi import REWARD_MODES, TERMINATED_MODES
from collectivecrossing_amd.params import lower_config

GRID = min(cases.GRIDS)
E, K, POOL, MAX_STEPS, SEED = 5, 20, 3, 6, 2024
GREEDY_ENVS = [0, 3]
PARAMS = [(n, r, t) for n in (3, 8) for r in REWARD_MODES for t in TERMINATED_MODES]
IDS = [f"N{n}-{r}-{t}" for n, r, t in PARAMS]


def near_destination_pool(rng, p, N):
    """u8 [POOL, N, 2]: boarding agents one or two rows below their destination row, exiting agents one or two above theirs."""
    cells = cases.legal_cells(p)
    rows_b = cells[(cells[:, 1] >= p.boarding_dest_y - 2) & (cells[:, 1] < p.boarding_dest_y)]
    rows_e = cells[(cells[:, 1] > p.exiting_dest_y) & (cells[:, 1] <= p.exiting_dest_y + 2)]
    pool = np.empty((POOL, N, 2), np.uint8)
    for k in range(POOL):
        pool[k, :p.num_boarding] = rows_b[rng.permutation(len(rows_b))[:p.num_boarding]]
        pool[k, p.num_boarding:] = rows_e[rng.permutation(len(rows_e))[:N - p.num_boarding]]
    return pool


def record(oracle, N, reward, terminated):
    """(config, pool, start state, actions u8 [K, E, N], the oracle's agent flags [K, E, N] and env flags [K, E])."""
    cfg = cases.make_config(*GRID, N, max_steps=MAX_STEPS, reward=reward, terminated=terminated)
    try:
        p = lower_config(cfg)
    except ValueError as err:
        pytest.skip(f"the config rejects reward '{reward}' with termination '{terminated}': {err}")
    rng = np.random.default_rng(SEED + N)
    pool = near_destination_pool(rng, p, N)
    ob = oracle.OracleBatch(p, E)
    ob.set_reset_pool(pool)
    ob.reset_from_pool()
    truncated = np.zeros((E, N), np.uint8)
    truncated[4, 0] = 1                                          # truncated in an earlier step: never live in this episode
    ob.set_state(truncated=truncated)
    start = {k: getattr(ob, k).copy() for k in spec.STATE_KEYS}
    random_bytes = rng.integers(0, 5, size=(K, E, N), dtype=np.uint8)
    actions, af, ef = np.empty((K, E, N), np.uint8), np.empty((K, E, N), np.uint8), np.empty((K, E), np.uint8)
    for s in range(K):
        actions[s] = random_bytes[s]
        actions[s, GREEDY_ENVS] = ob.greedy_actions()[GREEDY_ENVS]
        _, _, af[s:s + 1], ef[s:s + 1] = ob.rollout(actions[s:s + 1], auto_reset=True, want_obs=False)
    return cfg, pool, start, actions, af, ef


def assert_every_event(af, ef):
    live = (af & spec.AF_LIVE) != 0
    assert (live & ((af & spec.AF_TERMINATED) != 0)).any(), "no newly terminated agent"
    assert (live & ((af & spec.AF_TRUNCATED) != 0)).any(), "no truncated agent"
    assert (~live).any(), "no non-live agent-step"
    for bit, name in ((spec.EF_ALL_TERMINATED, "ALL_TERMINATED"), (spec.EF_ALL_TRUNCATED, "ALL_TRUNCATED"), (spec.EF_RESET, "RESET")):
        assert (ef & bit).any(), f"no EF_{name}"


@pytest.mark.parametrize("N, reward, terminated", PARAMS, ids=IDS)
def test_recorded_trajectories_reach_every_event(oracle, N, reward, terminated):
    _, _, _, actions, af, ef = record(oracle, N, reward, terminated)
    assert_every_event(af, ef)
    assert len(np.unique(actions[:, [1, 2, 4]])) == 5             # the random envs use every action


@pytest.mark.gpu
@pytest.mark.parametrize("N, reward, terminated", PARAMS, ids=IDS)
def test_rollout_step_and_split_step_agree_bit_for_bit(oracle, N, reward, terminated):
    import torch

    from collectivecrossing_amd.batched import BatchedCollectiveCrossing

    cfg, pool, start, actions, _, _ = record(oracle, N, reward, terminated)
    env = BatchedCollectiveCrossing(cfg, E, device="cuda:0")
    env.set_reset_pool(pool)
    acts = torch.from_numpy(actions).to(env.device)

    def bits(res):                                               # (copies: a step's result lives in buffers the next step reuses)
        return dict(reward=res.reward.cpu().numpy().view(np.uint64), agent_flags=res.agent_flags.cpu().numpy(),
                    env_flags=res.env_flags.cpu().numpy(), compact=res.obs_compact.cpu().numpy().view(np.uint32),
                    obs=res.obs.cpu().numpy().view(np.uint32))

    def stacked(steps):
        return {k: np.stack([s[k] for s in steps]) for k in steps[0]}

    # (A) one rollout of K = 20: the rollout kernel (the short-launch kernel serves K <= 16)
    env.set_state(**start)
    a = bits(env.rollout(acts, auto_reset=True, want_compact=True))
    a_state = env.get_state()
    # (B) 20 rollouts of K = 1 with auto-reset: the short-launch kernel
    assert env.step_shape()["ok"] == 1
    env.set_state(**start)
    b = stacked([{k: v[0] for k, v in bits(env.rollout(acts[s:s + 1], auto_reset=True, want_compact=True)).items()} for s in range(K)])
    b_state = env.get_state()
    # (C) 20 x begin + finish with no caller arrays: the split step
    env.set_state(**start)
    steps = []
    for s in range(K):
        env.step_begin(acts[s])
        steps.append(bits(env.step_finish(auto_reset=True, want_compact=True)))
    c = stacked(steps)
    c_state = env.get_state()
    env.close()

    assert_every_event(a["agent_flags"], a["env_flags"])
    for name, other, other_state in (("step kernel", b, b_state), ("split step", c, c_state)):
        for k in a:
            np.testing.assert_array_equal(other[k], a[k], err_msg=f"{name} vs rollout kernel: {k}")
        for k in spec.STATE_KEYS:
            np.testing.assert_array_equal(other_state[k], a_state[k], err_msg=f"{name} vs rollout kernel: final {k}")
