"""The split step (ccx_step_begin + ccx_step_finish, csrc/ccx_split_step.hip) with the handle's built-in rules:
begin + finish() equals the reference-recorded step, and equals ccx_step on a twin handle in every output byte and in the
state -- small grids, dense collisions with shuffled move orders, edge cases, position-only tables, 64 agents in
all_at_destination mode, and a 100 x 100 grid whose occupancy tables do not fit in LDS."""

import sys
from pathlib import Path

import numpy as np
import pytest
from _fixtures import Golden, assert_step_matches

sys.path.insert(0, str(Path(__file__).resolve().parent / "golden"))
import custom_strategies as cs  # noqa: E402

pytestmark = pytest.mark.gpu

FIXTURES = ["g1_c1_random", "g3_c3_dense_shuffled", "g3_c3_dense_simple_distance", "g5_edges_all_at_dest_binary",
            "g5_edges_constant_negative", "g5_edges_default", "g5_edges_simple_distance_zero_factor",
            "g13_position_only_both", "g4_c5_all_at_dest_greedy_32_32", "g14_waiting_100x100"]


@pytest.fixture(scope="module")
def ccx():
    import torch

    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    from collectivecrossing_amd import strategies
    from collectivecrossing_amd.batched import BatchedCollectiveCrossing
    plugins = cs.make_position_only(strategies.RewardFunction, strategies.TerminatedFunction)
    strategies.REWARD_FUNCTIONS[cs.PO_NAMES["reward"]] = plugins["reward"]
    strategies.TERMINATED_FUNCTIONS[cs.PO_NAMES["terminated"]] = plugins["terminated"]
    yield BatchedCollectiveCrossing
    strategies.REWARD_FUNCTIONS.pop(cs.PO_NAMES["reward"], None)
    strategies.TERMINATED_FUNCTIONS.pop(cs.PO_NAMES["terminated"], None)


def _np(t):
    return None if t is None else t.cpu().numpy()


def test_the_fixture_list_is_complete():
    assert len(FIXTURES) == 10 and all((Path(__file__).resolve().parent / "golden" / f"{n}.npz").exists() for n in FIXTURES)


@pytest.mark.parametrize("name", FIXTURES)
def test_begin_plus_finish_equals_the_reference_and_ccx_step(ccx, name):
    g = Golden(name)
    split, twin = ccx(g.config, g.E), ccx(g.config, g.E)
    assert not split.has_array_strategies
    if name.startswith("g14_"):
        assert twin.step_shape()["ok"] == 0, "this grid is meant to be too large for the LDS tables"
    for env in (split, twin):
        env.set_state(**g.init_state())
    for s in range(g.K):
        split.step_begin(g["actions"][s], g["order"][s])
        mid = split.get_state()
        for k in ("x", "y", "active", "step_count"):                       # begin: the moves, deactivation, the counter
            np.testing.assert_array_equal(mid[k], g[k][s], err_msg=f"{k} after begin, {name} step {s}")
        prev_t = g["terminated"][s - 1] if s else g["init_terminated"]
        prev_u = g["truncated"][s - 1] if s else g["init_truncated"]
        np.testing.assert_array_equal(mid["terminated"], prev_t, err_msg=f"begin touched a flag, {name} step {s}")
        np.testing.assert_array_equal(mid["truncated"], prev_u, err_msg=f"begin touched a flag, {name} step {s}")
        r = split.step_finish(want_compact=True)
        t = twin.step(g["actions"][s], g["order"][s], want_compact=True)
        got = [_np(v) for v in (r.obs, r.reward, r.agent_flags, r.env_flags, r.obs_compact)]
        exp = [_np(v) for v in (t.obs, t.reward, t.agent_flags, t.env_flags, t.obs_compact)]
        assert_step_matches(g, s, got[0], got[1], got[2], got[3], split.get_state(), label="split")
        for what, a, b in zip(("obs", "reward", "agent_flags", "env_flags", "obs_compact"), got, exp):
            np.testing.assert_array_equal(a.view(np.uint8), b.view(np.uint8), err_msg=f"{what} vs ccx_step, {name} step {s}")
        assert _np(r.term_present).all(), "built-in termination rules have an entry for every agent"
        sa, sb = split.get_state(), twin.get_state()
        for k in sa:
            np.testing.assert_array_equal(sa[k], sb[k], err_msg=f"state {k} vs ccx_step, {name} step {s}")
    assert split.counters() == twin.counters()
    split.close()
    twin.close()


def test_finish_without_observation_rows_and_with_auto_reset_equals_a_one_step_rollout(ccx):
    """want_obs=False, and auto_reset: the env restarts from the pool entry ccx_rollout takes (EF_RESET, episode cursor)."""
    import bench
    from collectivecrossing_amd.reset import build_reset_pool
    cfg = bench.c2_config(max_steps=5)
    E, K = 300, 17
    pool = build_reset_pool(cfg, 7, 41)
    actions = np.random.default_rng(3).integers(0, 5, size=(K, E, 8), dtype=np.uint8)
    split, twin = ccx(cfg, E), ccx(cfg, E)
    for env in (split, twin):
        env.set_reset_pool(pool)
        env.reset_from_pool()
    resets = 0
    for s in range(K):
        split.step_begin(actions[s])
        r = split.step_finish(want_obs=False, auto_reset=True)
        assert r.obs is None
        t = twin.rollout(actions[s][None], auto_reset=True, want_obs=False)
        np.testing.assert_array_equal(_np(r.agent_flags), _np(t.agent_flags)[0])
        np.testing.assert_array_equal(_np(r.env_flags), _np(t.env_flags)[0])
        np.testing.assert_array_equal(_np(r.reward).view(np.uint64), _np(t.reward)[0].view(np.uint64))
        resets += int(((_np(r.env_flags) & 4) != 0).sum())
        sa, sb = split.get_state(), twin.get_state()
        for k in sa:
            np.testing.assert_array_equal(sa[k], sb[k], err_msg=f"state {k} step {s}")
    assert resets >= 2 * E
    assert split.counters() == twin.counters()
    split.close()
    twin.close()
