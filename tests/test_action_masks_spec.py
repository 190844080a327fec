"""Legal-action masks without a GPU: the reference-recorded fixtures against the host view and against an independent
NumPy spec, the spec against ``oracle.step`` (the behavioural restatement of include/ccx.h: CCX_ACTION_MASKS), and
``unpack_action_masks``."""

import numpy as np
import pytest
import torch

from _action_masks import DIRS, MASK_NPZ, WAIT_ONLY, MaskFixture, random_states, spec_masks
from _fixtures import Golden


def test_the_fixture_set_is_complete():
    assert len(MASK_NPZ) == 6
    for key in ("c1", "c3_dense", "sealed_door", "edge_walk", "all_at_destination", "100x100"):
        assert f"g15_action_masks_{key}" in MASK_NPZ
    f = MaskFixture("g15_action_masks_edge_walk")
    assert (f["x"] == f.config.width).any() and (f["y"] == f.config.height).any()
    # arrived agents (inactive, still listed) that share a cell
    f = MaskFixture("g15_action_masks_all_at_destination")
    shared = 0
    for s in range(f.S):
        idle = (f["active"][s] == 0) & (f["listed"][s] != 0)
        cells = list(zip(f["x"][s][idle].tolist(), f["y"][s][idle].tolist()))
        shared += len(cells) - len(set(cells))
    assert shared > 0
    for name in MASK_NPZ:
        f = MaskFixture(name)
        assert ((f["masks"] & 0xE0) == 0).all() and ((f["masks"] & 0x10) != 0).all()
        assert (f["masks"][f["listed"] == 0] == WAIT_ONLY).all()
        assert ((f["listed"] != 0) == ((f["terminated"] == 0) & (f["truncated"] == 0))).all()


@pytest.mark.parametrize("name", MASK_NPZ)
def test_host_view_action_masks_equal_the_reference(name):
    """``CollectiveCrossingEnv.host_view(config).action_masks()`` on every recorded state."""
    from collectivecrossing_amd.env import CollectiveCrossingEnv

    f = MaskFixture(name)
    env = CollectiveCrossingEnv.host_view(f.config)
    ids = env.possible_agents
    for s in range(f.S):
        for i, aid in enumerate(ids):
            ag = env._agents[aid]
            ag.position = (int(f["x"][s, i]), int(f["y"][s, i]))
            ag.active, ag.terminated, ag.truncated = (bool(f[k][s, i]) for k in ("active", "terminated", "truncated"))
        got = env.action_masks()
        assert list(got) == [aid for i, aid in enumerate(ids) if f["listed"][s, i]], (name, s)
        for i, aid in enumerate(ids):
            if f["listed"][s, i]:
                m = got[aid]
                assert m.dtype == np.int8 and m.shape == (5,)
                assert int((m.astype(np.uint8) << np.arange(5, dtype=np.uint8)).sum()) == int(f["masks"][s, i]), (name, s, aid)


@pytest.mark.parametrize("name", MASK_NPZ)
def test_numpy_spec_equals_the_reference(name, oracle):
    f = MaskFixture(name)
    np.testing.assert_array_equal(spec_masks(oracle, f.params, **f.state()), f["masks"], err_msg=name)


@pytest.mark.parametrize("name,seed", [("g1_c1_random", 1), ("g3_c3_dense_shuffled", 2), ("g7_n3_small", 3), ("g7_n5_odd", 4)])
def test_spec_is_what_a_step_does(name, seed, oracle):
    """The behavioural restatement: for a live agent i that is still active, bit a is set <=> a step whose action tensor
    is 255 everywhere except actions[i] = a changes agent i's position.  A live agent that has arrived (inactive) is
    never moved by a step (collectivecrossing.py:397-399), whatever its bits say -- they follow ``_is_valid_action``,
    which looks at the target cell only -- and done agents hold 0x10.  Random states with truncated-but-active blockers
    and inactive agents on shared cells."""
    params = Golden(name).params
    N = params.num_agents
    S = 48
    st = random_states(oracle, params, S, seed)
    masks = spec_masks(oracle, params, **st)
    done = (st["terminated"] != 0) | (st["truncated"] != 0)
    assert (masks[done] == WAIT_ONLY).all()
    blockers = ((st["truncated"] != 0) & (st["active"] != 0)).sum()
    assert blockers > 0 and (st["active"] == 0).sum() > 0
    # one probe env per (state, agent, direction)
    rep = lambda a: np.repeat(a, N * 4, axis=0)  # noqa: E731
    ob = oracle.OracleBatch(params, S * N * 4)
    ob.set_state(**{k: rep(v) for k, v in st.items()}, step_count=np.zeros(S * N * 4, np.int32))
    actions = np.full((S, N, 4, N), 255, np.uint8)
    for i in range(N):
        for a in range(4):
            actions[:, i, a, i] = a
    x0, y0 = ob.x.copy(), ob.y.copy()
    ob.step(actions.reshape(S * N * 4, N), want_obs=False)
    moved_any = ((ob.x != x0) | (ob.y != y0)).reshape(S, N, 4, N)
    checked = cleared_by_blocker = 0
    for i in range(N):
        for a, (dx, dy) in enumerate(DIRS):
            moved = moved_any[:, i, a, i]
            assert not np.delete(moved_any[:, i, a], i, axis=1).any()           # nobody else moves
            bit = ((masks[:, i] >> a) & 1) != 0
            live_active = ~done[:, i] & (st["active"][:, i] != 0)
            np.testing.assert_array_equal(moved[live_active], bit[live_active], err_msg=f"{name} agent {i} action {a}")
            assert not moved[st["active"][:, i] == 0].any()                       # an arrived agent stays, whatever its bits
            checked += int(live_active.sum())
            tx, ty = st["x"][:, i] + dx, st["y"][:, i] + dy
            trunc_block = ((st["x"] == tx[:, None]) & (st["y"] == ty[:, None]) & (st["truncated"] != 0) & (st["active"] != 0)).any(1)
            cleared_by_blocker += int((trunc_block & live_active & ~bit).sum())
    assert checked > S and cleared_by_blocker > 0


def test_unpack_action_masks_round_trips():
    from collectivecrossing_amd import unpack_action_masks
    from collectivecrossing_amd.batched import pack_action_masks

    all_bytes = (np.arange(16, dtype=np.uint8) | 0x10).reshape(2, 8)
    u = unpack_action_masks(all_bytes)
    assert u.dtype == bool and u.shape == (2, 8, 5) and u[..., 4].all()
    for a in range(4):
        np.testing.assert_array_equal(u[..., a], ((all_bytes >> a) & 1) != 0)
    np.testing.assert_array_equal(pack_action_masks(u), all_bytes)
    t = unpack_action_masks(torch.from_numpy(all_bytes))
    assert isinstance(t, torch.Tensor) and t.dtype is torch.bool and tuple(t.shape) == (2, 8, 5)
    np.testing.assert_array_equal(t.numpy(), u)
    np.testing.assert_array_equal(pack_action_masks(t), all_bytes)
    # the use it is made for
    logits = torch.zeros(2, 8, 5).masked_fill(~t, float("-inf"))
    assert torch.isfinite(logits[..., 4]).all() and (torch.isinf(logits) == ~t).all()
    with pytest.raises(TypeError):
        unpack_action_masks(np.zeros(3, np.int32))


def test_mask_symbols_are_declared_and_bound():
    """(tests/test_abi.py compares the whole header with the bindings; this names the three new symbols)"""
    from collectivecrossing_amd import _abi

    for sym in ("ccx_action_masks", "ccx_bind_action_masks", "ccx_get_masks_fused"):
        assert sym in _abi.PROTOTYPES
    assert _abi.ABI_VERSION == 5
