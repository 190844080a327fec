"""CCX_RESET_OBS_NEXT on the GPU: every path against the NumPy spec (tests/_reset_obs_spec.py) as u32 bit patterns, the
side buffers' contract, and everything else of a call against a TERMINAL-mode twin."""

import numpy as np
import pytest
from _reset_obs_spec import CASES, EF_RESET, SENTINEL, Case, restart_conditions

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ccx():
    import torch

    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    from collectivecrossing_amd.batched import BatchedCollectiveCrossing

    return BatchedCollectiveCrossing


def _u32(t):
    return np.ascontiguousarray(t.cpu().numpy() if hasattr(t, "cpu") else t).view(np.uint32)


def _new(ccx, case, track=True):
    b = ccx(case.config, case.E, env_offset=case.env_offset, total_envs=case.total_envs)
    b.set_reset_pool(case.pool)
    b.reset_from_pool()
    b.set_state(step_count=case.step_count0)
    if track:
        b.track_episodes()
    return b


def _launch(b, case, q, mode, masks):
    """Launch q of the case on batch b -> (obs, compact, final_obs, final_compact, reward, agent_flags, env_flags)."""
    import torch
    k, nxt = case.chunks[q], mode == "next"
    acts = torch.from_numpy(case.actions[q]).cuda()
    if case.drive == "finish":
        b.step_begin(acts[0])
        if nxt:     # the batch's own side buffers: the sentinel goes in before the call
            for t in b.step_final_buffers(want_obs=True, want_compact=True):
                t.view(torch.uint8).fill_(SENTINEL)
        r = b.step_finish(auto_reset=True, want_compact=True, reset_obs=mode, want_final=nxt)
        return tuple(None if t is None else t.clone()[None] for t in
                     (r.obs, r.obs_compact, r.final_obs, r.final_compact, r.reward, r.agent_flags, r.env_flags))
    out = b.alloc_rollout(k, True, True, want_final=nxt)
    if nxt:
        out.final_obs.view(torch.uint8).fill_(SENTINEL)
        out.final_compact.view(torch.uint8).fill_(SENTINEL)
    kw = dict(auto_reset=True, out=out, masks_out=masks, reset_obs=mode)
    if case.drive == "greedy":
        b.rollout_greedy(k, want_actions=False, **kw)
    elif case.drive == "mixed":
        b.rollout_mixed(acts, "exiting", want_compact=True, **kw)
    else:
        b.rollout(acts, None if case.orders[q] is None else torch.from_numpy(case.orders[q]).cuda(), want_compact=True, **kw)
    return out.obs, out.obs_compact, out.final_obs, out.final_compact, out.reward, out.agent_flags, out.env_flags


@pytest.mark.parametrize("name", list(CASES))
def test_next_mode_equals_the_spec_and_changes_nothing_else(ccx, oracle, name):
    import torch
    case = Case(name, oracle)
    A, B = _new(ccx, case), _new(ccx, case)
    E, N = case.E, case.N
    if name.startswith("k1_") or name.startswith("order"):
        assert A.reset_obs_fused() and A.reset_obs_fused(1, order=False, mixed=False)
    assert not A.reset_obs_fused(16) and not A.reset_obs_fused(1, order=True) and not A.reset_obs_fused(1, mixed=True)
    if case.big:
        assert not A.reset_obs_fused()
    mA, mB = (torch.zeros((E, N), dtype=torch.uint8, device="cuda") for _ in range(2))
    flags = []
    for q, k in enumerate(case.chunks):
        masks = q % 2 == 0 and case.drive != "finish"         # with and without bound masks
        ep0 = B.get_state()["episode"].copy()
        oa = _launch(A, case, q, "next", mA if masks else None)
        ob = _launch(B, case, q, "terminal", mB if masks else None)
        torch.cuda.synchronize()
        term = dict(obs=ob[0].cpu().numpy(), obs_compact=ob[1].cpu().numpy(), agent_flags=ob[5].cpu().numpy(),
                    env_flags=ob[6].cpu().numpy(), episode_before=ep0)
        if case.oracle_chunks is not None:       # the spec's input is the CPU oracle's trajectory (and the twin equals it)
            och = case.oracle_chunks[q]
            assert np.array_equal(_u32(term["obs"]), _u32(och["obs"])) and np.array_equal(term["env_flags"], och["env_flags"])
            assert np.array_equal(ep0, och["episode_before"])
            term = dict(och, obs_compact=term["obs_compact"])
        s_obs, s_cmp, s_fo, s_fc, s_ep = case.spec(term)
        ef = term["env_flags"]
        flags.append(ef)
        r = (ef & EF_RESET) != 0
        for what, got, want in (("obs", oa[0], s_obs), ("obs_compact", oa[1], s_cmp), ("final_obs", oa[2], s_fo),
                                ("final_compact", oa[3], s_fc)):
            assert np.array_equal(_u32(got), _u32(want)), (name, q, what)
        # the side buffers: the caller's bytes wherever EF_RESET is clear, the TERMINAL-mode rows where it is set
        assert (oa[2].cpu().numpy()[~r].view(np.uint8) == SENTINEL).all() and (oa[3].cpu().numpy()[~r].view(np.uint8) == SENTINEL).all()
        assert np.array_equal(_u32(oa[2].cpu().numpy()[r]), _u32(term["obs"][r]))
        assert np.array_equal(_u32(oa[3].cpu().numpy()[r]), _u32(term["obs_compact"][r]))
        # nothing else moves: rewards, flags, state, masks, counters
        assert torch.equal(oa[4].view(torch.int64), ob[4].view(torch.int64)) and torch.equal(oa[5], ob[5]) and torch.equal(oa[6], ob[6])
        sa, sb = A.get_state(), B.get_state()
        assert all(np.array_equal(sa[f], sb[f]) for f in sa) and np.array_equal(sa["episode"], s_ep)
        assert A.counters() == B.counters()
        if masks:
            assert torch.equal(mA, mB) and torch.equal(mA, A.action_masks())
        # a restart on the launch's last step: the rows are those of the state the batch now holds
        last = torch.from_numpy(r[-1]).cuda()
        assert torch.equal(oa[0][-1][last].view(torch.int32), A.observe()[last].view(torch.int32))
    ea, eb = A.episode_stats(), B.episode_stats()
    for f in ("ret", "live_steps", "steps", "finished", "last_ret", "last_steps", "last_end"):
        assert torch.equal(getattr(ea, f), getattr(eb, f)), f
    restart_conditions(name, flags)
    A.close()
    B.close()


def test_next_mode_without_auto_reset_is_terminal_mode(ccx, oracle):
    import torch
    case = Case("k16_n5", oracle)
    A, B = _new(ccx, case, False), _new(ccx, case, False)
    acts = torch.from_numpy(case.actions[0]).cuda()
    for k in (1, 16):
        oa = A.alloc_rollout(k, True, True, want_final=True)
        oa.final_obs.view(torch.uint8).fill_(SENTINEL)
        A.rollout(acts[:k], auto_reset=False, out=oa, reset_obs="next")
        ob = B.rollout(acts[:k], auto_reset=False, want_compact=True)
        for f in ("obs", "obs_compact", "reward", "agent_flags", "env_flags"):
            assert torch.equal(getattr(oa, f).view(torch.uint8), getattr(ob, f).view(torch.uint8)), (k, f)
        assert bool((oa.final_obs.view(torch.uint8) == SENTINEL).all()) and not bool((oa.env_flags & EF_RESET).any())
    A.close()
    B.close()


def test_fused_rows_equal_the_fix_up_kernel_and_finals_may_be_dropped(ccx, oracle):
    """The same K = 1 launches through the step kernel's own redirect and (tunable) through the fix-up kernel; without
    side buffers the terminal rows are dropped and the rest is the same."""
    import torch
    case = Case("k1_n8", oracle)
    A, B, D = _new(ccx, case, False), _new(ccx, case, False), _new(ccx, case, False)
    B.set_tunable("reset_obs_fused", 0)
    assert A.reset_obs_fused() and not B.reset_obs_fused()
    for q in range(len(case.chunks)):
        oa, ob = _launch(A, case, q, "next", None), _launch(B, case, q, "next", None)
        od = D.rollout(torch.from_numpy(case.actions[q]).cuda(), auto_reset=True, want_compact=True, reset_obs="next")
        assert od.final_obs is None
        for x, y in zip(oa, ob):
            assert torch.equal(x.view(torch.uint8), y.view(torch.uint8))
        assert torch.equal(od.obs.view(torch.int32), oa[0].view(torch.int32)) and torch.equal(od.obs_compact.view(torch.int32), oa[1].view(torch.int32))
    for b in (A, B, D):
        b.close()


def test_a_call_without_env_flags_is_refused(ccx, oracle):
    import ctypes as C

    import torch

    from collectivecrossing_amd import _abi
    from collectivecrossing_amd._lib import CcxError, check
    case = Case("k1_n5", oracle)
    A = _new(ccx, case, False)
    out = A.alloc_rollout(1)
    acts = torch.from_numpy(case.actions[0]).cuda()
    ro = _abi.CcxRolloutOut(out.obs.data_ptr(), out.reward.data_ptr(), out.agent_flags.data_ptr(), None, None)
    check(A._lib.ccx_set_reset_obs(A._h, 1))
    with pytest.raises(CcxError, match="env_flags"):
        check(A._lib.ccx_rollout(A._h, 1, acts.data_ptr(), None, 1, C.byref(ro)))
    check(A._lib.ccx_rollout(A._h, 1, acts.data_ptr(), None, 0, C.byref(ro)))        # without auto-reset: untouched
    check(A._lib.ccx_set_reset_obs(A._h, 0))
    check(A._lib.ccx_rollout(A._h, 1, acts.data_ptr(), None, 1, C.byref(ro)))
    with pytest.raises(CcxError, match="mode"):
        check(A._lib.ccx_set_reset_obs(A._h, 2))
    with pytest.raises(ValueError, match="reset_obs"):
        A.rollout(acts, auto_reset=True, reset_obs="later")
    A.close()


def test_a_captured_next_mode_step_with_masks_replays_the_eager_run(ccx, oracle):
    import torch
    case = Case("k1_n8", oracle)
    A, B = _new(ccx, case, False), _new(ccx, case, False)
    E, N = case.E, case.N
    acts = torch.from_numpy(case.actions[0]).cuda()
    side = torch.cuda.Stream()
    B.use_stream(side)
    torch.cuda.synchronize()
    mA, mB = (torch.zeros((E, N), dtype=torch.uint8, device="cuda") for _ in range(2))
    oa, ob = A.alloc_rollout(1, True, True, want_final=True), B.alloc_rollout(1, True, True, want_final=True)
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        B.rollout(acts, auto_reset=True, out=ob, masks_out=mB, reset_obs="next")     # first call outside the capture
        side.synchronize()
        B.set_state(episode=np.zeros(E, np.int32))
        B.reset_from_pool()
        B.set_state(step_count=case.step_count0)
        keep = torch.zeros((30,) + tuple(ob.obs.shape[1:]), device="cuda")
        n = torch.zeros((), dtype=torch.int64, device="cuda")
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            B.rollout(acts, auto_reset=True, out=ob, masks_out=mB, reset_obs="next")
            keep.index_copy_(0, n.reshape(1), ob.obs)
            n.add_(1)
        B.set_state(episode=np.zeros(E, np.int32))
        B.reset_from_pool()
        B.set_state(step_count=case.step_count0)
        n.zero_()
        side.synchronize()
        for _ in range(30):
            graph.replay()
        side.synchronize()
    resets = 0
    for s in range(30):
        A.rollout(acts, auto_reset=True, out=oa, masks_out=mA, reset_obs="next")
        assert torch.equal(oa.obs[0].view(torch.int32), keep[s].view(torch.int32)), s
        resets += int((oa.env_flags & EF_RESET).ne(0).sum())
    torch.cuda.synchronize()
    assert resets >= 3 * E
    for f in ("obs", "obs_compact", "final_obs", "final_compact", "reward", "agent_flags", "env_flags"):
        assert torch.equal(getattr(oa, f).view(torch.uint8), getattr(ob, f).view(torch.uint8)), f
    assert torch.equal(mA, mB)
    sa, sb = A.get_state(), B.get_state()
    assert all(np.array_equal(sa[f], sb[f]) for f in sa)
    A.close()
    B.close()
