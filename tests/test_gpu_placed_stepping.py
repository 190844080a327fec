"""The env's kernels on arrays at every legal offset, inside guard bands (tests/_placed.py).

The rule: any placement include/ccx.h allows gives the same bits, and nothing outside the arrays handed over is written.
The rollout kernel picks its instantiation from ``out.obs & 127`` (csrc/ccx_rollout_g.hip), its row writers and the step
kernel derive a per-tile ``lead`` from the absolute address and move their store base below the region
(csrc/ccx_rollout_body.inc, csrc/ccx_step.hip), and NEXT mode offsets the side buffer by the lead of ``obs``: here every
array of a call sits at its own residue mod 128 (u8 arrays at odd addresses, rewards at +8, ``final_obs`` at another
residue than ``obs``) with 4096 sentinel bytes on either side.  Expected bits: the same call on a twin batch with
``alloc_rollout`` outputs, and for the tensor, move-order and greedy drives the CPU oracle's trajectory on top.
"""
import ctypes as C

import numpy as np
import pytest
from _placed import SENTINEL, PlacedCall

pytestmark = pytest.mark.gpu

EF_RESET = 0x04
# (N, E, E is a multiple of rows_alignment())
CASES = [(8, 64, True), (8, 67, False), (3, 64, True), (3, 70, False), (5, 64, True), (5, 67, False), (50, 136, True),
         (50, 131, False)]
IDS = [f"n{n}_e{e}" for n, e, _ in CASES]
ALL_OFFSETS = tuple(range(0, 128, 16))
EDGE_OFFSETS = (16, 112)
FINAL_OFFSET = {16: 80, 112: 16}        # final_obs never shares the residue of obs
# fixed residues of everything but obs: (offset, alignment include/ccx.h asks of that pointer)
AT = dict(obs_compact=(48, 16), reward=(8, 8), agent_flags=(1, 1), env_flags=(3, 1), actions=(1, 1), order=(3, 1),
          masks_out=(5, 1), actions_out=(7, 1), final_compact=(32, 16))


@pytest.fixture(scope="module")
def ccx():
    import torch

    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    from collectivecrossing_amd.batched import BatchedCollectiveCrossing

    return BatchedCollectiveCrossing


def _config(N):
    if N == 50:
        import bench
        return bench.workload_config("c5_50")[0]
    from test_gpu_round4_shapes import _cfg
    return _cfg(12, 8, N)


class Rig:
    """One (N, E): config, pool, the staggered start state, inputs, and fresh batches in that state."""

    def __init__(self, ccx, N, E, aligned):
        from collectivecrossing_amd.params import lower_config
        from collectivecrossing_amd.reset import build_reset_pool
        self.ccx, self.N, self.E = ccx, N, E
        self.config = _config(N)
        self.params = lower_config(self.config)
        assert self.params.num_agents == N
        self.L = 6 + 4 * N
        self.pool = build_reset_pool(self.config, 900 + N, 37)
        # step counters staggered just below max_steps: every launch of one step or more restarts envs (EF_RESET)
        self.step_count0 = (self.params.max_steps - 1 - np.arange(E) % 4).astype(np.int32)
        self.rng = np.random.default_rng(1000 * N + E)
        self.batches = []
        probe = self.batch()
        # the two classes of batch size, through the rule itself
        assert (E % probe.rows_alignment() == 0) == aligned, (N, E, probe.rows_alignment())
        self.obs_align = 16 if N % 2 == 0 else 8

    def batch(self, **tunables):
        b = self.ccx(self.config, self.E)
        self.batches.append(b)
        b.set_reset_pool(self.pool)
        for k, v in tunables.items():
            b.set_tunable(k, v)
        self.restore(b)
        return b

    def restore(self, b):
        b.set_state(episode=np.zeros(self.E, np.int32))
        b.reset_from_pool()
        b.set_state(step_count=self.step_count0)
        b.zero_counters()

    def oracle(self, oracle_mod):
        ob = oracle_mod.OracleBatch(self.params, self.E)
        ob.set_reset_pool(self.pool)
        ob.reset_from_pool()
        ob.set_state(step_count=self.step_count0)
        return ob

    def actions(self, K):
        return self.rng.integers(0, 5, size=(K, self.E, self.N), dtype=np.uint8)

    def orders(self, K):
        return np.argsort(self.rng.random((K, self.E, self.N)), axis=-1).astype(np.uint8)

    def close(self):
        for b in self.batches:
            b.close()


@pytest.fixture(params=CASES, ids=IDS)
def rig(request, ccx):
    r = Rig(ccx, *request.param)
    yield r
    r.close()


class Call(PlacedCall):
    """The placed arrays of one stepping call; arrays other than obs sit at the fixed residues of ``AT``."""

    def __init__(self, rig, ctx):
        super().__init__(ctx)
        self.rig = rig

    def out(self, name, shape, dtype, offset=None, align=None):
        if offset is None:
            offset, align = AT[name]
        return super().out(name, shape, dtype, offset, align)

    def inp(self, name, array):
        return super().inp(name, array, *AT[name])

    def rollout_out(self, K, obs_offset, want_compact=True, want_final=False):
        import torch

        from collectivecrossing_amd.batched import RolloutResult
        E, N, L = self.rig.E, self.rig.N, self.rig.L
        f32 = torch.float32
        res = RolloutResult(self.out("obs", (K, E, N, L), f32, obs_offset, self.rig.obs_align),
                            self.out("reward", (K, E, N), torch.float64), self.out("agent_flags", (K, E, N), torch.uint8),
                            self.out("env_flags", (K, E), torch.uint8),
                            self.out("obs_compact", (K, E, N, 4), f32) if want_compact else None)
        if want_final:
            fo = FINAL_OFFSET[obs_offset]
            assert fo % 128 != obs_offset % 128
            res.final_obs = self.out("final_obs", (K, E, N, L), f32, fo, self.rig.obs_align)
            res.final_compact = self.out("final_compact", (K, E, N, 4), f32)
        return res


def _np(t):
    return t.detach().cpu().numpy()


def _state_equal(a, b, ctx):
    sa, sb = a.get_state(), b if isinstance(b, dict) else b.get_state()
    for f in ("x", "y", "active", "terminated", "truncated", "step_count", "episode"):
        assert np.array_equal(sa[f], np.asarray(sb[f])), (ctx, "state", f)


def _ctx(rig, b, drive, off):
    return f"N={rig.N} E={rig.E} {drive} obs at +{off} launch_shape={b.launch_shape()}"


def _twin_dict(res, **more):
    d = {k: getattr(res, k) for k in ("obs", "reward", "agent_flags", "env_flags", "obs_compact") if getattr(res, k) is not None}
    d.update(more)
    return d


def _oracle_state(ob):
    return {f: getattr(ob, f) for f in ("x", "y", "active", "terminated", "truncated", "step_count", "episode")}


def _check_against_oracle(res, o_obs, o_rew, o_af, o_ef, ctx):
    assert np.array_equal(_np(res.agent_flags), o_af), (ctx, "agent_flags vs oracle")
    assert np.array_equal(_np(res.env_flags), o_ef), (ctx, "env_flags vs oracle")
    assert np.array_equal(_np(res.reward).view(np.uint64), o_rew.view(np.uint64)), (ctx, "reward vs oracle")
    assert np.array_equal(_np(res.obs).view(np.uint32), o_obs.view(np.uint32)), (ctx, "obs vs oracle")


# ------------------------------------------------------------------------------------------------ rollout from tensors
def _tensor_drive(rig, oracle, K, order, offsets, drive, tunables=None, writers=(0,)):
    acts = rig.actions(K)
    ords = rig.orders(K) if order else None
    ob = rig.oracle(oracle)
    o_obs, o_rew, o_af, o_ef = ob.rollout(acts, ords, auto_reset=True)
    assert (o_ef & EF_RESET).any()
    twin = rig.batch()
    want = twin.rollout(acts, ords, auto_reset=True, want_compact=True)
    _check_against_oracle(want, o_obs, o_rew, o_af, o_ef, f"N={rig.N} E={rig.E} {drive} twin")
    _state_equal(twin, _oracle_state(ob), "twin vs oracle")
    assert twin.counters() == ob.counters.as_dict()
    b = rig.batch(**(tunables or {}))
    for w in writers:
        if w:
            b.set_writers(w)
            assert b.launch_shape()["writers_per_tile"] == w, b.launch_shape()
        for off in offsets:
            rig.restore(b)
            call = Call(rig, _ctx(rig, b, drive + (f" writers={w}" if w else ""), off))
            out = call.rollout_out(K, off)
            a = call.inp("actions", acts)
            o = call.inp("order", ords) if order else None
            b.rollout(a, o, auto_reset=True, out=out)
            call.check(_twin_dict(want))
            _state_equal(b, _oracle_state(ob), call.ctx)
            assert b.counters() == ob.counters.as_dict(), call.ctx


def test_plain_rollout_at_every_16_byte_offset(rig, oracle):
    """K = 24 from an action tensor: all eight residues of ``obs``.  N = 8 / E = 64 is the shape whose base alone decides
    between the aligned instantiation and the edge one."""
    _tensor_drive(rig, oracle, 24, False, ALL_OFFSETS, "rollout")


@pytest.mark.parametrize("E", [64, 67])
def test_plain_rollout_with_one_two_and_three_writers(ccx, oracle, E):
    rig = Rig(ccx, 8, E, E == 64)
    try:
        _tensor_drive(rig, oracle, 24, False, EDGE_OFFSETS, "rollout", writers=(1, 2, 3))
    finally:
        rig.close()


def test_rollout_with_a_move_order(rig, oracle):
    _tensor_drive(rig, oracle, 24, True, EDGE_OFFSETS, "rollout+order")


def test_rollout_cut_into_sub_launches(rig, oracle):
    """max_launch_steps = 5: each sub-launch's slice starts at base + s * slab, whatever residue that is."""
    _tensor_drive(rig, oracle, 24, False, EDGE_OFFSETS, "rollout cut at 5", tunables=dict(max_launch_steps=5))


# ------------------------------------------------------------------------------------------------ scripted drives
def test_greedy_rollout_with_actions_out(rig, oracle):
    import torch
    K = 12
    ob = rig.oracle(oracle)
    o_act, o_obs, o_rew, o_af, o_ef = ob.rollout_greedy(K, auto_reset=True)
    assert (o_ef & EF_RESET).any()
    b = rig.batch()
    for off in EDGE_OFFSETS:
        rig.restore(b)
        call = Call(rig, _ctx(rig, b, "rollout_greedy", off))
        out = call.rollout_out(K, off, want_compact=False)
        ao = call.out("actions_out", (K, rig.E, rig.N), torch.uint8)
        b.rollout_greedy(K, auto_reset=True, out=out, actions_out=ao)
        call.check(dict(obs=o_obs, reward=o_rew, agent_flags=o_af, env_flags=o_ef, actions_out=o_act))
        _state_equal(b, _oracle_state(ob), call.ctx)
        assert b.counters() == ob.counters.as_dict(), call.ctx


def test_mixed_control_rollout(rig):
    import torch
    K = 17
    acts = rig.actions(K)
    twin = rig.batch()
    t_ao = torch.empty((K, rig.E, rig.N), dtype=torch.uint8, device="cuda")
    want = twin.rollout_mixed(acts, "exiting", auto_reset=True, want_compact=True, actions_out=t_ao)
    assert bool((want.env_flags & EF_RESET).any())
    b = rig.batch()
    for off in EDGE_OFFSETS:
        rig.restore(b)
        call = Call(rig, _ctx(rig, b, "rollout_mixed", off))
        out = call.rollout_out(K, off)
        ao = call.out("actions_out", (K, rig.E, rig.N), torch.uint8)
        a = call.inp("actions", acts)
        b.rollout_mixed(a, "exiting", auto_reset=True, out=out, actions_out=ao)
        call.check(_twin_dict(want, actions_out=t_ao))
        _state_equal(b, twin, call.ctx)
        assert b.counters() == twin.counters(), call.ctx


# ------------------------------------------------------------------------------------------------ NEXT mode
@pytest.mark.parametrize("fused", [1, 0], ids=["redirect_in_launch", "fix_up_kernel"])
@pytest.mark.parametrize("K", [1, 16])
def test_next_mode_with_side_buffers_and_bound_masks(rig, K, fused):
    """``reset_obs="next"`` with ``final_obs`` at another residue than ``obs``: the step kernel's fused redirect (K = 1),
    and with the tunable off (or K = 16) the fix-up kernel.  Rows of envs that did not restart keep the sentinel."""
    import torch
    acts = rig.actions(K)
    twin = rig.batch(reset_obs_fused=fused)
    t_out = twin.alloc_rollout(K, True, True, want_final=True)
    t_out.final_obs.view(torch.uint8).fill_(SENTINEL)
    t_out.final_compact.view(torch.uint8).fill_(SENTINEL)
    t_masks = torch.zeros((rig.E, rig.N), dtype=torch.uint8, device="cuda")
    twin.rollout(acts, auto_reset=True, out=t_out, masks_out=t_masks, reset_obs="next")
    r = (_np(t_out.env_flags) & EF_RESET) != 0
    assert r.any() and not r.all(), "the launch needs envs that restart and envs that do not"
    assert (_np(t_out.final_obs)[~r].view(np.uint8) == SENTINEL).all() and (_np(t_out.final_obs)[r].view(np.uint8) != SENTINEL).any()
    b = rig.batch(reset_obs_fused=fused)
    if K == 1 and fused and b.step_shape()["ok"]:
        assert b.reset_obs_fused(1)
    if not fused or K > 1:
        assert not b.reset_obs_fused(K)
    for off in EDGE_OFFSETS:
        rig.restore(b)
        call = Call(rig, _ctx(rig, b, f"rollout K={K} reset_obs=next fused={fused}", off))
        out = call.rollout_out(K, off, want_final=True)
        m = call.out("masks_out", (rig.E, rig.N), torch.uint8)
        a = call.inp("actions", acts)
        b.rollout(a, auto_reset=True, out=out, masks_out=m, reset_obs="next")
        call.check(_twin_dict(t_out, final_obs=t_out.final_obs, final_compact=t_out.final_compact, masks_out=t_masks))
        _state_equal(b, twin, call.ctx)
        assert b.counters() == twin.counters(), call.ctx
    b.rollout(acts, auto_reset=True, reset_obs="terminal")          # (unbinds the placed side buffers and masks)


# ------------------------------------------------------------------------------------------------ one step
@pytest.mark.parametrize("step_kernel", [1, 0], ids=["step_kernel", "rollout_kernel"])
def test_single_step_through_either_kernel(rig, oracle, step_kernel):
    """``ccx_step`` itself on placed arrays, with masks bound: through the short-launch kernel and through the rollout
    kernel, without and with a move order."""
    import torch

    from collectivecrossing_amd import _abi
    from collectivecrossing_amd._lib import check
    E, N, L = rig.E, rig.N, rig.L
    acts, ords = rig.actions(1)[0], rig.orders(1)[0]
    b = rig.batch(step_kernel=step_kernel)
    twin = rig.batch(step_kernel=step_kernel)
    if not step_kernel:
        assert b.step_shape()["ok"] == 0
    for order in (None, ords):
        ob = rig.oracle(oracle)
        o_obs, o_rew, o_af, o_ef = ob.step(acts, order)[:4]
        rig.restore(twin)
        want = twin.step(acts, order, want_compact=True, want_masks=True)
        assert np.array_equal(_np(want.obs).view(np.uint32), np.asarray(o_obs).view(np.uint32)), "twin obs vs oracle"
        assert np.array_equal(_np(want.reward).view(np.uint64), np.asarray(o_rew).view(np.uint64)), "twin reward vs oracle"
        assert np.array_equal(_np(want.agent_flags), o_af) and np.array_equal(_np(want.env_flags), o_ef)
        for off in EDGE_OFFSETS:
            rig.restore(b)
            call = Call(rig, _ctx(rig, b, f"step step_kernel={step_kernel} order={order is not None}", off))
            so = _abi.CcxStepOut(call.out("obs", (E, N, L), torch.float32, off, rig.obs_align).data_ptr(),
                                 call.out("reward", (E, N), torch.float64).data_ptr(),
                                 call.out("agent_flags", (E, N), torch.uint8).data_ptr(),
                                 call.out("env_flags", (E,), torch.uint8).data_ptr(),
                                 call.out("obs_compact", (E, N, 4), torch.float32).data_ptr())
            m = call.out("masks_out", (E, N), torch.uint8)
            a = call.inp("actions", acts)
            o = None if order is None else call.inp("order", order)
            check(b._lib.ccx_bind_action_masks(b._h, C.c_void_p(m.data_ptr())))
            try:
                check(b._lib.ccx_step(b._h, C.c_void_p(a.data_ptr()), None if o is None else C.c_void_p(o.data_ptr()), C.byref(so)))
            finally:
                check(b._lib.ccx_bind_action_masks(b._h, None))
            call.check(dict(obs=want.obs, reward=want.reward, agent_flags=want.agent_flags, env_flags=want.env_flags,
                            obs_compact=want.obs_compact, masks_out=want.action_masks))
            _state_equal(b, twin, call.ctx)
            assert b.counters() == twin.counters(), call.ctx


# ------------------------------------------------------------------------------------------------ state readers
def test_observe_expand_masks_and_policy_actions_into_placed_arrays(rig, oracle):
    import torch
    E, N, L = rig.E, rig.N, rig.L
    b = rig.batch()
    ob = rig.oracle(oracle)
    acts = rig.actions(3)
    ob.rollout(acts, None, auto_reset=True)
    compact = b.rollout(acts, auto_reset=True, want_compact=True).obs_compact          # [3, E, N, 4]
    want_rows = b.expand_observations(compact)
    want_masks, want_greedy, want_waiting = b.action_masks(), b.policy_actions("greedy"), b.policy_actions("waiting")
    assert np.array_equal(_np(want_greedy), ob.policy_actions("greedy")) and np.array_equal(_np(want_waiting), ob.policy_actions("waiting"))
    state = b.get_state()
    for off in EDGE_OFFSETS:
        call = Call(rig, _ctx(rig, b, "observe / expand / masks / policy_actions", off))
        o = call.out("obs", (E, N, L), torch.float32, off, rig.obs_align)
        rows = call.out("rows", (3, E, N, L), torch.float32, 128 - off, rig.obs_align)
        m = call.out("masks_out", (E, N), torch.uint8)
        g = call.out("actions_out", (E, N), torch.uint8)
        w = call.out("waiting", (E, N), torch.uint8, 9, 1)
        c = call.inp("obs_compact", _np(compact))
        b.observe(out=o)
        assert b.expand_observations(c, out=rows) is rows
        b.action_masks(out=m)
        b.policy_actions("greedy", out=g)
        b.policy_actions("waiting", out=w)
        call.check(dict(obs=ob.observe(), rows=want_rows, masks_out=want_masks, actions_out=want_greedy, waiting=want_waiting))
        _state_equal(b, state, call.ctx)


def test_render_into_placed_frames(rig):
    import torch
    b = rig.batch()
    acts = rig.actions(2)
    compact = b.rollout(acts, auto_reset=True, want_compact=True).obs_compact          # [2, E, N, 4]
    ids = torch.arange(rig.E - 1, -1, -3, dtype=torch.int32, device="cuda")
    want_all, want_ids, want_compact = b.render(cell_px=3), b.render(ids, cell_px=3), b.render_compact(compact, cell_px=3)
    fs = b.frame_shape(3)
    for off in EDGE_OFFSETS:
        call = Call(rig, _ctx(rig, b, "render / render_compact cell_px=3 frames", off))
        f_all = call.out("frames", (rig.E, *fs), torch.uint8, off, 16)
        f_ids = call.out("frames_of_ids", (len(ids), *fs), torch.uint8, 128 - off, 16)
        f_cmp = call.out("frames_of_compact", (2, rig.E, *fs), torch.uint8, off, 16)
        c = call.inp("obs_compact", _np(compact))
        b.render(cell_px=3, out=f_all)
        b.render(ids, cell_px=3, out=f_ids)
        b.render_compact(c, cell_px=3, out=f_cmp)
        call.check(dict(frames=want_all, frames_of_ids=want_ids, frames_of_compact=want_compact))
