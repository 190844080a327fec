"""Every instantiation of rollout_kernel, step_kernel and observe_kernel that a call can select, run on the GPU and compared
with the CPU oracle bit for bit.  The cases are the catalogue of tests/_kernel_keys.py (tests/test_kernel_keys.py shows on the
CPU that it holds every reachable key); each case asserts FIRST that the handle launched the key it stands for
(``ccxi_handle_last_key``: written by the launch path from the very struct the launch switched on), so a case that ran
another instantiation fails instead of passing for the wrong kernel.

A case: a tiny batch on the smallest grid that admits its agent count, a reset pool of five placements, ``max_steps`` 3 with
step counters staggered over the episode, auto-reset on -- envs restart on the first, a middle and the last step of the launch.
Compared: obs as u32 (at residue 16 inside guard bands where the case says so), compact rows, rewards as u64, agent and env
flags, ``actions_out``, the bound masks, ``final_obs`` / ``final_compact`` with the caller's bytes around the restarted rows,
the final state and the six counters; for OUT 0 there are no output arrays and the state and the counters are what is left.
Expected values: the oracle's trajectory (tests/_user_table_cases.oracle_launch: tensor, in-kernel policy, mixed control, user
tables), tests/_reset_obs_spec.next_mode for NEXT-mode rows, tests/_action_masks.spec_masks for the masks."""

import ctypes as C

import numpy as np
import pytest

import _kernel_keys as kk
from _action_masks import spec_masks
from _fixtures import config_from_dict
from _reset_obs_spec import SENTINEL, compact_of, next_mode
from _user_table_cases import STATE_KEYS, make_tables, new_oracle, oracle_launch

pytestmark = pytest.mark.gpu

MAX_STEPS, POOL_SIZE = 3, 5


@pytest.fixture(scope="module")
def ccx():
    import torch

    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    from collectivecrossing_amd.batched import BatchedCollectiveCrossing

    return BatchedCollectiveCrossing


def grid_config(w, h, n):
    """A valid env of any grid from 4 x 4 up: the tram spans the width, the door sits in its middle."""
    nb = (n + 1) // 2
    return config_from_dict(dict(
        width=w, height=h, division_y=h // 2, tram_door_left=w // 2 - 1, tram_door_right=w // 2 + 1, tram_length=w,
        boarding_destination_area_y=h, exiting_destination_area_y=0, num_boarding_agents=nb, num_exiting_agents=n - nb,
        strict_reference_limits=False, truncated_config=dict(truncated_function="max_steps", max_steps=MAX_STEPS),
        terminated_config=dict(terminated_function="individual_at_destination")))


class Setup:
    """What a case needs on the CPU: config, pool, staggered step counters, inputs, tables, scripted slots."""

    def __init__(self, case):
        from collectivecrossing_amd.params import lower_config
        from collectivecrossing_amd.reset import build_reset_pool
        c = self.c = kk.case_dict(case)
        self.N, self.E, self.K = c["N"], c["E"], c["K"]
        self.config = grid_config(*c["grid"], self.N)
        self.params = lower_config(self.config)
        self.pool = build_reset_pool(self.config, 7, POOL_SIZE)
        self.step_count0 = (np.arange(self.E) % MAX_STEPS).astype(np.int32)
        rng = np.random.default_rng([self.N, self.E, max(self.K, 1)])
        K = max(self.K, 1)
        self.actions = rng.integers(0, 5, size=(K, self.E, self.N), dtype=np.uint8)
        self.order = np.argsort(rng.random((K, self.E, self.N)), axis=-1).astype(np.uint8)     # a shuffled move order
        self.tables = {"none": (None, None), "terminated": make_tables("term_only", self.config),
                       "reward": make_tables("reward_only", self.config)}[c["tables"]]
        self.scripted = (np.arange(self.N) % 2 == 1) if self.N > 1 else np.ones(1, bool)       # mixed control: the odd slots
        self.mask = int(sum(1 << i for i in np.flatnonzero(self.scripted)))

    def oracle(self, oracle_mod):
        return new_oracle(oracle_mod, self.params, self.E, self.pool, self.step_count0, self.tables)

    def batch(self, ccx):
        c = self.c
        b = ccx(self.config, self.E)
        b.set_reset_pool(self.pool)
        b.reset_from_pool()
        b.set_state(step_count=self.step_count0)
        if c["lanes"]:
            b.set_launch_shape(c["lanes"], 0)
        for name in ("occ_tables", "step_kernel"):
            if c[name] != -1:
                b.set_tunable(name, c[name])
        reward, term = self.tables
        if reward is not None:
            b.set_reward_table(*reward)
        if term is not None:
            b.set_terminated_table(*term)
        kk.bind_keys(b._lib)
        return b


def last_key(b, which=0):
    k = kk.Key()
    assert b._lib.ccxi_handle_last_key(b._h, which, C.byref(k)) == 0
    return k.tuple()


def _np(t):
    return t.cpu().numpy()


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}.get(a.dtype.itemsize, np.uint8))


def expected(oracle_mod, s, policy):
    """The oracle's launch of the case and, from it, every array the GPU call may be asked for."""
    c = s.c
    drive, _ = kk.DRIVE_NAMES[c["drive"]]
    _actions, has_order, in_kernel, _ao, mixed = drive
    ob = s.oracle(oracle_mod)
    order = s.order if has_order else None
    if in_kernel:
        och = oracle_launch(ob, "greedy", s.K, policy=policy)
    elif mixed:
        scripted = np.ones(s.N, bool) if c["drive"] == "mixed_all_actions_out" else s.scripted
        och = oracle_launch(ob, "mixed", s.K, s.actions, order, policy, scripted)
    else:
        och = oracle_launch(ob, "tensor", s.K, s.actions, order)
    och["obs_compact"] = compact_of(och["obs"], och["agent_flags"], s.params.num_boarding)
    sent = lambda a: np.frombuffer(bytes([SENTINEL]) * a.nbytes, a.dtype).reshape(a.shape)
    och["final_obs"], och["final_compact"] = sent(och["obs"]), sent(och["obs_compact"])
    if c["reset"]:
        och["obs"], och["obs_compact"], och["final_obs"], och["final_compact"], _ = next_mode(
            och["obs"], och["obs_compact"], och["env_flags"], s.pool, 0, s.E, och["episode_before"], s.params,
            och["final_obs"], och["final_compact"])
    st = och["state"]
    och["masks"] = spec_masks(oracle_mod, s.params, st["x"], st["y"], st["active"], st["terminated"], st["truncated"])
    return och


def run_case(oracle_mod, ccx, case, policy="greedy"):
    import torch
    from _placed import assert_guards, place

    from collectivecrossing_amd.batched import RolloutResult
    s = Setup(case)
    c, K, E, N, L = s.c, s.K, s.E, s.N, 6 + 4 * s.N
    tag = (kk.describe(c["key"]), case, policy)
    want = expected(oracle_mod, s, policy)
    drive, _ = kk.DRIVE_NAMES[c["drive"]]
    _actions, has_order, in_kernel, has_ao, mixed = drive
    has_obs, has_rew, _, _, has_cmp, residue = kk.OUTPUTS[c["outputs"]]
    b = s.batch(ccx)
    try:
        def new(shape, dtype):
            t = torch.empty(shape, dtype=dtype, device="cuda")
            t.view(torch.uint8).fill_(SENTINEL)
            return t

        obs = placed = None
        if has_obs:
            obs, placed = place((K, E, N, L), torch.float32, residue)
            assert obs.data_ptr() % 128 == residue
        out = RolloutResult(obs, new((K, E, N), torch.float64) if has_rew else None, new((K, E, N), torch.uint8) if has_rew else None,
                            new((K, E), torch.uint8) if has_rew else None, new((K, E, N, 4), torch.float32) if has_cmp else None,
                            final_obs=new((K, E, N, L), torch.float32) if c["reset"] and has_obs else None,
                            final_compact=new((K, E, N, 4), torch.float32) if c["reset"] and has_cmp else None)
        masks = new((E, N), torch.uint8) if c["masks"] else None
        taken = new((K, E, N), torch.uint8) if has_ao else None
        acts, order = torch.from_numpy(s.actions).cuda(), torch.from_numpy(s.order).cuda() if has_order else None
        kw = dict(auto_reset=True, out=out, masks_out=masks)
        if in_kernel:
            b.rollout_greedy(K, actions_out=taken, want_actions=False, policy=policy, **kw)
        elif mixed:
            every = c["drive"] == "mixed_all_actions_out"
            b.rollout_mixed(None if every else acts, "all" if every else s.mask, policy, order, actions_out=taken,
                            num_steps=K if every else None, **kw)
        else:
            b.rollout(acts, order, reset_obs="next" if c["reset"] else "terminal", **kw)
        b.synchronize()
        # ---- the instantiation that ran ----
        assert last_key(b) == c["key"], ("launched " + kk.describe(last_key(b)), tag)
        # ---- what it wrote ----
        for name, t in (("obs", out.obs), ("reward", out.reward), ("agent_flags", out.agent_flags), ("env_flags", out.env_flags),
                        ("obs_compact", out.obs_compact), ("final_obs", out.final_obs), ("final_compact", out.final_compact),
                        ("actions", taken), ("masks", masks)):
            if t is not None:
                assert np.array_equal(_bits(_np(t)), _bits(want[name])), (name, tag)
        if placed is not None:
            assert_guards(placed, f"obs of {tag}")
        st = b.get_state()
        for f in STATE_KEYS:
            assert np.array_equal(st[f], want["state"][f]), (f, tag)
        assert b.counters() == want["counters"], tag
    finally:
        b.close()


def _cases(kernel, glog, outs=None):
    return [c for c in kk.CASES if c[0][0] == kernel and c[0][1] == glog and (outs is None or c[0][3] in outs)]


def _run_all(oracle, ccx, cases):
    assert cases
    for case in cases:
        policies = ("greedy", "waiting") if "policy" in case[-1] else ("greedy",)
        for policy in policies:
            run_case(oracle, ccx, case, policy)


@pytest.mark.parametrize("outs", [(0, 1), (2, 3)], ids=["out01", "out23"])
@pytest.mark.parametrize("glog", range(7))
def test_every_reachable_rollout_kernel_equals_the_oracle(oracle, ccx, glog, outs):
    _run_all(oracle, ccx, _cases(kk.KERNEL_ROLLOUT, glog, outs))


@pytest.mark.parametrize("glog", range(7))
def test_every_reachable_step_kernel_equals_the_oracle(oracle, ccx, glog):
    _run_all(oracle, ccx, _cases(kk.KERNEL_STEP, glog))


def test_every_reachable_observe_kernel_equals_the_oracle(oracle, ccx):
    """ccx_observe (full rows from the state) and ccx_expand_observations (the same kernel fed compact rows), once per
    (GLOG, PAIR)."""
    import torch
    cases = [c for c in kk.CASES if c[0][0] == kk.KERNEL_OBSERVE]
    assert len(cases) == 12
    for case in cases:
        s = Setup(case)
        ob, b = s.oracle(oracle), s.batch(ccx)
        try:
            assert last_key(b, 1)[0] == -1
            want = ob.observe()
            got = b.observe()
            b.synchronize()
            assert last_key(b, 1) == case[0], (kk.describe(last_key(b, 1)), case)
            assert np.array_equal(_bits(_np(got)), _bits(want)), case
            compact = np.stack([ob.x, ob.y, np.broadcast_to(np.arange(s.N) >= s.params.num_boarding, ob.x.shape), ob.active],
                               -1).astype(np.float32)
            got = b.expand_observations(torch.from_numpy(compact).cuda())
            b.synchronize()
            assert last_key(b, 1) == case[0], case
            assert np.array_equal(_bits(_np(got)), _bits(want)), case
        finally:
            b.close()
