"""Far shards and late episodes on the GPU: every copy of the reset-pool cursor, the three sites that key the counter-based
RNG by the global env index, the finished-episode log's 64-bit env column and the invariance of a global env's trajectory to
how the batch is cut into shards -- at env offsets around 2^31, 2^32 and above 2^40, total_envs above 2^32, a pool of
100 003 entries and episode counters up to 2^31 - 250 (tests/_far_shard_cases.py; test_far_shard_spec.py shows on the CPU
that these cases expose every wrong-width model of the cursor).  Every comparison is on bytes / bit patterns, against the
CPU oracle built from the same env_offset, total_envs, pool and start episodes.  Nothing here is large: E <= 130, K = 38.

The batches are driven by the harness of tests/test_gpu_call_paths.py (every call with auto-reset, reset_obs="next" and
side buffers, bound masks, episode tracking, input checking)."""

import _far_shard_cases as far
import numpy as np
import pytest
from _episode_stats_spec import ACC_KEYS, LOG_KEYS, StatsSpec, bits, sort_log
from _reset_obs_spec import SENTINEL
from _split_step_spec import pool_cursor
from test_gpu_call_paths import CHUNKS, FIELDS, STATS, _alloc, _call, _new

pytestmark = pytest.mark.gpu

K, N = far.K, far.N
ONE = (1,) * K
INT64_MAX = (1 << 63) - 1


@pytest.fixture(scope="module")
def ccx():
    import torch

    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    from collectivecrossing_amd.batched import BatchedCollectiveCrossing

    return BatchedCollectiveCrossing


@pytest.fixture(scope="module")
def pools(ccx):
    """P -> the pool on the device, built there (`make_reset_pool`) and byte-equal to the host pool the oracle uses."""
    b = ccx(far.config(), 4)
    out = {}
    for P in sorted({c.P for c in far.CASES.values()}):
        b.make_reset_pool(far.POOL_SEED, P)
        out[P] = b.reset_pool()
        assert np.array_equal(out[P].cpu().numpy(), far.pool(P)), P
    b.close()
    return out


def _np(t):
    return np.ascontiguousarray(t.cpu().numpy())


def _same(got, want):
    got, want = _np(got) if hasattr(got, "cpu") else np.ascontiguousarray(got), np.ascontiguousarray(want)
    return got.shape == want.shape and got.dtype == want.dtype and got.tobytes() == want.tobytes()


def _start(ccx, pools, case, drive, cut=0, tunables=(), **kw):
    return _new(ccx, far.config(), pools[case.P], drive, cut, E=case.E, env_offset=case.env_offset,
                total_envs=case.total_envs, episode=case.episodes(), tunables=tunables, **kw)


def _drive(b, case, drive, chunks, policy="greedy", with_order=False):
    """The K steps of the case in calls of `chunks` steps -> (result, actions_out, masks)."""
    import torch
    acts, orders = (torch.from_numpy(a).cuda() for a in far.inputs(case.name))
    res, masks = _alloc(b, K), torch.zeros((case.E, N), dtype=torch.uint8, device="cuda")
    acts_out = torch.full((K, case.E, N), SENTINEL, dtype=torch.uint8, device="cuda")
    s0 = 0
    for k in chunks:
        k = min(k, K - s0)
        _call(b, drive, res, acts_out, masks, acts, orders, s0, s0 + k, policy)
        s0 += k
    assert s0 == K
    b.check_inputs()
    return res, acts_out, masks


def _assert_reference(b, res, ref, tag):
    for f in FIELDS:
        assert _same(getattr(res, f), getattr(ref, f)), (tag, f)
    state = b.get_state()
    for f in ref.state:
        assert np.array_equal(state[f], ref.state[f]), (tag, f)
    assert b.counters() == ref.counters, tag


# --------------------------------------------------------------------------------------- every copy of the cursor
@pytest.mark.parametrize("name", list(far.CASES))
def test_reset_from_pool_lands_on_the_cursor(ccx, pools, oracle, name):
    """ccx_kernels.hip (reset_from_pool), without and with a mask: against the cursor in Python integers and the oracle."""
    c = far.CASES[name]
    pool, ep = far.pool(c.P), c.episodes()
    b = ccx(far.config(), c.E, env_offset=c.env_offset, total_envs=c.total_envs)
    b.set_reset_pool(pools[c.P])
    b.set_state(episode=ep)
    b.reset_from_pool()
    b.set_state(step_count=c.step_counts())          # (a masked restart clears the counters of the envs it restarts only)
    ob = far.new_oracle(c)
    want = np.stack([pool[pool_cursor(c.env_offset, c.total_envs, c.P, e, int(ep[e]))] for e in range(c.E)])
    st = b.get_state()
    assert np.array_equal(st["x"], want[..., 0]) and np.array_equal(st["y"], want[..., 1])
    assert np.array_equal(st["x"], ob.x) and np.array_equal(st["y"], ob.y)
    mask = (np.arange(c.E) % 3 != 1).astype(np.uint8)
    for batch in (b, ob):
        batch.set_state(episode=ep + 3)
        batch.reset_from_pool(mask)
    later = np.stack([pool[pool_cursor(c.env_offset, c.total_envs, c.P, e, int(ep[e]) + 3)] for e in range(c.E)])
    want = np.where(mask[:, None, None] != 0, later, want)
    st = b.get_state()
    assert np.array_equal(st["x"], want[..., 0]) and np.array_equal(st["y"], want[..., 1])
    assert all(np.array_equal(st[k], getattr(ob, k)) for k in st)
    b.close()


# what runs a case's K steps -> which copy of the cursor places the restarted envs and writes their rows
PATHS = {
    # ccx_step.hip: one-step launches of the step kernel, the restarted rows from the same launch
    "step_kernel_fused": dict(chunks=ONE, tunables=(("step_kernel", 1),), fused=True, step_ok=1),
    # ... and from the stand-alone fix-up kernel (ccx_reset_obs.hip), one step per launch
    "step_kernel_fixup": dict(chunks=ONE, tunables=(("step_kernel", 1), ("reset_obs_fused", 0)), fused=False, step_ok=1),
    # the step kernel's launches of up to 16 steps; the fix-up kernel derives the ordinals of several restarts per launch
    "step_kernel_chunks": dict(chunks=CHUNKS, tunables=(("step_kernel", 1),), step_ok=1),
    # ccx_rollout_body.inc: the rollout kernel takes the one-step launches (closed form at every launch)
    "rollout_kernel_steps": dict(chunks=ONE, tunables=(("step_kernel", 0),), fused=False, step_ok=0),
    # the whole call in one launch: the incremental walk over 7+ restarts
    "rollout_kernel_whole": dict(chunks=(K,), tunables=(("step_kernel", 0),), step_ok=0),
    # cut into launches of 7 steps: the closed form restarts mid-walk and must land where the walk stood
    "rollout_kernel_cut7": dict(chunks=(K,), cut=7, tunables=(("step_kernel", 0),), step_ok=0),
    "rollout_kernel_order_cut7": dict(chunks=(K,), cut=7, drive="order"),
}


@pytest.mark.parametrize("path", list(PATHS))
@pytest.mark.parametrize("name", list(far.CASES))
def test_auto_reset_lands_on_the_cursor_on_every_path(ccx, pools, oracle, name, path):
    c, p = far.CASES[name], PATHS[path]
    drive = p.get("drive", "tensor")
    ref = far.tensor_reference(name, drive == "order")
    assert int(((ref.env_flags & 0x04) != 0).sum(0).min()) >= far.RESTARTS
    b = _start(ccx, pools, c, drive, p.get("cut", 0), p.get("tunables", ()))
    if "step_ok" in p:
        assert b.step_shape()["ok"] == p["step_ok"]
    if "fused" in p:
        assert b.reset_obs_fused() == p["fused"]
    res, _, masks = _drive(b, c, drive, p["chunks"])
    _assert_reference(b, res, ref, (name, path))
    import torch
    assert torch.equal(masks, b.action_masks())
    b.close()


@pytest.mark.parametrize("name", list(far.CASES))
def test_step_finish_lands_on_the_cursor(ccx, pools, oracle, name):
    """ccx_split_step.hip (step_finish with auto-reset; reset_obs="next" through the fix-up kernel, one step per call)."""
    import torch
    c = far.CASES[name]
    ref = far.tensor_reference(name)
    b = _start(ccx, pools, c, "tensor")
    acts = torch.from_numpy(far.inputs(name)[0]).cuda()
    for s in range(K):
        b.step_begin(acts[s])
        for t in b.step_final_buffers(want_obs=True, want_compact=True):
            t.view(torch.uint8).fill_(SENTINEL)
        r = b.step_finish(auto_reset=True, want_compact=True, reset_obs="next", want_final=True)
        for f in FIELDS:
            assert _same(getattr(r, f), getattr(ref, f)[s]), (name, s, f)
    state = b.get_state()
    assert all(np.array_equal(state[f], ref.state[f]) for f in ref.state) and b.counters() == ref.counters
    b.close()


# --------------------------------------------------------------------------------------- the RNG key's low word
RNG_CASES = ("cross32", "far40")       # env 29 of cross32 is global env 2^32: the key's low word wraps inside a tile


def _explore(b):
    b.set_rng_seed(far.RNG_SEED)
    b.set_policy_epsilon(far.EPSILON)


def _assert_draws_on_both_sides(c, acts, acts0, sel=slice(None)):
    """Step 0 starts from the same state with and without epsilon: a differing action there IS an exploration draw."""
    d = (acts[0] != acts0[0])[:, sel].any(axis=1)
    wrap = (1 << 32) - c.env_offset
    if 0 < wrap < c.E:
        assert d[:wrap].any() and d[wrap:].any(), (c.name, int(d[:wrap].sum()), int(d[wrap:].sum()))
    else:
        assert d.any(), c.name


@pytest.mark.parametrize("policy", ["greedy", "waiting"])
@pytest.mark.parametrize("name", RNG_CASES)
def test_policy_rollout_draws_by_the_low_word_of_the_global_env(ccx, pools, oracle, name, policy):
    """ccx_rollout_body.inc (genv): rollout_policy whole and as consecutive calls."""
    c = far.CASES[name]
    ref = far.policy_reference(name, policy)
    _assert_draws_on_both_sides(c, ref.actions, far.policy_reference(name, policy, 0.0).actions)
    for chunks in ((K,), CHUNKS):
        b = _start(ccx, pools, c, "greedy")
        _explore(b)
        res, acts_out, _ = _drive(b, c, "greedy", chunks, policy)
        assert _same(acts_out, ref.actions), (name, policy, chunks)
        _assert_reference(b, res, ref, (name, policy, chunks))
        b.close()


@pytest.mark.parametrize("drive", ["mixed", "mixed_unfused"])
@pytest.mark.parametrize("name", RNG_CASES)
def test_mixed_rollout_draws_by_the_low_word_of_the_global_env(ccx, pools, oracle, name, drive):
    """ccx_step.hip (genv0: the step kernel's policy instantiations) and, unfused, ccx_policy.hip + the rollout kernel."""
    c = far.CASES[name]
    policy = "greedy" if drive == "mixed" else "waiting"
    ref = far.mixed_reference(name, policy)
    exiting = np.arange(N) >= far.params().num_boarding
    _assert_draws_on_both_sides(c, ref.actions, far.mixed_reference(name, policy, 0.0).actions, exiting)
    b = _start(ccx, pools, c, drive)
    assert b.step_shape()["ok"] == (1 if drive == "mixed" else 0)
    _explore(b)
    res, acts_out, _ = _drive(b, c, drive, CHUNKS, policy)
    assert _same(acts_out, ref.actions), (name, drive)
    _assert_reference(b, res, ref, (name, drive))
    b.close()


@pytest.mark.parametrize("policy", ["greedy", "waiting"])
@pytest.mark.parametrize("name", RNG_CASES)
def test_policy_actions_draw_by_the_low_word_of_the_global_env(ccx, pools, oracle, name, policy):
    """ccx_policy.hip: policy_actions with epsilon on the states of the first steps of the oracle's policy run."""
    import torch
    c = far.CASES[name]
    ref = far.policy_reference(name, policy)
    b = _start(ccx, pools, c, "tensor")
    b.set_check_inputs(False)   # (the policy's own actions go back in: 255 for agents that are done)
    _explore(b)
    for s in range(8):         # (the run restarts envs from step 0 on: the episode word of the key changes too)
        assert _same(b.policy_actions(policy), ref.actions[s]), (name, policy, s)
        b.rollout(torch.from_numpy(ref.actions[s][None]).cuda(), auto_reset=True)
    b.set_policy_epsilon(0.0)
    b.close()


# --------------------------------------------------------------------------------------- shard invariance
SHARD_LO, SHARD_E = (1 << 32) - 40, 80
SPLITS = ((80,), (40, 40), (13, 67))          # (40, 40): the shards meet exactly at global env 2^32


def test_a_global_env_does_not_depend_on_the_shards(ccx, pools):
    """The global envs [2^32 - 40, 2^32 + 40) as one shard, two shards meeting at 2^32, and shards of 13 and 67: a policy
    rollout with exploration, auto-reset, reset_obs="next" and episode statistics gives the same bytes for every global
    env.  No oracle involved."""
    import torch
    P, total = far.P_BIG, far.T_STRIDE_PM1
    runs = []
    for split in SPLITS:
        parts, lo = [], SHARD_LO
        for E in split:
            ep = (far.EP_BIG_RESIDUE + (lo + np.arange(E)) % 5).astype(np.int32)
            b = _new(ccx, far.config(), pools[P], "greedy", E=E, env_offset=lo, total_envs=total, episode=ep)
            b.track_episodes(4096)
            _explore(b)
            res, acts_out = _alloc(b, K), torch.full((K, E, N), SENTINEL, dtype=torch.uint8, device="cuda")
            masks = torch.zeros((E, N), dtype=torch.uint8, device="cuda")
            _call(b, "greedy", res, acts_out, masks, None, None, 0, K)
            st, es = b.get_state(), b.episode_stats()
            part = {f: _np(getattr(res, f)) for f in FIELDS}                         # [K, E, ...]: env axis 1
            part.update(actions=_np(acts_out))
            per_env = {f"state_{k}": v for k, v in st.items()}                       # [E, ...]: env axis 0
            per_env.update({f"stats_{f}": _np(getattr(es, f)) for f in STATS}, masks=_np(masks))
            log = b.finished_episodes()
            assert log.dropped == 0
            parts.append((part, per_env, {k: getattr(log, k) for k in LOG_KEYS}, b.counters()))
            b.close()
            lo += E
        assert lo == SHARD_LO + SHARD_E
        whole = {k: np.concatenate([p[0][k] for p in parts], axis=1) for k in parts[0][0]}
        whole.update({k: np.concatenate([p[1][k] for p in parts], axis=0) for k in parts[0][1]})
        log = sort_log({k: np.concatenate([p[2][k] for p in parts], axis=0) for k in LOG_KEYS})
        counters = {k: sum(p[3][k] for p in parts) for k in parts[0][3]}
        runs.append((split, whole, log, counters))
    _, wA, lA, cA = runs[0]
    assert int(((wA["env_flags"] & 0x04) != 0).sum(0).min()) >= far.RESTARTS
    assert len(lA["env"]) > 0 and lA["env"].min() == SHARD_LO and lA["env"].max() == SHARD_LO + SHARD_E - 1
    for split, w, log, counters in runs[1:]:
        for k in wA:
            assert w[k].tobytes() == wA[k].tobytes(), (split, k)
        for k in LOG_KEYS:
            assert bits(log[k]).tobytes() == bits(lA[k]).tobytes(), (split, k)
        assert counters == cA, split


# --------------------------------------------------------------------------------------- the finished-episode log
@pytest.mark.parametrize("name", ["far40", "cross32"])
def test_the_episode_log_holds_64_bit_global_env_indices(ccx, pools, oracle, name):
    """ccx_episode_stats.hip: log_env = env_offset + e as i64; returns and lengths as tests/_episode_stats_spec.py has them."""
    c = far.CASES[name]
    ref = far.tensor_reference(name)
    spec = StatsSpec(c.E, N, 4096, env_offset=c.env_offset)
    spec.update(ref.reward, ref.agent_flags, ref.env_flags)
    b = _start(ccx, pools, c, "tensor")
    b.track_episodes(4096)
    res, _, _ = _drive(b, c, "tensor", CHUNKS)
    assert _same(res.reward, ref.reward) and _same(res.env_flags, ref.env_flags)
    got = b.finished_episodes()
    assert got.env.dtype == np.int64 and got.dropped == 0 and len(got) == spec.emitted >= far.RESTARTS * c.E
    assert set(got.env.tolist()) == set(range(c.env_offset, c.env_offset + c.E))
    want = sort_log(spec.log())
    have = sort_log({k: getattr(got, k) for k in LOG_KEYS})
    for k in LOG_KEYS:
        assert bits(have[k]).tobytes() == bits(want[k]).tobytes(), (name, k)
    es = b.episode_stats()
    for k in ACC_KEYS:
        assert bits(_np(getattr(es, k))).tobytes() == bits(spec.accumulators()[k]).tobytes(), (name, k)
    b.close()


# --------------------------------------------------------------------------------------- ccx_create's range check
def test_the_last_shard_below_int64_max_is_accepted(ccx, pools):
    """env_offset = INT64_MAX - 4 with 4 envs of INT64_MAX: in range (the refusals are in test_far_shard_spec.py), and
    the cursor holds up there."""
    off, total, P = INT64_MAX - 4, INT64_MAX, far.P_BIG
    b = ccx(far.config(), 4, env_offset=off, total_envs=total)
    b.set_reset_pool(pools[P])
    ep = np.array([0, 1, far.EP_BIG_RESIDUE, far.EP_LATE], np.int32)
    b.set_state(episode=ep)
    b.reset_from_pool()
    want = np.stack([far.pool(P)[pool_cursor(off, total, P, e, int(ep[e]))] for e in range(4)])
    st = b.get_state()
    assert np.array_equal(st["x"], want[..., 0]) and np.array_equal(st["y"], want[..., 1])
    b.close()
