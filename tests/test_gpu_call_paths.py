"""Every stepping entry point with all the per-call extras at once -- auto-reset, reset_obs="next" with side buffers, bound
masks, episode tracking, input checking -- run whole, cut into sub-launches (tunable max_launch_steps) and as consecutive
calls: the three must leave the same bytes everywhere.  An env's trajectory does not depend on how its steps are grouped
into calls and launches, so every comparison is bitwise (integer views)."""

import numpy as np
import pytest
from _reset_obs_spec import POOL_SIZE, SENTINEL, make_config

pytestmark = pytest.mark.gpu

E, K, MAX_STEPS = 67, 38, 5
CHUNKS = (1, 16, 5, 16)            # batch C: a fused single step, a full short launch, a short one, a full one
DRIVES = ("tensor", "order", "greedy", "mixed", "mixed_unfused", "mt")
FIELDS = ("obs", "obs_compact", "final_obs", "final_compact", "reward", "agent_flags", "env_flags")
STATS = ("ret", "live_steps", "steps", "closed", "finished", "last_ret", "last_live_steps", "last_steps", "last_end")


@pytest.fixture(scope="module")
def ccx():
    import torch

    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    from collectivecrossing_amd.batched import BatchedCollectiveCrossing

    return BatchedCollectiveCrossing


def _new(ccx, cfg, pool, drive, max_launch_steps=0, E=E, env_offset=0, total_envs=None, episode=None, tunables=()):
    """A batch at the start of a case.  The harness serves other test files too (tests/test_gpu_far_shards.py): a shard of
    `E` envs at `env_offset` of `total_envs`, start episode counters `episode` (set before the placement, which depends on
    them), further `tunables` as (name, value) pairs.  The step counters are staggered by GLOBAL env index."""
    b = ccx(cfg, E, env_offset=env_offset, total_envs=total_envs)
    b.set_reset_pool(pool)
    if episode is not None:
        b.set_state(episode=episode)
    b.reset_from_pool()
    b.set_state(step_count=((env_offset + np.arange(E)) % MAX_STEPS).astype(np.int32))     # restarts on every step of a launch
    b.track_episodes()
    b.set_check_inputs(True)
    if drive == "mixed_unfused":
        b.set_tunable("step_kernel", 0)
    if drive == "mt":                 # the only drive with exploration: the MT19937 stream is keyed per env, not per launch
        b.set_policy_stream("mt19937", seeds=np.arange(E) + 11)
        b.set_policy_epsilon(0.3)
    if max_launch_steps:
        b.set_tunable("max_launch_steps", max_launch_steps)
    for name, value in tunables:
        b.set_tunable(name, value)
    return b


def _alloc(b, k):
    import torch
    out = b.alloc_rollout(k, True, True, want_final=True)
    out.final_obs.view(torch.uint8).fill_(SENTINEL)
    out.final_compact.view(torch.uint8).fill_(SENTINEL)
    return out


def _call(b, drive, res, acts_out, masks, acts, orders, s0, s1, policy="greedy"):
    """Steps s0 .. s1 of the case into res[s0:s1].  A slice whose observation rows do not start on 16 bytes (odd E x N, odd
    s0) is refused by the library by design: such a call goes into buffers of its own and is copied into the slice."""
    from collectivecrossing_amd.batched import RolloutResult
    sl, k = slice(s0, s1), s1 - s0
    dst = RolloutResult(res.obs[sl], res.reward[sl], res.agent_flags[sl], res.env_flags[sl], res.obs_compact[sl],
                        final_obs=res.final_obs[sl], final_compact=res.final_compact[sl])
    out = dst if dst.obs.data_ptr() % 16 == 0 else _alloc(b, k)
    kw = dict(auto_reset=True, out=out, masks_out=masks, reset_obs="next")
    if drive in ("tensor", "order"):
        b.rollout(acts[sl], orders[sl] if drive == "order" else None, **kw)
    elif drive in ("greedy", "mt"):
        b.rollout_greedy(k, actions_out=acts_out[sl], policy=policy, **kw)
    else:
        b.rollout_mixed(acts[sl], "exiting", policy, actions_out=acts_out[sl], **kw)
    if out is not dst:
        for f in FIELDS:
            getattr(dst, f).copy_(getattr(out, f))


def _bits(t):
    import torch
    return t.contiguous().view(torch.uint8)


@pytest.mark.parametrize("N", [5, 8])
@pytest.mark.parametrize("drive", DRIVES)
def test_whole_cut_and_consecutive_calls_leave_the_same_bytes(ccx, drive, N):
    import torch

    from collectivecrossing_amd.reset import build_reset_pool
    cfg = make_config(N, MAX_STEPS)
    pool = build_reset_pool(cfg, 7, POOL_SIZE)
    rng = np.random.default_rng(1000 * N + DRIVES.index(drive))
    acts = torch.from_numpy(rng.integers(0, 5, size=(K, E, N), dtype=np.uint8)).cuda()
    orders = torch.from_numpy(np.argsort(rng.random((K, E, N)), axis=-1).astype(np.uint8)).cuda()
    runs = []
    for name, cut, chunks in (("A", 0, (K,)), ("B", 7, (K,)), ("C", 0, CHUNKS)):
        b = _new(ccx, cfg, pool, drive, cut)
        res, masks = _alloc(b, K), torch.zeros((E, N), dtype=torch.uint8, device="cuda")
        acts_out = torch.full((K, E, N), SENTINEL, dtype=torch.uint8, device="cuda")
        s0 = 0
        for k in chunks:
            _call(b, drive, res, acts_out, masks, acts, orders, s0, s0 + k)
            s0 += k
        assert s0 == K
        b.check_inputs()                                            # raises nothing: every input was valid
        state, counters = b.get_state(), b.counters()
        assert torch.equal(masks, b.action_masks()), name
        runs.append((name, b, res, acts_out, masks, state, counters))
    _, bA, rA, aA, mA, sA, cA = runs[0]
    assert int((rA.env_flags & 0x04).ne(0).sum(0).min()) >= 3      # several restarts of every env within the call
    for name, b, res, acts_out, masks, state, counters in runs[1:]:
        for f in FIELDS:
            assert torch.equal(_bits(getattr(res, f)), _bits(getattr(rA, f))), (name, f)
        if drive not in ("tensor", "order"):
            assert torch.equal(acts_out, aA), name
        assert all(np.array_equal(state[f], sA[f]) for f in sA), name
        assert counters == cA, name
        assert torch.equal(masks, mA), name
        ea, eb = bA.episode_stats(), b.episode_stats()
        for f in STATS:
            assert torch.equal(_bits(getattr(eb, f)), _bits(getattr(ea, f))), (name, f)
    for run in runs:
        run[1].close()


def test_an_odd_slab_is_not_cut_into_single_steps(ccx):
    """E x N odd: one step's observation slab is 8 bytes short of a multiple of 16, a cut at every step is refused before
    anything is launched."""
    import torch

    from collectivecrossing_amd._lib import CcxError
    from collectivecrossing_amd.reset import build_reset_pool
    cfg = make_config(5, MAX_STEPS)
    b = _new(ccx, cfg, build_reset_pool(cfg, 7, POOL_SIZE), "tensor", 1)
    acts = torch.zeros((2, E, 5), dtype=torch.uint8, device="cuda")
    before = b.get_state()
    with pytest.raises(CcxError, match="cannot be cut into launches of one step"):
        b.rollout(acts, auto_reset=True, out=_alloc(b, 2), reset_obs="next")
    after = b.get_state()
    assert all(np.array_equal(before[f], after[f]) for f in before)
    b.close()
