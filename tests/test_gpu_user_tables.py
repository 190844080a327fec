"""Position-only user tables (ccx_set_reward_table / ccx_set_terminated_table) under every feature that reads the bits they
change: legal-action masks, reset_obs="next" with side buffers, scripted and mixed control, episode statistics, cut
launches and consecutive calls.  A terminated table produces agents that are ACTIVE AND TERMINATED (they block, are not
live, may only wait) and agents that are INACTIVE AND NOT TERMINATED; a reward table shifts the step kernel's occupancy
tables in the LDS.  tests/test_user_tables_spec.py shows on the CPU that the cases of tests/_user_table_cases.py reach these.

Every comparison is bitwise (u32 / u64 views) against the CPU oracle with the same tables plus the NumPy specs of the
features (tests/_reset_obs_spec.next_mode, tests/_action_masks.spec_masks, tests/_episode_stats_spec.StatsSpec)."""

import numpy as np
import pytest
from _action_masks import spec_masks
from _episode_stats_spec import LOG_KEYS, StatsSpec, bits, sort_log
from _reset_obs_spec import SENTINEL
from _user_table_cases import DROP_WAVES, PLANNER_PAIR, RNG_SEED, STATE_KEYS, TableCase, make_tables, names

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ccx():
    import torch

    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    from collectivecrossing_amd.batched import BatchedCollectiveCrossing

    return BatchedCollectiveCrossing


def _np(t):
    return t.cpu().numpy()


def _u32(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _install(b, tables):
    reward, term = tables
    b.set_reward_table(*(reward or (None, None)))
    b.set_terminated_table(*(term or (None, None)))


def _new(ccx, case):
    b = ccx(case.config, case.E, env_offset=case.env_offset, total_envs=case.total_envs)
    b.set_reset_pool(case.pool)
    b.reset_from_pool()
    b.set_state(step_count=case.step_count0)
    b.track_episodes(case.log)
    b.set_check_inputs(True)
    if case.unfused:
        b.set_tunable("step_kernel", 0)
    if case.cut:
        b.set_tunable("max_launch_steps", case.cut)
    if case.drive == "greedy" and case.eps > 0:
        b.set_policy_stream("mt19937", seeds=case.mt_seeds)
        b.set_policy_epsilon(case.eps)
    if case.drive == "mixed":
        b.set_rng_seed(RNG_SEED)
        b.set_policy_epsilon(case.eps)
    _install(b, case.tables)
    return b


def _launch(b, drive, k, actions, order, masks, policy="greedy"):
    """One auto-reset launch with every per-call extra: NEXT-mode rows, side buffers prefilled with SENTINEL, bound masks.
    Returns the result and the actions the steps took (None for a tensor drive)."""
    import torch
    out = b.alloc_rollout(k, True, True, want_final=True)
    out.final_obs.view(torch.uint8).fill_(SENTINEL)
    out.final_compact.view(torch.uint8).fill_(SENTINEL)
    kw = dict(auto_reset=True, out=out, masks_out=masks, reset_obs="next")
    acts = None if actions is None else torch.from_numpy(actions).cuda()
    taken = None
    if drive == "greedy":
        taken = torch.full((k, b.num_envs, b.num_agents), SENTINEL, dtype=torch.uint8, device="cuda")
        b.rollout_greedy(k, actions_out=taken, policy=policy, **kw)
    elif drive == "mixed":
        taken = torch.full((k, b.num_envs, b.num_agents), SENTINEL, dtype=torch.uint8, device="cuda")
        b.rollout_mixed(acts, "exiting", policy, None if order is None else torch.from_numpy(order).cuda(), actions_out=taken,
                        want_compact=True, **kw)
    else:
        b.rollout(acts, None if order is None else torch.from_numpy(order).cuda(), want_compact=True, **kw)
    return out, taken


def _assert_launch(oracle, case, b, out, taken, masks, och, stats, tag):
    """Everything a launch leaves against the oracle's launch `och`: rows, compact rows and side buffers against next_mode,
    reward, flags, the actions taken, state, counters, the masks of the state behind it, the episode statistics."""
    s_obs, s_cmp, s_fo, s_fc, s_ep = case.spec(och)
    for what, got, exp in (("obs", out.obs, s_obs), ("final_obs", out.final_obs, s_fo), ("obs_compact", out.obs_compact, s_cmp),
                           ("final_compact", out.final_compact, s_fc)):
        assert np.array_equal(_u32(_np(got)), _u32(exp)), (tag, what)
    assert np.array_equal(_np(out.reward).view(np.uint64), och["reward"].view(np.uint64)), (tag, "reward")
    assert np.array_equal(_np(out.agent_flags), och["agent_flags"]), (tag, "agent_flags")
    assert np.array_equal(_np(out.env_flags), och["env_flags"]), (tag, "env_flags")
    if taken is not None:
        assert np.array_equal(_np(taken), och["actions"]), (tag, "actions_out")
    st = b.get_state()
    for f in STATE_KEYS:
        assert np.array_equal(st[f], och["state"][f]), (tag, f)
    assert np.array_equal(st["episode"], s_ep), tag
    assert b.counters() == och["counters"], tag
    o = och["state"]
    exp_masks = spec_masks(oracle, case.params, o["x"], o["y"], o["active"], o["terminated"], o["truncated"])
    assert np.array_equal(_np(masks), exp_masks), (tag, "masks")
    if stats is not None:
        stats.update(och["reward"], och["agent_flags"], och["env_flags"])
        got = b.episode_stats()
        b.synchronize()
        for k, exp in stats.accumulators().items():
            assert np.array_equal(bits(_np(getattr(got, k))), bits(exp)), (tag, "stats", k)


def _run_case(ccx, oracle, name, check=None):
    import torch
    case = TableCase(name)
    chunks = case.run_oracle(oracle)
    b = _new(ccx, case)
    if check is not None:
        check(case, b)
    masks = torch.zeros((case.E, case.N), dtype=torch.uint8, device="cuda")
    stats = StatsSpec(case.E, case.N, case.log, case.env_offset)
    for q, k in enumerate(case.chunks):
        out, taken = _launch(b, case.drive, k, case.actions[q], case.orders[q], masks, case.policy)
        _assert_launch(oracle, case, b, out, taken, masks, chunks[q], stats, (name, q))
    b.check_inputs()
    return case, b, stats


# ------------------------------------------------------------------------------------------- (a) fused one-step extras
@pytest.mark.parametrize("name", names("a"))
def test_fused_single_steps_equal_the_oracle_and_the_specs(ccx, oracle, name):
    def fused(case, b):
        assert b.step_shape()["ok"] == 1 and b.masks_fused(1) and b.reset_obs_fused(1)

    _, b, _ = _run_case(ccx, oracle, name, fused)
    b.close()


# ------------------------------------------------------------------------------------------- (b) the unfused kernels
@pytest.mark.parametrize("name", names("b"))
def test_unfused_paths_equal_the_oracle_and_the_specs(ccx, oracle, name):
    def unfused(case, b):
        k_max = max(case.chunks)
        assert not b.masks_fused(k_max, order=case.order) or k_max == 1
        if case.unfused or case.big:
            assert b.step_shape()["ok"] == 0 and not b.masks_fused(1) and not b.reset_obs_fused(1)
        if case.order:
            assert not b.masks_fused(1, order=True) and not b.reset_obs_fused(1, order=True)

    _, b, _ = _run_case(ccx, oracle, name, unfused)
    b.close()


# ------------------------------------------------------------------------------------------- (c) scripted and mixed control
@pytest.mark.parametrize("name", names("c"))
def test_scripted_and_mixed_control_equal_the_oracle(ccx, oracle, name):
    case, b, _ = _run_case(ccx, oracle, name)
    assert (b.step_shape()["ok"] == 0) == case.unfused
    b.close()


# ------------------------------------------------------------------------------------------- (d) episode statistics
@pytest.mark.parametrize("name", names("d"))
def test_episode_statistics_equal_the_spec_on_the_oracles_arrays(ccx, oracle, name):
    case, b, stats = _run_case(ccx, oracle, name)
    rec = b.finished_episodes(clear=False)
    got, want = {k: getattr(rec, k) for k in LOG_KEYS}, stats.log()
    assert rec.dropped == stats.dropped == 0 and len(want["env"]) == stats.emitted > case.E
    for k in LOG_KEYS:                                            # the exact, env-major order of every update
        assert np.array_equal(bits(got[k]), bits(want[k])), (name, "log", k)
    got, want = sort_log(got), sort_log(want)
    assert np.array_equal(bits(got["ret"]), bits(want["ret"]))
    # the returns are sums of arbitrary f64 values: some would change with the order of the additions
    ret = want["ret"][want["live_steps"] >= 3]
    assert len(ret) > 20 and (np.abs(ret) > 0).any()
    b.close()


# ------------------------------------------------------------------------------------------- (e) whole / cut / consecutive
@pytest.mark.parametrize("name", names("e"))
def test_whole_cut_and_consecutive_calls_with_tables(ccx, oracle, name):
    """The three-way comparison of tests/test_gpu_call_paths.py (its harness, batch size, steps and input seeds) with the
    `sparse` tables installed: the same bytes everywhere, and run A equal to the oracle."""
    import torch
    from test_gpu_call_paths import CHUNKS, DRIVES, FIELDS, MAX_STEPS, STATS, E, K, _alloc, _bits, _call
    from test_gpu_call_paths import _new as _new_call
    case = TableCase(name)
    drive, N = name.split("_")[1], case.N
    assert (case.E, case.chunks, case.max_steps, case.input_seed) == (E, [K], MAX_STEPS, 1000 * N + DRIVES.index(drive))
    acts, orders = torch.from_numpy(case.actions[0]).cuda(), torch.from_numpy(case.drawn_orders[0]).cuda()
    runs = []
    for run, cut, chunks in (("A", 0, (K,)), ("B", 7, (K,)), ("C", 0, CHUNKS)):
        b = _new_call(ccx, case.config, case.pool, drive, cut)
        _install(b, case.tables)
        res, masks = _alloc(b, K), torch.zeros((E, N), dtype=torch.uint8, device="cuda")
        acts_out = torch.full((K, E, N), SENTINEL, dtype=torch.uint8, device="cuda")
        s0 = 0
        for k in chunks:
            _call(b, drive, res, acts_out, masks, acts, orders, s0, s0 + k)
            s0 += k
        b.check_inputs()
        assert torch.equal(masks, b.action_masks()), run
        runs.append((run, b, res, acts_out, masks, b.get_state(), b.counters()))
    _, bA, rA, aA, mA, sA, cA = runs[0]
    for run, b, res, acts_out, masks, state, counters in runs[1:]:
        for f in FIELDS:
            assert torch.equal(_bits(getattr(res, f)), _bits(getattr(rA, f))), (run, f)
        if drive not in ("tensor", "order"):
            assert torch.equal(acts_out, aA), run
        assert all(np.array_equal(state[f], sA[f]) for f in sA), run
        assert counters == cA and torch.equal(masks, mA), run
        ea, eb = bA.episode_stats(), b.episode_stats()
        for f in STATS:
            assert torch.equal(_bits(getattr(eb, f)), _bits(getattr(ea, f))), (run, f)
    och = case.run_oracle(oracle)[0]
    assert int(((och["env_flags"] & 0x04) != 0).sum(0).min()) >= 3      # several restarts of every env within the call
    _assert_launch(oracle, case, bA, rA, None if drive in ("tensor", "order") else aA, mA, och, StatsSpec(E, N), (name, "A"))
    for run in runs:
        run[1].close()


# ------------------------------------------------------------------------------------------- (f) switching tables
@pytest.mark.parametrize("grid", PLANNER_PAIR)
def test_tables_switch_on_a_live_handle(ccx, oracle, grid):
    """sparse -> none -> dense -> reward_only in the middle of episodes, masks bound and tracking on, on both sides of the
    planner's boundary: with a reward table the larger grid's short launches leave the step kernel, without one they
    come back.  The oracle does the same switches."""
    import torch
    case = TableCase(f"f_switch_{grid[0]}x{grid[1]}")
    chunks = case.run_oracle(oracle)
    b = _new(ccx, case)
    masks = torch.zeros((case.E, case.N), dtype=torch.uint8, device="cuda")
    stats = StatsSpec(case.E, case.N)
    ok = []
    for q, k in enumerate(case.chunks):
        if q % 2 == 0:
            _install(b, case.tables_of_launch(q))
            ok.append(b.step_shape()["ok"])
        out, _ = _launch(b, "tensor", k, case.actions[q], None, masks)
        _assert_launch(oracle, case, b, out, None, masks, chunks[q], stats, (grid, case.switches[q // 2], q))
    assert ok == ([1, 1, 1, 1] if grid == PLANNER_PAIR[0] else [0, 1, 0, 0])
    assert stats.finished.min() >= 1
    b.close()


def test_a_refused_reward_table_leaves_the_built_in_reward(ccx, oracle):
    """100 x 100: a reward table does not fit and is refused; the handle then runs the built-in reward next to the
    terminated table set before, like the oracle."""
    import torch

    from collectivecrossing_amd._lib import CcxError
    case = TableCase("f_refused_big_n3")
    chunks = case.run_oracle(oracle)
    b = _new(ccx, case)
    reward, _ = make_tables("sparse", case.config)
    before = b.get_state()
    with pytest.raises(CcxError, match="does not fit"):
        b.set_reward_table(*reward)
    after = b.get_state()
    assert all(np.array_equal(before[f], after[f]) for f in before)
    masks = torch.zeros((case.E, case.N), dtype=torch.uint8, device="cuda")
    stats = StatsSpec(case.E, case.N)
    for q, k in enumerate(case.chunks):
        out, _ = _launch(b, "tensor", k, case.actions[q], None, masks)
        _assert_launch(oracle, case, b, out, None, masks, chunks[q], stats, ("refused", q))
    b.close()


def test_a_refusal_drops_the_reward_table_the_handle_held(ccx, oracle):
    """A handle that HOLDS a reward table (it fits the default launch shape), is given two sim waves per workgroup and is
    then refused the same table (tests/test_user_tables_spec.py shows both from the planner): the library frees the table it
    held and plans again without one.  Nothing is launched between the shape change and the refusal.  Behind it: the step
    shape of a handle that never had a reward table, and the oracle's bytes with the built-in reward and the terminated table."""
    import torch

    from collectivecrossing_amd._lib import CcxError
    case = TableCase("f_dropped_84x62_n33")
    chunks = case.run_oracle(oracle)
    b = _new(ccx, case)
    masks = torch.zeros((case.E, case.N), dtype=torch.uint8, device="cuda")
    stats = StatsSpec(case.E, case.N)
    for q, k in enumerate(case.chunks):
        if q == 2:
            b.set_launch_shape(waves_per_block=DROP_WAVES)
            with pytest.raises(CcxError, match="does not fit"):
                b.set_reward_table(*case.tables[0])
            twin = ccx(case.config, case.E)
            twin.set_launch_shape(waves_per_block=DROP_WAVES)
            twin.set_terminated_table(*case.tables[1])
            assert b.step_shape() == twin.step_shape() and b.launch_shape() == twin.launch_shape()
            twin.close()
        out, _ = _launch(b, "tensor", k, case.actions[q], None, masks)
        _assert_launch(oracle, case, b, out, None, masks, chunks[q], stats, ("dropped", q))
    b.close()
