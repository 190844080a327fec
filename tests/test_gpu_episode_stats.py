"""Episode returns and lengths on the device (include/ccx.h: CCX_EPISODE_STATS) against the NumPy spec
(tests/_episode_stats_spec.py): recorded fixtures, cut invariance, adversarial synthetic trajectories across the kernel's
chunk boundaries, log overflow, the public API on twin batches, and a captured graph.  f64 values are compared as bit
patterns throughout."""

import numpy as np
import pytest
from _episode_stats_spec import ACC_KEYS, LOG_KEYS, StatsSpec, bits, make_trajectory, sort_log
from _fixtures import Golden

pytestmark = pytest.mark.gpu

FIXTURES = {"g8_rollout_c1": 36, "g8_rollout_small_all_at_dest": 40, "g9_c1_waiting_policy": 8, "g7_n1_exiting_only": 4,
            "g7_n5_odd": None, "g4_c5_all_at_dest_greedy_32_32": None}      # records the issue counted (None: not stated)
CONFIG_OF_N = {3: "g7_n3_small", 1: "g7_n1_exiting_only", 50: "g4_c5_all_at_dest_greedy_25_25"}
# K: one step, the accumulate kernel's 16-step chunk - 1 / exact / + 1, the count kernel's 32-step chunk likewise, many chunks
SYNTHETIC_K = (1, 15, 16, 17, 31, 32, 33, 130)


@pytest.fixture(scope="module")
def ccx():
    import torch

    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    from collectivecrossing_amd.batched import BatchedCollectiveCrossing

    return BatchedCollectiveCrossing


@pytest.fixture(scope="module")
def goldens():
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = Golden(name)
        return cache[name]

    return get


@pytest.fixture(scope="module")
def batches(ccx, goldens):
    """One batch per (config fixture, E), shared by the tests of this module (tracking is re-enabled per test)."""
    cache = {}

    def get(name, E):
        if (name, E) not in cache:
            cache[name, E] = ccx(goldens(name).config, E)
        return cache[name, E]

    yield get
    for b in cache.values():
        b.close()


def _dev(*arrays):
    import torch

    return [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in arrays]


def _feed(batch, spec, r, af, ef, cuts=None):
    """The same steps into the device and the spec, as one update or cut at `cuts`."""
    K = ef.shape[0]
    edges = [0, K] if cuts is None else [0, *cuts, K]
    tr, taf, tef = _dev(r, af, ef)
    for a, b in zip(edges[:-1], edges[1:]):
        batch.update_episode_stats(tr[a:b], taf[a:b], tef[a:b])
        spec.update(r[a:b], af[a:b], ef[a:b])
    batch.synchronize()          # (the device tensors stay alive until the updates have run)


def _accumulators(batch) -> dict:
    batch.synchronize()
    st = batch.episode_stats()
    return {k: getattr(st, k).cpu().numpy() for k in ACC_KEYS}


def _log(batch) -> tuple[dict, int]:
    rec = batch.finished_episodes(clear=False)
    return {k: getattr(rec, k) for k in LOG_KEYS}, rec.dropped


def _assert_accumulators(batch, spec, tag=""):
    got = _accumulators(batch)
    for k, want in spec.accumulators().items():
        np.testing.assert_array_equal(bits(got[k]), bits(want), err_msg=f"{k} {tag}")


def _assert_log(batch, spec, tag="", sort=False):
    got, dropped = _log(batch)
    want = spec.log()
    if sort:
        got, want = sort_log(got), sort_log(want)
    for k in LOG_KEYS:
        np.testing.assert_array_equal(bits(got[k]), bits(want[k]), err_msg=f"log {k} {tag}")
    assert dropped == spec.dropped, tag


# ------------------------------------------------------------------------------------------------- 1. fixture replay
@pytest.mark.parametrize("name", sorted(FIXTURES))
def test_fixture_replay(batches, goldens, name):
    g = goldens(name)
    batch = batches(name, g.E)
    for capacity in (1024, 0):
        batch.track_episodes(capacity)
        spec = StatsSpec(g.E, g.N, capacity)
        _feed(batch, spec, g["reward"], g["agent_flags"], g["env_flags"])
        _assert_accumulators(batch, spec, f"{name} capacity {capacity}")
        if capacity:
            _assert_log(batch, spec, name)                        # the exact, env-major log order
            assert len(spec.records) == spec.emitted > 0
            if FIXTURES[name] is not None:
                assert spec.emitted == FIXTURES[name]
    batch.track_episodes(False)


# ------------------------------------------------------------------------------------------------- 2. cut invariance
def test_cut_invariance(batches, goldens):
    g = goldens("g8_rollout_c1")
    assert g.K == 90
    batch = batches("g8_rollout_c1", g.E)
    results = []
    for cuts in (None, [1], list(range(16, 90, 16)), list(range(1, 90))):
        batch.track_episodes(1024)
        spec = StatsSpec(g.E, g.N, 1024)
        _feed(batch, spec, g["reward"], g["agent_flags"], g["env_flags"], cuts)
        _assert_accumulators(batch, spec, f"cuts {cuts}")
        _assert_log(batch, spec, f"cuts {cuts}")                  # (each cut's own order, update after update)
        log, dropped = _log(batch)
        results.append((_accumulators(batch), sort_log(log)))
        assert dropped == 0 and len(log["env"]) == 36
    acc0, log0 = results[0]
    for acc, log in results[1:]:
        for k in ACC_KEYS:
            np.testing.assert_array_equal(bits(acc[k]), bits(acc0[k]), err_msg=k)
        for k in LOG_KEYS:
            np.testing.assert_array_equal(bits(log[k]), bits(log0[k]), err_msg=k)
    batch.track_episodes(False)


# ------------------------------------------------------------------------------------------------- 3. synthetic
@pytest.fixture(scope="module")
def synthetic():
    """(reward, agent_flags, env_flags) of the spec's generator, made once per (K, N)."""
    cache = {}

    def get(K, N, seed):
        if (K, N, seed) not in cache:
            cache[K, N, seed] = make_trajectory(K, 67, N, seed=seed)
        return cache[K, N, seed]

    return get


@pytest.mark.parametrize("K", SYNTHETIC_K)
@pytest.mark.parametrize("N", sorted(CONFIG_OF_N))
def test_synthetic_trajectories(batches, synthetic, N, K):
    E = 67
    batch = batches(CONFIG_OF_N[N], E)
    assert batch.num_agents == N
    first, second = synthetic(K, N, 11), synthetic(K, N, 12)
    assert np.isnan(first[0]).any() and (first[2][0] & 3).any() and (first[2][K - 1] & 3).any()     # finishes on step 0 and K - 1
    try:
        for mode in ("log", "no log", "one load per step"):
            batch.set_tunable("stats_naive", int(mode == "one load per step"))
            capacity = 0 if mode == "no log" else 100_000
            batch.track_episodes(capacity)
            spec = StatsSpec(E, N, capacity)
            _feed(batch, spec, *first)
            _feed(batch, spec, *second)                           # carried accumulators, latches and the log's fill level
            _assert_accumulators(batch, spec, f"N {N} K {K} {mode}")
            assert not np.isnan(spec.ret).any() and spec.emitted >= 2 * (E // 7) * min(K, 2)
            if capacity:
                _assert_log(batch, spec, f"N {N} K {K} {mode}")
    finally:
        batch.set_tunable("stats_naive", 0)
        batch.track_episodes(False)


def test_one_load_per_step_without_a_log(batches):
    """The accumulate kernel's fourth instantiation (no log, one dependent load per step), which the three modes above do not
    launch: 13 envs x 5 agents (65 slots), two updates of 17 steps (one 16-step chunk and a tail), carried accumulators.
    (The two load schedules are defined to give the same bytes, so only the log flag can show in the results: with the log
    on by mistake the kernel would write records where none are kept.)"""
    E, N, K = 13, 5, 17
    batch = batches("g7_n5_odd", E)
    assert batch.num_agents == N
    first, second = make_trajectory(K, E, N, seed=21), make_trajectory(K, E, N, seed=22)
    assert (first[2] & 3).any() and (second[2] & 3).any()         # episodes finish inside both updates
    try:
        batch.set_tunable("stats_naive", 1)
        batch.track_episodes(0)
        spec = StatsSpec(E, N, 0)
        _feed(batch, spec, *first)
        _feed(batch, spec, *second)
        _assert_accumulators(batch, spec, "one load per step, no log")
        assert spec.emitted > 0 and not np.isnan(spec.ret).any()
    finally:
        batch.set_tunable("stats_naive", 0)
        batch.track_episodes(False)


# (grids larger than the device holds at once, with agent counts that do not divide a wavefront: the blocks of a later
# round start after earlier ones have stored their results, so an env whose lanes were spread over two workgroups -- or any
# other read of a value the same launch writes -- would show here, and only here)
@pytest.fixture(scope="module")
def large():
    cache = {}

    def get(K, E, N, seed):
        if (K, E, N, seed) not in cache:
            cache[K, E, N, seed] = make_trajectory(K, E, N, seed=seed)
        return cache[K, E, N, seed]

    return get


@pytest.mark.parametrize("K", (1, 17))
@pytest.mark.parametrize("E,N", ((4096, 50), (60_000, 3)))
def test_grids_beyond_residency(batches, large, E, N, K):
    batch = batches(CONFIG_OF_N[N], E)
    first, second = large(K, E, N, 21), large(K, E, N, 22)
    try:
        for capacity in (400_000, 0):
            batch.track_episodes(capacity)
            spec = StatsSpec(E, N, capacity)
            _feed(batch, spec, *first)
            _feed(batch, spec, *second)
            _assert_accumulators(batch, spec, f"E {E} N {N} K {K} capacity {capacity}")
            assert spec.emitted > E // 7
            if capacity:
                assert spec.dropped == 0
                _assert_log(batch, spec, f"E {E} N {N} K {K}")
    finally:
        batch.track_episodes(False)


# ------------------------------------------------------------------------------------------------- 4. log overflow
def test_log_overflow_and_clear(batches, synthetic):
    E, N, K, C = 67, 3, 17, 50
    batch = batches(CONFIG_OF_N[N], E)
    r, af, ef = synthetic(K, N, 11)
    full = StatsSpec(E, N, 100_000)
    full.update(r, af, ef)
    total = full.emitted
    assert total > 2 * C
    batch.track_episodes(C)
    spec = StatsSpec(E, N, C)
    _feed(batch, spec, r, af, ef)
    log, dropped = _log(batch)
    assert len(log["env"]) == C and dropped == total - C == spec.dropped
    want = full.log()
    for k in LOG_KEYS:                                            # the first C records of the env-major order
        np.testing.assert_array_equal(bits(log[k]), bits(want[k][:C]), err_msg=k)
    _feed(batch, spec, r, af, ef)                                 # full: everything is dropped, and counted
    log, dropped = _log(batch)
    assert len(log["env"]) == C and dropped == spec.dropped > total - C
    _assert_accumulators(batch, spec, "full log")
    batch.clear_episode_log()                                     # ccx_episode_log_clear
    spec.clear_log()
    rec = batch.finished_episodes(clear=True)
    assert len(rec) == 0 and rec.dropped == 0
    _feed(batch, spec, r, af, ef)                                 # later records get in again
    _assert_log(batch, spec, "after clear")
    assert len(spec.records) == C
    batch.track_episodes(False)


# ------------------------------------------------------------------------------------------------- 5. public API
def _twins(ccx, g, E):
    A, B = ccx(g.config, E), ccx(g.config, E)
    for b in (A, B):
        b.make_reset_pool(seed0=5, size=64)
        b.reset_from_pool()
    return A, B


def test_rollout_and_single_steps_leave_the_same_stats(ccx, goldens):
    import torch

    g = goldens("g8_rollout_c1")
    E, N, K = g.E, g.N, 90
    A, B = _twins(ccx, g, E)
    A.track_episodes(256)
    B.track_episodes(256)
    assert A.episode_stats_launches() == 3
    acts = torch.from_numpy(g["actions"][:K]).cuda()
    traj = A.rollout(acts, auto_reset=True, want_obs=False)
    for s in range(K):
        B.step_begin(acts[s])
        B.step_finish(auto_reset=True, want_obs=False)
    a, b = _accumulators(A), _accumulators(B)
    for k in ACC_KEYS:
        np.testing.assert_array_equal(bits(a[k]), bits(b[k]), err_msg=k)
    la, lb = sort_log(_log(A)[0]), sort_log(_log(B)[0])
    for k in LOG_KEYS:
        np.testing.assert_array_equal(bits(la[k]), bits(lb[k]), err_msg=k)
    assert len(la["env"]) == int(a["finished"].sum()) >= E           # every env finished at least one episode in 90 steps
    # the stats are those of the spec on the very trajectory the rollout wrote
    spec = StatsSpec(E, N, 256)
    spec.update(traj.reward.cpu().numpy(), traj.agent_flags.cpu().numpy(), traj.env_flags.cpu().numpy())
    _assert_accumulators(A, spec, "rollout")
    _assert_log(A, spec, "rollout")
    # tracking covered the whole run from a fresh reset: the episode length in progress is the env's own step counter
    open_ = a["closed"] == 0
    assert open_.any()
    np.testing.assert_array_equal(a["steps"][open_], A.get_state()["step_count"][open_])
    # a rollout that writes no trajectory cannot be tracked, and says so before it steps
    before = A.get_state()["step_count"].copy()
    with pytest.raises(ValueError):
        A.rollout(acts[:4], auto_reset=True, want_traj=False)
    np.testing.assert_array_equal(A.get_state()["step_count"], before)
    # reset_from_pool(mask) clears exactly the masked envs, writes no record
    mask = (np.arange(E) % 3 == 0).astype(np.uint8)
    A.reset_from_pool(mask)
    c = _accumulators(A)
    m = mask != 0
    assert (a["steps"][~m] > 0).any() and (a["steps"][m] > 0).any()
    for k in ("ret", "live_steps", "steps", "closed"):
        assert not c[k][m].any(), k
        np.testing.assert_array_equal(bits(c[k][~m]), bits(a[k][~m]), err_msg=k)
    for k in ("finished", "last_ret", "last_live_steps", "last_steps", "last_end"):
        np.testing.assert_array_equal(bits(c[k]), bits(a[k]), err_msg=k)
    assert len(_log(A)[0]["env"]) == len(la["env"])
    A.close()
    B.close()


def test_without_a_log_an_update_is_one_launch(ccx, goldens):
    import torch

    g = goldens("g8_rollout_c1")
    A, B = _twins(ccx, g, g.E)
    with pytest.raises(RuntimeError):
        A.episode_stats()
    A.track_episodes()                                               # log_capacity = 0
    B.track_episodes(64)
    assert A.episode_stats_launches() == 1 and B.episode_stats_launches() == 3
    acts = torch.from_numpy(g["actions"][:40]).cuda()
    A.rollout_greedy(40, auto_reset=True, want_obs=False)
    B.rollout_greedy(40, auto_reset=True, want_obs=False)
    a, b = _accumulators(A), _accumulators(B)
    for k in ACC_KEYS:
        np.testing.assert_array_equal(bits(a[k]), bits(b[k]), err_msg=k)
    assert a["finished"].sum() > 0 and int(A.episode_stats().log_count.sum()) == 0
    with pytest.raises(RuntimeError):
        A.finished_episodes()
    # step / step_mixed / rollout_mixed are tracked too: 3 + 1 + 2 more steps on both twins, by different calls
    for s in range(3):
        A.step(acts[s], want_obs=False)
    A.step_mixed(acts[3], "exiting", want_obs=False)
    A.rollout_mixed(acts[4:6], "exiting", want_obs=False)
    for s in range(3):
        B.rollout(acts[s:s + 1], want_obs=False)
    B.step_mixed(acts[3], "exiting", want_obs=False)
    B.step_mixed(acts[4], "exiting", want_obs=False)
    B.step_mixed(acts[5], "exiting", want_obs=False)
    a, b = _accumulators(A), _accumulators(B)
    for k in ACC_KEYS:
        np.testing.assert_array_equal(bits(a[k]), bits(b[k]), err_msg=k)
    open_ = a["closed"] == 0
    np.testing.assert_array_equal(a["steps"][open_], A.get_state()["step_count"][open_])
    A.track_episodes(False)
    A.rollout(acts[:2], want_traj=False)                             # not tracked any more: allowed again
    with pytest.raises(RuntimeError):
        A.episode_stats()
    A.close()
    B.close()


# ------------------------------------------------------------------------------------------------- 6. graph
def test_captured_step_and_update(ccx, goldens):
    import torch

    g = goldens("g8_rollout_c1")
    E, N, n = g.E, g.N, 45
    A, B = _twins(ccx, g, E)
    acts = torch.empty((E, N), dtype=torch.uint8, device="cuda")
    side = torch.cuda.Stream()
    B.use_stream(side)
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        B.greedy_actions(out=acts)
        B.step(acts, want_obs=False)                      # first call: the output buffers
        side.synchronize()
        B.reset_from_pool()
        B.track_episodes(128)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            B.greedy_actions(out=acts)
            B.step(acts, want_obs=False)                  # tracked: the update's three kernels are captured behind the step
        B.reset_from_pool()                               # (the capture ran nothing)
        side.synchronize()
        for _ in range(n):
            graph.replay()
        side.synchronize()
    A.track_episodes(128)
    mine = torch.empty((E, N), dtype=torch.uint8, device="cuda")
    for _ in range(n):
        A.greedy_actions(out=mine)
        A.step(mine, want_obs=False)
    a, b = _accumulators(A), _accumulators(B)
    for k in ACC_KEYS:
        np.testing.assert_array_equal(bits(a[k]), bits(b[k]), err_msg=k)
    assert a["finished"].sum() > 0 and a["closed"].any()             # no auto-reset: finished envs stay latched
    assert (a["finished"] <= 1).all()
    la, lb = _log(A)[0], _log(B)[0]
    for k in LOG_KEYS:
        np.testing.assert_array_equal(bits(la[k]), bits(lb[k]), err_msg=k)
    A.close()
    B.use_stream(None)
    B.close()
