"""Array-form user strategies on the GPU batch path: begin -> the classes' batched methods -> finish on the handle's
stream.  Reference recordings (g12 with the array-form twins, g15) replay dict for dict through
``BatchedCollectiveCrossing.step`` and ``VectorCollectiveCrossing.step_dicts``; a 4096-env batch with auto-reset equals
single-env objects running the per-agent form on the host slow path; a graph-captured loop body equals eager steps."""

import gzip
import json
import sys
from pathlib import Path

import numpy as np
import pytest

GOLDEN = Path(__file__).resolve().parent / "golden"
sys.path.insert(0, str(GOLDEN))
import array_strategies as ast  # noqa: E402
import custom_strategies as cs  # noqa: E402

pytestmark = pytest.mark.gpu


def _load(name):
    with gzip.open(GOLDEN / name) as z:
        return json.loads(z.read())


def _np(t):
    return None if t is None else t.cpu().numpy()


@pytest.fixture()
def S():
    import torch

    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    from collectivecrossing_amd import strategies
    undo = [ast.register(strategies, ast.make_g12_twins(strategies.RewardFunction, strategies.TerminatedFunction,
                                                        strategies.TruncatedFunction), cs.NAMES),
            ast.register(strategies, ast.make_g15(strategies.RewardFunction, strategies.TerminatedFunction,
                                                  strategies.TruncatedFunction), ast.G15_NAMES)]
    yield strategies
    for u in undo:
        u()


def _expected_row(i, pos, active, nb, consts):
    """DefaultObservation row of agent slot i (observations.py:43-94) from positions [N][2] and active [N]."""
    n = len(pos)
    row = np.empty(6 + 4 * n, np.float32)
    row[:6] = (pos[i][0], pos[i][1], *consts)
    for j in range(n):
        row[6 + 4 * j:10 + 4 * j] = (-1, -1, -1, -1) if j == i else (pos[j][0], pos[j][1], 0 if j < nb else 1, 1 if active[j] else 0)
    return row


def _assert_env_step(tag, ids, e, out, want, obs_rows=None):
    """One env of a batched step (arrays of `out`: obs, reward, agent_flags, env_flags, term_present as numpy) against the
    reference-shaped dicts `want` = (rewards, terminateds, truncateds, obs keys): values, entries AND absences."""
    obs, rew, af, ef, tp = out
    rewards, terminateds, truncateds, obs_keys = want
    live = [(int(af[e, i]) & 4) != 0 for i in range(len(ids))]
    assert sorted(rewards) == sorted(a for a, l in zip(ids, live) if l), (tag, "reward entries")
    for i, a in enumerate(ids):
        if live[i]:
            assert np.float64(rew[e, i]).view(np.uint64) == np.float64(rewards[a]).view(np.uint64), (tag, a, rew[e, i], rewards[a])
        else:
            assert np.float64(rew[e, i]).view(np.uint64) == 0, (tag, a, "+0.0 where not live")
    got_t = {a: (int(af[e, i]) & 1) != 0 for i, a in enumerate(ids) if tp[e, i]}
    got_t["__all__"] = (int(ef[e]) & 1) != 0
    assert got_t == {k: bool(v) for k, v in terminateds.items()}, (tag, "terminateds")
    got_u = {a: (int(af[e, i]) & 2) != 0 for i, a in enumerate(ids) if live[i]}
    got_u["__all__"] = (int(ef[e]) & 2) != 0
    assert got_u == {k: bool(v) for k, v in truncateds.items()}, (tag, "truncateds")
    assert sorted(a for i, a in enumerate(ids) if int(af[e, i]) & 8) == sorted(obs_keys), (tag, "observation keys")
    if obs_rows is not None:
        for i, a in enumerate(ids):
            if a in obs_rows:
                np.testing.assert_array_equal(obs[e, i].view(np.uint32), np.asarray(obs_rows[a], np.float32).view(np.uint32), err_msg=f"{tag} {a}")


def _g12_batch(mix, recorded):
    from collectivecrossing_amd import configs as C
    from collectivecrossing_amd.params import agent_ids
    config = cs.build_config(C, C, C, C, cs.MIXES[mix])
    ids = agent_ids(config)
    eps = recorded[mix]
    pos = np.zeros((len(eps), len(ids), 2), np.int32)
    for e, ep in enumerate(eps):
        for i, a in enumerate(ids):
            pos[e, i] = ep["forced"].get(a, ep["initial"][a][:2])
    return config, ids, eps, pos


def _set_positions(batch, pos):
    E, N = pos.shape[:2]
    batch.set_state(x=pos[..., 0], y=pos[..., 1], active=np.ones((E, N), np.uint8), terminated=np.zeros((E, N), np.uint8),
                    truncated=np.zeros((E, N), np.uint8), step_count=np.zeros(E, np.int32), episode=np.zeros(E, np.int32))


@pytest.mark.parametrize("mix", ["all", "reward", "terminated", "truncated"])
def test_g12_episodes_replay_on_one_batch_through_step(S, mix):
    from collectivecrossing_amd.batched import BatchedCollectiveCrossing
    from collectivecrossing_amd.env import encode_actions
    config, ids, eps, pos = _g12_batch(mix, _load("g12_custom_strategies.json.gz"))
    batch = BatchedCollectiveCrossing(config, len(eps))
    assert batch.has_array_strategies and batch.num_envs == 3
    _set_positions(batch, pos)
    for s in range(len(eps[0]["steps"])):
        enc = [encode_actions(ids, ep["steps"][s]["actions"]) for ep in eps]
        r = batch.step(np.stack([a for a, _ in enc]), np.stack([o for _, o in enc]))
        out = [_np(v) for v in (r.obs, r.reward, r.agent_flags, r.env_flags, r.term_present)]
        state = batch.get_state()
        for e, ep in enumerate(eps):
            st = ep["steps"][s]
            _assert_env_step(f"{mix} seed {ep['seed']} step {s}", ids, e, out,
                             (st["rewards"], st["terminateds"], st["truncateds"], list(st["observations"])), st["observations"])
            for i, a in enumerate(ids):
                assert [bool(state[k][e, i]) for k in ("active", "terminated", "truncated")] == st["flags"][a], (mix, e, s, a)
                info = st["infos"].get(a)
                if info is not None:
                    f = int(out[2][e, i])
                    assert ((f & 0x10) != 0, (f & 0x20) != 0, (f & 0x40) != 0, (f & 0x80) != 0) == (
                        info["in_tram_area"], info["at_door"], info["active"], info["at_destination"]), (mix, e, s, a)
            assert int(state["step_count"][e]) == st["step_count"]
    batch.close()


@pytest.mark.parametrize("mix", ["all", "reward", "terminated", "truncated"])
def test_g12_episodes_replay_through_vector_step_dicts(S, mix):
    from collectivecrossing_amd.vector import VectorCollectiveCrossing
    config, ids, eps, pos = _g12_batch(mix, _load("g12_custom_strategies.json.gz"))
    vec = VectorCollectiveCrossing(config, len(eps))
    _set_positions(vec.batch, pos)
    absent = 0
    for s in range(len(eps[0]["steps"])):
        vec.step_dicts([dict(ep["steps"][s]["actions"]) for ep in eps])
        for e, ep in enumerate(eps):
            st = ep["steps"][s]
            o, r, te, tr, inf = vec.view(e)
            tag = f"{mix} seed {ep['seed']} step {s}"
            assert {k: v.tolist() for k, v in o.items()} == st["observations"], tag
            assert {k: float(v) for k, v in r.items()} == st["rewards"], tag
            assert {k: bool(v) for k, v in te.items()} == st["terminateds"], tag
            assert {k: bool(v) for k, v in tr.items()} == st["truncateds"], tag
            assert inf == st["infos"], tag
            absent += len(ids) + 1 - len(te)
    if "terminated" in cs.MIXES[mix]:
        assert absent > 0, "the recording holds termination entries that are absent (None)"
    else:
        assert absent == 0, "a built-in termination rule has an entry for every agent"
    vec.close()


def test_g15_recording_replays_exactly_small_and_large_grid(S):
    from collectivecrossing_amd import configs as C
    from collectivecrossing_amd.batched import BatchedCollectiveCrossing
    from collectivecrossing_amd.env import encode_actions
    from collectivecrossing_amd.params import agent_ids, calculate_tram_boundaries
    episodes = _load("g15_array_strategies.json.gz")["episodes"]
    groups = {}
    for ep in episodes:
        groups.setdefault((ep["geometry"], ep["max_steps"], len(ep["steps"])), []).append(ep)
    assert sorted(k[0] for k in groups) == ["BIG", "C1"] and len(groups[("C1", 14, 24)]) >= 3
    for (geometry, max_steps, K), eps in groups.items():
        config = ast.g15_config(C, C, C, C, getattr(ast, geometry), max_steps)
        ids = agent_ids(config)
        nb = config.num_boarding_agents
        tb = calculate_tram_boundaries(config)
        consts = ((tb.tram_door_left + tb.tram_door_right) // 2, config.division_y, tb.tram_door_left, tb.tram_door_right)
        batch = BatchedCollectiveCrossing(config, len(eps))
        assert batch.has_array_strategies
        if geometry == "BIG":
            assert batch.step_shape()["ok"] == 0, "a grid too large for the LDS occupancy tables"
        _set_positions(batch, np.asarray([ep["initial"] for ep in eps], np.int32))
        for s in range(K):
            enc = [encode_actions(ids, ep["steps"][s]["actions"]) for ep in eps]
            r = batch.step(np.stack([a for a, _ in enc]), np.stack([o for _, o in enc]))
            out = [_np(v) for v in (r.obs, r.reward, r.agent_flags, r.env_flags, r.term_present)]
            state = batch.get_state()
            for e, ep in enumerate(eps):
                st = ep["steps"][s]
                tag = f"g15 {geometry} seed {ep['seed']} step {s}"
                active = [f[0] for f in st["flags"]]
                rows = {a: _expected_row(ids.index(a), st["positions"], active, nb, consts) for a in st["obs_keys"]}
                _assert_env_step(tag, ids, e, out, (st["rewards"], st["terminateds"], st["truncateds"], st["obs_keys"]), rows)
                np.testing.assert_array_equal(np.stack([state["x"][e], state["y"][e]], 1), np.asarray(st["positions"]), err_msg=tag)
                got = [[bool(state[k][e, i]) for k in ("active", "terminated", "truncated")] for i in range(len(ids))]
                assert got == st["flags"], tag
                assert int(state["step_count"][e]) == st["step_count"], tag
        batch.close()


SAMPLE = [0, 1, 2, 3, 63, 64, 127, 255, 256, 511, 777, 1000, 1023, 1024, 1500, 1999, 2047, 2048, 2500, 2999, 3000, 3071, 3072,
          3333, 3500, 3777, 3900, 4000, 4050, 4093, 4094, 4095]


def test_4096_envs_with_auto_reset_equal_single_envs_on_the_host_slow_path(S):
    """C2 geometry, g15 plugins, 40 steps with auto_reset.  Actions: the on-device greedy policy's choice with one action in
    five replaced by a uniform draw (agents then really arrive, so termination entries go absent and episodes end within
    the crowd budget of max_steps = 12 at the latest: both are asserted below)."""
    import torch

    from collectivecrossing_amd import CollectiveCrossingEnv
    from collectivecrossing_amd import configs as C
    from collectivecrossing_amd.batched import BatchedCollectiveCrossing
    from collectivecrossing_amd.params import agent_ids
    E, K, P, seed0, max_steps = 4096, 40, 1000, 500, 12
    assert len(SAMPLE) == 32 and SAMPLE[0] == 0 and SAMPLE[-1] == E - 1
    config = ast.g15_config(C, C, C, C, ast.C2, max_steps)
    ids = agent_ids(config)
    N = len(ids)
    batch = BatchedCollectiveCrossing(config, E)
    batch.make_reset_pool(seed0, P, on_device=False)
    batch.reset_from_pool()
    stride = E % P or 1                                    # include/ccx.h: the cursor of ccx_set_reset_pool
    seed_of = lambda g, j: seed0 + (g + j * stride) % P     # noqa: E731  (reset.py: pool entry p = reset(seed = seed0 + p))
    singles = {}
    for g in SAMPLE:
        env = CollectiveCrossingEnv(config=config)
        assert env._host_strategies
        env.reset(seed=seed_of(g, 0))
        singles[g] = env
    episode = {g: 0 for g in SAMPLE}
    rng = np.random.default_rng(11)
    resets = absent = 0
    for s in range(K):
        a = batch.policy_actions("greedy").cpu().numpy()
        noise = rng.integers(0, 5, size=a.shape, dtype=np.uint8)
        a = np.where((rng.random(a.shape) < 0.2) & (a != 255), noise, a).astype(np.uint8)
        batch.step_begin(a)
        r = batch.step_finish(*batch.run_array_strategies(), auto_reset=True)
        out = [_np(v) for v in (r.obs, r.reward, r.agent_flags, r.env_flags, r.term_present)]
        for g in SAMPLE:
            env = singles[g]
            o, rew, te, tr, _ = env.step({aid: int(a[g, i]) for i, aid in enumerate(ids) if a[g, i] != 255})
            _assert_env_step(f"env {g} step {s}", ids, g, out, (rew, te, tr, list(o)), o)
            absent += N + 1 - len(te)
            assert ((int(out[3][g]) & 4) != 0) == bool(te["__all__"] or tr["__all__"]), (g, s)
            if int(out[3][g]) & 4:
                resets += 1
                episode[g] += 1
                env.reset(seed=seed_of(g, episode[g]))
    state = batch.get_state()
    for g in SAMPLE:
        assert int(state["episode"][g]) == episode[g]
        singles[g].close()
    assert resets >= 1, "the sample must contain an auto-reset"
    assert absent >= 1, "the sample must contain a termination entry of -1 (None)"
    torch.cuda.synchronize()
    batch.close()


def test_graph_captured_loop_body_equals_eager_steps(S):
    import torch

    from collectivecrossing_amd import configs as C
    from collectivecrossing_amd.batched import BatchedCollectiveCrossing
    from collectivecrossing_amd.reset import build_reset_pool
    E, steps = 256, 20
    config = ast.g15_config(C, C, C, C, ast.C2, 9)
    pool = build_reset_pool(config, 40, 97)
    actions = torch.from_numpy(np.random.default_rng(5).integers(0, 5, size=(steps + 3, E, 8), dtype=np.uint8)).cuda()
    eager, graphed = BatchedCollectiveCrossing(config, E), BatchedCollectiveCrossing(config, E)
    for b in (eager, graphed):
        b.set_reset_pool(pool)
        b.reset_from_pool()

    def body(b, a):
        b.step_begin(a)
        return b.step_finish(*b.run_array_strategies(), auto_reset=True)

    side = torch.cuda.Stream()
    graphed.use_stream(side)
    static_a = torch.empty((E, 8), dtype=torch.uint8, device="cuda")
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for s in range(3):                                   # warm-up: allocator, lazy initialisation
            static_a.copy_(actions[s])
            body(graphed, static_a)
    side.synchronize()
    for s in range(3):
        body(eager, actions[s])
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        res = body(graphed, static_a)
    # (capture records, it does not run: the state is where the warm-up left it)
    for s in range(3, steps + 3):
        want = body(eager, actions[s])
        want = [_np(v).copy() for v in (want.obs, want.reward, want.agent_flags, want.env_flags, want.term_present)]
        with torch.cuda.stream(side):
            static_a.copy_(actions[s])
            g.replay()
        side.synchronize()
        got = [_np(v) for v in (res.obs, res.reward, res.agent_flags, res.env_flags, res.term_present)]
        for what, x, y in zip(("obs", "reward", "agent_flags", "env_flags", "term_present"), got, want):
            np.testing.assert_array_equal(x.view(np.uint8), y.view(np.uint8), err_msg=f"{what} replay {s - 3}")
    sa, sb = graphed.get_state(), eager.get_state()
    for k in sa:
        np.testing.assert_array_equal(sa[k], sb[k], err_msg=k)
    assert int(sa["episode"].sum()) > 0, "episodes ended and restarted inside the replays"
    eager.close()
    graphed.close()


def test_rollout_and_policy_rollout_of_an_array_batch_equal_the_step_loop(S):
    """``rollout`` / ``rollout_greedy`` of a batch with array-form strategies loop the split step into the usual result."""
    from collectivecrossing_amd import configs as C
    from collectivecrossing_amd.batched import BatchedCollectiveCrossing
    from collectivecrossing_amd.reset import build_reset_pool
    E, K = 130, 30
    config = ast.g15_config(C, C, C, C, ast.C2, 10)
    pool = build_reset_pool(config, 3, 53)
    actions = np.random.default_rng(8).integers(0, 5, size=(K, E, 8), dtype=np.uint8)
    a, b, c, d = (BatchedCollectiveCrossing(config, E) for _ in range(4))
    for env in (a, b, c, d):
        env.set_reset_pool(pool)
        env.reset_from_pool()
    traj = a.rollout(actions, auto_reset=True, want_compact=True)
    ptraj, pacts = c.rollout_greedy(K, auto_reset=True)
    assert (_np(traj.env_flags) & 4).any() and (_np(traj.term_present) == 0).any()
    for s in range(K):
        b.step_begin(actions[s])
        r = b.step_finish(want_compact=True, auto_reset=True)       # arguments left out: the config's own classes
        for what in ("obs", "reward", "agent_flags", "env_flags", "obs_compact", "term_present"):
            np.testing.assert_array_equal(_np(getattr(traj, what))[s].view(np.uint8), _np(getattr(r, what)).view(np.uint8),
                                          err_msg=f"{what} step {s}")
        acts = d.policy_actions("greedy")
        np.testing.assert_array_equal(_np(pacts)[s], _np(acts), err_msg=f"policy actions step {s}")
        d.step_begin(acts)
        r = d.step_finish(*d.run_array_strategies(), auto_reset=True)
        for what in ("obs", "reward", "agent_flags", "env_flags", "term_present"):
            np.testing.assert_array_equal(_np(getattr(ptraj, what))[s].view(np.uint8), _np(getattr(r, what)).view(np.uint8),
                                          err_msg=f"policy {what} step {s}")
    assert a.get_state()["episode"].tolist() == b.get_state()["episode"].tolist()
    assert a.counters() == b.counters() and c.counters() == d.counters()
    for env in (a, b, c, d):
        env.close()


def test_rollout_of_an_odd_slab_without_trajectory_and_into_a_callers_result(S):
    """11 agents x 3 envs: a step's rows are a multiple of 8 bytes only (the 8-byte row units of odd agent counts take
    that); ``want_traj=False`` writes nothing out; a caller's own result object is filled as it is."""
    from collectivecrossing_amd import configs as C
    from collectivecrossing_amd.batched import BatchedCollectiveCrossing
    E, K = 3, 6
    config = ast.g15_config(C, C, C, C, ast.BIG, 4)
    assert (E * 11 * 50 * 4) % 16 == 8
    actions = np.random.default_rng(2).integers(0, 5, size=(K, E, 11), dtype=np.uint8)
    a, b, c = (BatchedCollectiveCrossing(config, E) for _ in range(3))
    for env in (a, b, c):
        env.reset_host([5, 6, 7])
    own = a.alloc_rollout(K)
    assert own.term_present is None
    traj = a.rollout(actions, out=own)
    assert traj is own and own.term_present is None
    assert b.rollout(actions, want_traj=False) is None
    for s in range(K):
        r = c.step(actions[s])
        for what in ("obs", "reward", "agent_flags", "env_flags"):
            np.testing.assert_array_equal(_np(getattr(own, what))[s].view(np.uint8), _np(getattr(r, what)).view(np.uint8),
                                          err_msg=f"{what} step {s}")
    assert (_np(own.agent_flags) & 2).any(), "the crowd budget ran out inside the rollout"
    sa, sb, sc = a.get_state(), b.get_state(), c.get_state()
    for k in sa:
        np.testing.assert_array_equal(sa[k], sc[k], err_msg=k)
        np.testing.assert_array_equal(sb[k], sc[k], err_msg=k)
    for env in (a, b, c):
        env.close()
