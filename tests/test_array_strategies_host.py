"""Array-form user strategies on the CPU: the batched methods of tests/golden/array_strategies.py, called on a
``StrategyView`` of CPU tensors rebuilt from reference recordings, give what the reference's per-agent calls gave --
values, entries and absences.  No GPU, no libccx."""

import gzip
import json
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

GOLDEN = Path(__file__).resolve().parent / "golden"
sys.path.insert(0, str(GOLDEN))

from collectivecrossing_amd import configs as C  # noqa: E402
from collectivecrossing_amd import strategies as S  # noqa: E402
from collectivecrossing_amd.params import agent_ids, array_form_strategies, lower_config  # noqa: E402


def _load(name):
    with gzip.open(GOLDEN / name) as z:
        return json.loads(z.read())


def _view(config, pos, active, term, trunc, step_count):
    t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(np.asarray(a)[None], dt))  # noqa: E731
    pos = np.asarray(pos, np.int32)
    return S.StrategyView(config, t(pos[:, 0], np.int32), t(pos[:, 1], np.int32), t(active, np.bool_), t(term, np.bool_),
                          t(trunc, np.bool_), torch.tensor([step_count], dtype=torch.int32))


def _compare(tag, ids, view, fns, st, live):
    """The batched methods against one recorded step: rewards / truncations exist exactly for live agents, termination
    entries where the value is not -1."""
    if "reward" in fns:
        r = S.check_batch_result("reward", fns["reward"], fns["reward"].calculate_rewards_batch(view), view)[0]
        assert sorted(st["rewards"]) == sorted(a for a, l in zip(ids, live) if l), tag
        for i, a in enumerate(ids):
            if live[i]:
                assert np.float64(r[i].item()).view(np.uint64) == np.float64(st["rewards"][a]).view(np.uint64), (tag, a)
    if "termination" in fns:
        t = S.check_batch_result("termination", fns["termination"], fns["termination"].calculate_terminateds_batch(view), view)[0]
        assert t.dtype is torch.int8
        got = {a: bool(t[i].item()) for i, a in enumerate(ids) if t[i].item() != -1}
        want = {a: v for a, v in st["terminateds"].items() if a != "__all__"}
        assert got == want, tag
        assert st["terminateds"]["__all__"] == (bool(got) and all(got.values())), tag
    if "truncation" in fns:
        u = S.check_batch_result("truncation", fns["truncation"], fns["truncation"].calculate_truncateds_batch(view), view)[0]
        assert u.dtype is torch.uint8
        got = {a: bool(u[i].item()) for i, a in enumerate(ids) if live[i]}
        want = {a: v for a, v in st["truncateds"].items() if a != "__all__"}
        assert got == want, tag
        assert st["truncateds"]["__all__"] == (bool(got) and all(got.values())), tag


@pytest.fixture()
def g12_twins():
    import array_strategies as ast
    import custom_strategies as cs
    undo = ast.register(S, ast.make_g12_twins(S.RewardFunction, S.TerminatedFunction, S.TruncatedFunction), cs.NAMES)
    yield cs
    undo()


@pytest.fixture()
def g15_plugins():
    import array_strategies as ast
    undo = ast.register(S, ast.make_g15(S.RewardFunction, S.TerminatedFunction, S.TruncatedFunction), ast.G15_NAMES)
    yield ast
    undo()


@pytest.mark.parametrize("mix", ["all", "reward", "terminated", "truncated"])
def test_g12_twins_reproduce_every_recorded_step(g12_twins, mix):
    cs = g12_twins
    recorded = _load("g12_custom_strategies.json.gz")[mix]
    config = cs.build_config(C, C, C, C, cs.MIXES[mix])
    ids = agent_ids(config)
    fns = array_form_strategies(config)
    assert sorted(fns) == sorted({"reward": "reward", "terminated": "termination", "truncated": "truncation"}[k] for k in cs.MIXES[mix])
    compared = 0
    for ep in recorded:
        pos = {a: [int(v) for v in ep["initial"][a][:2]] for a in ids}
        pos.update({a: list(p) for a, p in ep["forced"].items()})
        term, trunc = [False] * len(ids), [False] * len(ids)
        for s, st in enumerate(ep["steps"]):
            # the post-move state: positions from the recorded observation rows (every row holds all agents), active
            # from this step's flags, the PRE-step terminated / truncated flags from the previous step's
            rows = st["observations"]
            if rows:
                k, row = next(iter(rows.items()))
                for j, a in enumerate(ids):
                    pos[a] = [int(row[0]), int(row[1])] if a == k else [int(row[6 + 4 * j]), int(row[7 + 4 * j])]
            live = [not (t or u) for t, u in zip(term, trunc)]
            # (a step in which nobody is observed cannot be rebuilt from the recording; then nobody is live either and no
            #  agent can still be terminated by a move only if all are terminated already: require that)
            if rows or all(term):
                view = _view(config, [pos[a] for a in ids], [st["flags"][a][0] for a in ids], term, trunc, st["step_count"])
                _compare(f"{mix} seed {ep['seed']} step {s}", ids, view, fns, st, live)
                compared += 1
            term = [st["flags"][a][1] for a in ids]
            trunc = [st["flags"][a][2] for a in ids]
    assert compared >= 30


def test_g15_plugins_reproduce_every_recorded_step(g15_plugins):
    ast = g15_plugins
    for ep in _load("g15_array_strategies.json.gz")["episodes"]:
        config = ast.g15_config(C, C, C, C, getattr(ast, ep["geometry"]), ep["max_steps"])
        ids = agent_ids(config)
        assert ids == ep["ids"]
        fns = array_form_strategies(config)
        assert sorted(fns) == ["reward", "termination", "truncation"]
        term, trunc = [False] * len(ids), [False] * len(ids)
        for s, st in enumerate(ep["steps"]):
            live = [not (t or u) for t, u in zip(term, trunc)]
            view = _view(config, st["positions"], [f[0] for f in st["flags"]], term, trunc, st["step_count"])
            _compare(f"g15 seed {ep['seed']} step {s}", ids, view, fns, st, live)
            term, trunc = [f[1] for f in st["flags"]], [f[2] for f in st["flags"]]


def test_view_predicates_match_the_flag_bit_definitions():
    import array_strategies as ast
    config = C.CollectiveCrossingConfig(**ast.C1)
    W, H = config.width, config.height
    ys, xs = np.mgrid[0:H + 1, 0:W + 1]
    n = config.num_boarding_agents + config.num_exiting_agents
    E = xs.size
    x = np.repeat(xs.reshape(-1, 1), n, 1)
    y = np.repeat(ys.reshape(-1, 1), n, 1)
    z = torch.zeros((E, n), dtype=torch.bool)
    v = S.StrategyView(config, torch.from_numpy(x.astype(np.int32)), torch.from_numpy(y.astype(np.int32)), ~z, z, z,
                       torch.zeros(E, dtype=torch.int32))
    from collectivecrossing_amd.env import CollectiveCrossingEnv
    env = CollectiveCrossingEnv.host_view(config)
    ids = list(env._agents)
    for e in range(E):
        for i, a in enumerate(ids):
            env._agents[a].position = np.array([x[e, i], y[e, i]])
        for i, a in enumerate(ids):
            assert bool(v.in_tram_area()[e, i]) == bool(env.is_in_tram_area(a))
            assert bool(v.at_door()[e, i]) == bool(env.is_at_tram_door(a))
            assert bool(v.at_destination()[e, i]) == bool(env.has_agent_reached_destination(a))
            assert bool(v.in_exiting_destination_area()[e, i]) == bool(env.is_in_exiting_destination_area(a))


def test_lower_config_accepts_array_form_classes_only_with_the_keyword(g12_twins):
    cs = g12_twins
    config = cs.build_config(C, C, C, C, cs.MIXES["all"])
    with pytest.raises(ValueError, match="E = 1"):
        lower_config(config)
    with pytest.raises(ValueError, match="E = 1"):
        lower_config(config, allow_position_only=True)
    p = lower_config(config, allow_array_form=True)
    assert (p.reward_mode, p.terminated_mode, p.truncated_mode, p.max_steps) == (3, 0, 0, 9)


def test_an_undeclared_class_still_raises_the_single_env_message():
    import custom_strategies as cs
    made = cs.make(S.RewardFunction, S.TerminatedFunction, S.TruncatedFunction)       # per-agent methods only
    S.REWARD_FUNCTIONS[cs.NAMES["reward"]] = made["reward"]
    S.TRUNCATED_FUNCTIONS[cs.NAMES["truncated"]] = made["truncated"]
    try:
        with pytest.raises(ValueError, match="E = 1"):
            lower_config(cs.build_config(C, C, C, C, cs.MIXES["reward"]), allow_position_only=True, allow_array_form=True)
        with pytest.raises(ValueError, match="Unknown truncation function"):
            lower_config(cs.build_config(C, C, C, C, cs.MIXES["truncated"]), allow_array_form=True)
        assert array_form_strategies(cs.build_config(C, C, C, C, cs.MIXES["reward"])) == {}
    finally:
        S.REWARD_FUNCTIONS.pop(cs.NAMES["reward"], None)
        S.TRUNCATED_FUNCTIONS.pop(cs.NAMES["truncated"], None)


def test_returned_tensors_are_checked(g15_plugins):
    ast = g15_plugins
    config = ast.g15_config(C, C, C, C, ast.C1, 9)
    z = torch.zeros((2, 8), dtype=torch.bool)
    v = S.StrategyView(config, torch.zeros((2, 8), dtype=torch.int32), torch.zeros((2, 8), dtype=torch.int32), ~z, z, z,
                       torch.zeros(2, dtype=torch.int32))
    fn = array_form_strategies(config)["reward"]
    with pytest.raises(TypeError, match="torch.float64"):
        S.check_batch_result("reward", fn, torch.zeros((2, 8), dtype=torch.float32), v)
    with pytest.raises(TypeError, match="shape"):
        S.check_batch_result("reward", fn, torch.zeros((2, 7), dtype=torch.float64), v)
    with pytest.raises(TypeError, match="torch.Tensor"):
        S.check_batch_result("reward", fn, np.zeros((2, 8)), v)
    with pytest.raises(TypeError, match="torch.bool"):
        S.check_batch_result("truncation", fn, torch.zeros((2, 8), dtype=torch.int8), v)
    with pytest.raises(TypeError, match="expected"):
        S.StrategyView(config, torch.zeros((2, 8), dtype=torch.int64), v.y, ~z, z, z, v.step_count)
