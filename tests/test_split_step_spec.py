"""Pins ``tests/_split_step_spec.py`` -- the NumPy statement of ``ccx_step_begin`` / ``ccx_step_finish`` the split-step
kernels are compared with -- against reference recordings, on the CPU, and asserts that the seeded inputs of
``tests/_split_step_cases.py`` reach the edges the GPU matrix relies on.  No GPU, no libccx."""

import gzip
import json
import sys
from pathlib import Path

import _split_step_cases as cases
import _split_step_spec as spec
import numpy as np
import pytest
from _fixtures import ALL_NPZ, PLUGIN_NPZ, ROLLOUT_NPZ, Golden

GOLDEN = Path(__file__).resolve().parent / "golden"
sys.path.insert(0, str(GOLDEN))

from collectivecrossing_amd import configs as C  # noqa: E402
from collectivecrossing_amd import strategies as S  # noqa: E402
from collectivecrossing_amd.params import agent_ids, lower_config  # noqa: E402


def _load(name):
    with gzip.open(GOLDEN / name) as z:
        return json.loads(z.read())


# ---- reference recordings with user strategies: the recorded dicts ARE the caller's arrays ------------------------------
def _encode(ids, action_dict):
    """action dict -> (actions with 255 = absent, move order: the dict's order, then the agents it leaves out)."""
    a = np.full(len(ids), 255, np.uint8)
    order = [ids.index(k) for k in action_dict]
    for k, v in action_dict.items():
        a[ids.index(k)] = v
    return a, np.asarray(order + [i for i in range(len(ids)) if i not in order], np.uint8)


def _replay(tag, oracle, p, ids, initial, steps, obs_rows_key):
    N = len(ids)
    st = spec.make_state(1, N, x=initial[:, 0], y=initial[:, 1])
    absent = nonlive_emitted = 0
    for s, rec in enumerate(steps):
        a, o = _encode(ids, rec["actions"])
        st, _, _ = spec.begin(p, st, a[None], o[None], oracle=oracle)
        assert int(st["step_count"][0]) == rec["step_count"], (tag, s)
        live = (st["terminated"][0] == 0) & (st["truncated"][0] == 0)
        r = np.array([[rec["rewards"].get(k, 123.0) for k in ids]], np.float64)        # (values at non-LIVE agents are ignored)
        t = np.array([[{None: -1, True: 1, False: 0}[rec["terminateds"].get(k)] for k in ids]], np.int8)
        u = np.array([[int(rec["truncateds"].get(k, True)) for k in ids]], np.uint8)
        f = spec.finish(p, st, r, t, u)
        want = f"{tag} step {s}"
        assert sorted(rec["rewards"]) == sorted(k for k, l in zip(ids, live) if l), want
        for i, k in enumerate(ids):
            exp = np.float64(rec["rewards"][k]).view(np.uint64) if live[i] else 0
            assert f.reward_bits[0, i] == exp, (want, k)
        got_t = {k: bool(f.agent_flags[0, i] & 1) for i, k in enumerate(ids) if f.term_present[0, i]}
        got_t["__all__"] = bool(f.env_flags[0] & 1)
        assert got_t == rec["terminateds"], want
        got_u = {k: bool(f.agent_flags[0, i] & 2) for i, k in enumerate(ids) if f.agent_flags[0, i] & 4}
        got_u["__all__"] = bool(f.env_flags[0] & 2)
        assert got_u == rec["truncateds"], want
        keys = rec["observations"] if obs_rows_key == "observations" else rec["obs_keys"]
        assert sorted(k for i, k in enumerate(ids) if f.emitted[0, i]) == sorted(keys), want
        assert (f.emitted[0] == ((f.agent_flags[0] & 8) != 0)).all()
        if obs_rows_key == "observations":
            rows = spec.observe(oracle, p, st)[0]
            for i, k in enumerate(ids):
                if k in rec["observations"]:
                    np.testing.assert_array_equal(rows[i], np.asarray(rec["observations"][k], np.float32), err_msg=want)
                    info = rec["infos"][k]
                    b = int(f.agent_flags[0, i])
                    assert (bool(b & 0x10), bool(b & 0x20), bool(b & 0x40), bool(b & 0x80)) == (
                        info["in_tram_area"], info["at_door"], info["active"], info["at_destination"]), (want, k)
        else:
            np.testing.assert_array_equal(np.stack([st["x"][0], st["y"][0]], 1), np.asarray(rec["positions"]), err_msg=want)
        absent += N - int(f.term_present.sum())
        nonlive_emitted += int((f.emitted[0] & ~live).sum())
        st = f.state
        flags = rec["flags"] if isinstance(rec["flags"], list) else [rec["flags"][k] for k in ids]
        got = [[bool(st[k][0, i]) for k in ("active", "terminated", "truncated")] for i in range(N)]
        assert got == flags, want
    return absent, nonlive_emitted


@pytest.mark.parametrize("mix", ["all", "reward", "terminated", "truncated"])
def test_g12_recordings_every_step(oracle, mix):
    import array_strategies as ast
    import custom_strategies as cs
    undo = ast.register(S, ast.make_g12_twins(S.RewardFunction, S.TerminatedFunction, S.TruncatedFunction), cs.NAMES)
    try:
        config = cs.build_config(C, C, C, C, cs.MIXES[mix])
        p = lower_config(config, allow_position_only=True, allow_array_form=True)
    finally:
        undo()
    ids = agent_ids(config)
    absent = 0
    for ep in _load("g12_custom_strategies.json.gz")[mix]:
        init = np.asarray([ep["forced"].get(k, ep["initial"][k][:2]) for k in ids], np.int32)
        absent += _replay(f"g12 {mix} seed {ep['seed']}", oracle, p, ids, init, ep["steps"], "observations")[0]
    assert (absent > 0) == ("terminated" in cs.MIXES[mix])


def test_g15_recordings_every_step(oracle):
    import array_strategies as ast
    undo = ast.register(S, ast.make_g15(S.RewardFunction, S.TerminatedFunction, S.TruncatedFunction), ast.G15_NAMES)
    absent = 0
    try:
        for ep in _load("g15_array_strategies.json.gz")["episodes"]:
            config = ast.g15_config(C, C, C, C, getattr(ast, ep["geometry"]), ep["max_steps"])
            p = lower_config(config, allow_position_only=True, allow_array_form=True)
            a, _ = _replay(f"g15 {ep['geometry']} seed {ep['seed']}", oracle, p, agent_ids(config),
                           np.asarray(ep["initial"], np.int32), ep["steps"], "obs_keys")
            absent += a
    finally:
        undo()
    assert absent > 0


# ---- the 67 recorded batches: begin at every step, finish with the built-in rules ---------------------------------------
def test_all_67_fixtures_are_walked():
    assert len(ALL_NPZ) + len(PLUGIN_NPZ) == 67


@pytest.mark.parametrize("name", ALL_NPZ + PLUGIN_NPZ)
def test_recorded_batches_begin_and_finish(oracle, name):
    import custom_strategies as cs
    plugins = cs.make_position_only(S.RewardFunction, S.TerminatedFunction)      # (g13: the configs name these classes)
    S.REWARD_FUNCTIONS[cs.PO_NAMES["reward"]] = plugins["reward"]
    S.TERMINATED_FUNCTIONS[cs.PO_NAMES["terminated"]] = plugins["terminated"]
    try:
        g = Golden(name)
    finally:
        S.REWARD_FUNCTIONS.pop(cs.PO_NAMES["reward"], None)
        S.TERMINATED_FUNCTIONS.pop(cs.PO_NAMES["terminated"], None)
    rollout = name in ROLLOUT_NPZ
    st = spec.make_state(g.E, g.N, **g.init_state())
    pool = g["pool_xy"] if rollout else None
    off, total = (int(g["env_offset"]), int(g["total_envs"])) if rollout else (0, g.E)
    for s in range(g.K):
        mid, _, _ = spec.begin(g.params, st, g["actions"][s], g["order"][s], oracle=oracle)
        own = spec.resolve_moves(g.params, st, g["actions"][s], g["order"][s])
        np.testing.assert_array_equal(own[0], mid["x"], err_msg=f"{name} step {s}: the spec's own move rule vs the oracle")
        np.testing.assert_array_equal(own[1], mid["y"], err_msg=f"{name} step {s}: the spec's own move rule vs the oracle")
        if name in PLUGIN_NPZ:      # position-only plugins: the recorded values themselves are the arrays
            r, t, u = g["reward"][s], (g["agent_flags"][s] & 1).astype(np.int8), ((g["agent_flags"][s] >> 1) & 1).astype(np.uint8)
        else:
            r, t, u = spec.builtin_arrays(oracle, g.params, mid)
        f = spec.finish(g.params, mid, r, t, u, auto_reset=rollout, pool=pool, env_offset=off, total_envs=total)
        reset = (f.env_flags & 4) != 0
        for k in ("x", "y", "active", "step_count"):      # (a rollout fixture records a resetting env before its reset)
            np.testing.assert_array_equal(mid[k], g[k][s], err_msg=f"{name} step {s}: {k} after begin")
        np.testing.assert_array_equal(f.agent_flags, g["agent_flags"][s], err_msg=f"{name} step {s}")
        np.testing.assert_array_equal(f.env_flags if rollout else f.env_flags & 3, g["env_flags"][s] if rollout else g["env_flags"][s] & 3,
                                      err_msg=f"{name} step {s}")
        live = (g["agent_flags"][s] & 4) != 0
        np.testing.assert_array_equal(f.reward_bits, np.where(live, g["reward"][s], 0.0).view(np.uint64), err_msg=f"{name} step {s}")
        np.testing.assert_array_equal(spec.observe(oracle, g.params, mid).view(np.uint32), g["obs"][s].view(np.uint32))
        for k in ("terminated", "truncated"):
            np.testing.assert_array_equal(np.where(reset[:, None], mid[k] | ((f.agent_flags >> (k == "truncated")) & 1), f.state[k]),
                                          g[k][s], err_msg=f"{name} step {s}: {k}")
        assert not f.state["terminated"][reset].any() and not f.state["truncated"][reset].any() and f.state["active"][reset].all()
        assert f.term_present.all()
        st = f.state
    if rollout:
        np.testing.assert_array_equal(st["episode"], g["final_episode"])


# ---- input adequacy: the seeded inputs of the GPU matrix reach their edges ------------------------------------------------
def _params(n, grid=(12, 8), **kw):
    return lower_config(cases.make_config(*grid, n, **kw))


def test_every_agent_count_meets_every_grid_and_every_batch_class():
    m = cases.matrix_cases()
    assert len(m) == 105 and len(set(m)) == 105
    assert {(n, g) for n, g, _ in m} == {(n, g) for n in cases.AGENT_COUNTS for g in cases.GRIDS}
    assert {(n, c) for n, _, c in m} == {(n, c) for n in cases.AGENT_COUNTS for c in cases.E_CLASSES}
    for n in cases.AGENT_COUNTS:
        G = cases.lane_group(n)
        assert G >= n > G // 2 or n == 1
        assert {cases.class_envs(n, c) for c in cases.E_CLASSES} >= {1, 64 // G + 1, 4 * (64 // G) + 1}
    # the counts whose wave-wide byte run is not a multiple of 4: the byte-wise branch of the small outputs
    assert sorted(n for n in cases.AGENT_COUNTS if ((64 // cases.lane_group(n)) * n) % 4) == [17, 31, 33, 50, 63]
    assert 1 in {min(cases.NUM_BOARDING[n], n - cases.NUM_BOARDING[n]) for n in cases.AGENT_COUNTS if n > 2}


@pytest.mark.parametrize("n", cases.AGENT_COUNTS)
def test_caller_array_family_reaches_its_edges(n):
    p = _params(n)
    rng = np.random.default_rng(1000 + n)
    E = max(64, 16384 // n)
    st = cases.random_state(rng, p, E, n)
    r, t, u = cases.caller_arrays(rng, st)
    f = spec.finish(p, st, r, t, u)
    live = (st["terminated"] == 0) & (st["truncated"] == 0)
    assert ((t == -1).all(axis=1)).any() and not (f.env_flags[(t == -1).all(axis=1)] & 1).any(), "an env whose entries are all -1"
    assert (~live.any(axis=1)).any() and not (f.env_flags[~live.any(axis=1)] & 2).any(), "an env with nobody LIVE"
    assert (live.any(axis=1) & ((f.env_flags & 2) != 0)).any(), "an env where every LIVE agent truncates"
    assert (f.emitted & ~live).any(), "a non-LIVE agent that is emitted"
    assert ((st["truncated"][:, 0] != 0) & (st["terminated"][:, 0] == 0) & (t[:, 0] == 1) & f.emitted[:, 0]).any()
    assert ((f.env_flags & 1) != 0).any() and ((f.env_flags & 3) == 0).any()
    # every combination of the flags before x the values now (t: 1 / 0 / -1 / another byte; u: zero / non-zero)
    tcls = np.select([t == 1, t == 0, t == -1], [0, 1, 2], 3)
    combos = {(a, b, c, d) for a, b, c, d in zip(st["terminated"].ravel(), st["truncated"].ravel(), tcls.ravel(), (u != 0).ravel())}
    assert len(combos) == 2 * 2 * 4 * 2, len(combos)
    assert set(np.unique(t)) == set(cases.TERM_BYTES.tolist()) and set(np.unique(u)) == set(cases.TRUNC_BYTES.tolist())
    assert set(np.unique(r)) == set(cases.REWARD_BITS.tolist())
    assert set(np.unique(f.reward_bits[live])) == set(cases.REWARD_BITS.tolist()) and not f.reward_bits[~live].any()


@pytest.mark.parametrize("n", cases.AGENT_COUNTS)
def test_begin_family_reaches_its_edges(oracle, n):
    p = _params(n)
    st, acts, order = cases.queue_case(p, n, np.random.default_rng(2000 + n))
    m = max(0, min(n - 1, p.width - 1))
    ev = [cases.move_events(p, {k: v[e:e + 1] for k, v in st.items()}, acts[e:e + 1], order[e:e + 1]) for e in range(3)]
    assert ev[0].arrivals == ev[1].arrivals == 1, "the last slot arrives in the step"
    assert ev[0].into_vacated == max(m - 1, 0) and ev[0].blocked == 0, "head first: every follower enters a cell just left"
    assert ev[0].longest_chain == max(m - 1, 0)
    assert ev[1].blocked_by_later == max(m - 1, 0) and ev[1].moves == (1 if m else 0) + 1, "slot order: blocked by later ranks"
    if n >= 5:
        assert ev[0].longest_chain >= 3
    if n >= 3:
        assert ev[1].arrival_with_block == 1, "an arrival in the same step as a block"
    # the spec's own rule and the oracle agree on these (well-formed) inputs, and the counters are what the events say
    assert spec.well_formed_orders(order, n).all()
    with_oracle, mv, ar = spec.begin(p, st, acts, order, oracle=oracle)
    alone, mv2, ar2 = spec.begin(p, st, acts, order)
    for k in spec.STATE_KEYS:
        np.testing.assert_array_equal(with_oracle[k], alone[k], err_msg=k)
    total = cases.move_events(p, st, acts, order)
    assert (mv, ar) == (mv2, ar2) == (total.moves, total.arrivals)


def test_action_byte_classes_over_the_matrix_inputs():
    a = cases.random_actions(np.random.default_rng(5), 64, 8)
    assert {int(v) for v in np.unique(a)} >= {0, 1, 2, 3, 4, 255} and ((a > 4) & (a < 255)).any()
    for n in cases.AGENT_COUNTS:       # the crowds of the begin family: moves, bytes 5 .. 254 and absent agents in every one
        p = _params(n)
        a = cases.queue_case(p, n, np.random.default_rng(2000 + n), E=cases.QUEUE_ENVS)[1]
        assert (a < 4).any() and ((a > 4) & (a < 255)).any() and (a == 255).any(), n


@pytest.mark.parametrize("n", [3, 8, 17])
def test_malformed_orders_follow_the_documented_rule(n):
    """include/ccx.h (ccx_step_begin): an order byte >= N names no agent and moves nothing -- also a byte whose low bits
    name a slot, such as 9 for 8 agents --, a slot named twice moves at most once."""
    p = _params(n)
    rng = np.random.default_rng(3000 + n)
    st, acts, order = cases.queue_case(p, n, rng)
    G = cases.lane_group(n)
    m = min(n - 1, p.width - 1)
    bad = order.copy()
    bad[0, 0] = G + (m - 1)                    # the head's rank now holds a byte >= G whose low bits name the head
    x, y, moved = spec.resolve_moves(p, st, acts, bad)
    assert not moved[0, m - 1], "the head was not named: it stays"
    assert moved[0, :m - 1].sum() == 0, "so nobody behind it can move"
    np.testing.assert_array_equal(spec.resolve_moves(p, st, acts, order)[0][1:], x[1:])      # other envs: unaffected
    twice = order.copy()
    twice[0, 1] = twice[0, 0]                  # the head twice, its follower never
    x2, _, moved2 = spec.resolve_moves(p, st, acts, twice)
    assert moved2[0, m - 1] and x2[0, m - 1] == st["x"][0, m - 1] + 1, "named twice, moved one cell"
    assert not spec.well_formed_orders(bad, n)[0] and not spec.well_formed_orders(twice, n)[0]
    assert spec.well_formed_orders(bad, n)[1:].all()


@pytest.mark.parametrize("P,total,offset", [(1, 10, 0), (3, 10, 0), (10, 10, 0), (11, 10, 0), (5, 20, 7), (7, 20, 13)])
def test_auto_reset_family_resets_for_every_pool_size(P, total, offset):
    n, E = 8, 10 if total == 10 else 7
    p = _params(n)
    rng = np.random.default_rng(4000 + P)
    st = cases.random_state(rng, p, E, n)
    st["episode"] = rng.integers(P, 2**31 - 2, size=E).astype(np.int32)
    st["episode"][0] = 2**31 - 2
    pool = cases.make_pool(rng, p, P, n)
    r, t, u = cases.caller_arrays(rng, st)
    f = spec.finish(p, st, r, t, u, auto_reset=True, pool=pool, env_offset=offset, total_envs=total)
    reset = (f.env_flags & 4) != 0
    assert reset.any() and not reset.all()
    assert (reset == ((f.env_flags & 3) != 0)).all()
    stride = total % P or 1
    for e in np.nonzero(reset)[0]:
        entry = pool[(offset + int(e) + (int(st["episode"][e]) + 1) * stride) % P]
        assert (f.state["x"][e] == entry[:, 0]).all() and (f.state["y"][e] == entry[:, 1]).all()
        assert f.state["episode"][e] == st["episode"][e] + 1 and f.state["step_count"][e] == 0
        assert f.state["active"][e].all() and not f.state["terminated"][e].any() and not f.state["truncated"][e].any()
    assert f.counters["episodes"] == int(reset.sum())
