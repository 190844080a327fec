"""Far shards and late episodes on the CPU: the case table of tests/_far_shard_cases.py is ADEQUATE (every wrong-width
model of the reset-pool cursor is exposed by one of its cases), and the C oracle -- i64 throughout -- equals the cursor of
include/ccx.h in Python integers on all of them.  The refusal of ccx_create for a shard that reaches past total_envs is here
too: the range check runs before any device call."""

import ctypes as C

import _far_shard_cases as far
import numpy as np
import pytest
from _split_step_spec import pool_cursor

EF_RESET = 0x04
INT64_MAX = (1 << 63) - 1


# ------------------------------------------------------------------------------------------------ the case table
def test_the_table_holds_what_the_issue_asks_for():
    cs = list(far.CASES.values())
    for c in cs:
        assert 0 <= c.env_offset and c.env_offset + c.E <= c.total_envs and c.E in (67, 130), c.name
        assert int(c.episodes().max()) + far.K < (1 << 31) - 1, c.name          # no counter passes INT32_MAX
    assert any(c.env_offset < 1 << 31 < c.env_offset + c.E for c in cs)
    # (tiles hold a power-of-two number of envs: a wrap at an odd local index falls inside a tile of two envs and more)
    assert any(c.env_offset < 1 << 32 < c.env_offset + c.E and ((1 << 32) - c.env_offset) % 2 for c in cs)
    assert any(c.env_offset >= 1 << 40 for c in cs)
    assert any(c.env_offset + c.E == 1 << 32 for c in cs) and any(c.env_offset == 1 << 32 for c in cs)
    big = [c for c in cs if c.P > 92_682]
    assert all(c.total_envs >= 1 << 32 for c in cs)
    assert any(c.stride > 65_536 and c.stride != c.P - 1 for c in big)
    assert any(c.total_envs % c.P == 0 and c.stride == 1 for c in big) and any(c.stride == c.P - 1 for c in big)
    assert any(c.P == 1 for c in cs) and any(1 < c.P < 100 for c in cs)
    assert any((1 << 31) - 400 <= c.episode0 < (1 << 31) - 200 for c in cs)
    assert any(1 << 16 < c.episode0 < (1 << 16) + 100 for c in cs)
    assert any((c.episode0 % c.P) * c.stride > 1 << 32 for c in big)


def test_the_pool_is_the_seeded_one_and_its_entries_differ():
    """The shared pool is `build_reset_pool`'s (checked on a prefix: the Python loop is slow), and a wrong cursor shows:
    at least 99 % of the entries differ from their neighbour at distance 1 and at every stride the table uses."""
    from collectivecrossing_amd.reset import build_reset_pool
    pool = far.pool(far.P_BIG)
    assert pool.shape == (far.P_BIG, far.N, 2) and pool.dtype == np.uint8
    assert np.array_equal(pool[:1500], build_reset_pool(far.config(), far.POOL_SEED, 1500))
    assert np.array_equal(far.pool(37), pool[:37]) and np.array_equal(far.pool(1), pool[:1])
    for P in sorted({c.P for c in far.CASES.values()} - {1}):
        p = far.pool(P)
        for d in sorted({1} | {c.stride for c in far.CASES.values() if c.P == P}):
            differ = (p != np.roll(p, -d, axis=0)).any(axis=(1, 2))
            assert differ.mean() >= 0.99, (P, d, float(differ.mean()))


def _exposure(model, case):
    """Fraction of the case's (env, restart) pairs at which the model points to ANOTHER PLACEMENT than the spec."""
    pool = far.pool(case.P)
    a = (case.env_offset, case.total_envs, case.P)
    pairs = far.cursor_pairs(case)
    hit = sum(bool((pool[model(*a, e, j)] != pool[pool_cursor(*a, e, j)]).any()) for e, j in pairs)
    return hit / len(pairs)


# the case that exposes each model (the adequacy condition names it; any other case may expose it as well)
EXPOSED_BY = dict(u32_product="far40", u32_global="edge32_above", i32_global="cross31", u32_total="cross31")


@pytest.mark.parametrize("model", list(far.MODELS))
def test_every_wrong_width_model_is_exposed_by_a_case(model):
    assert set(EXPOSED_BY) == set(far.MODELS)
    by_case = {name: _exposure(far.MODELS[model], c) for name, c in far.CASES.items()}
    print(model, {k: round(v, 3) for k, v in by_case.items()})
    assert by_case[EXPOSED_BY[model]] >= 0.5, (model, by_case)


def test_the_product_model_needs_both_residues_large():
    """Why P must exceed 92 682: below it no product of two residues reaches 2^32 and the u32-product model IS the spec."""
    c = far.CASES["far40"]
    assert (c.episode0 % c.P) * c.stride > 1 << 32
    for e, j in far.cursor_pairs(c)[:50]:
        assert far.model_u32_product(c.env_offset, c.total_envs, 70_001, e, j) == pool_cursor(c.env_offset, c.total_envs, 70_001, e, j)


def test_the_incremental_walk_is_the_closed_form():
    """The rollout kernel's walk `idx += stride; if (idx >= P) idx -= P` from a closed-form start, in exact integers."""
    for c in far.CASES.values():
        a = (c.env_offset, c.total_envs, c.P)
        for e, j0 in ((0, c.episode0), (c.E - 1, c.episode0 + 4)):
            idx = pool_cursor(*a, e, j0)
            for j in range(j0 + 1, j0 + 40):
                idx += c.stride % c.P
                idx -= c.P if idx >= c.P else 0
                assert idx == pool_cursor(*a, e, j), (c.name, e, j)


# ------------------------------------------------------------------------------------------------ the oracle
@pytest.mark.parametrize("name", list(far.CASES))
def test_oracle_reset_from_pool_equals_the_cursor(oracle, name):
    c = far.CASES[name]
    pool, ep = far.pool(c.P), c.episodes()
    ob = far.new_oracle(c)
    want = np.stack([pool[pool_cursor(c.env_offset, c.total_envs, c.P, e, int(ep[e]))] for e in range(c.E)])
    assert np.array_equal(ob.x, want[..., 0]) and np.array_equal(ob.y, want[..., 1])
    # with a mask, three episodes later: masked envs move to the new entry, the others keep theirs
    mask = (np.arange(c.E) % 3 != 1).astype(np.uint8)
    ob.set_state(episode=ep + 3)
    ob.reset_from_pool(mask)
    later = np.stack([pool[pool_cursor(c.env_offset, c.total_envs, c.P, e, int(ep[e]) + 3)] for e in range(c.E)])
    want = np.where(mask[:, None, None] != 0, later, want)
    assert np.array_equal(ob.x, want[..., 0]) and np.array_equal(ob.y, want[..., 1])


@pytest.mark.parametrize("name", list(far.CASES))
def test_oracle_auto_reset_rollout_equals_the_cursor(oracle, name):
    """Step by step, so that the placement behind every restart is seen before the next step moves it."""
    c = far.CASES[name]
    pool, acts = far.pool(c.P), far.inputs(name)[0]
    ob = far.new_oracle(c)
    restarts = np.zeros(c.E, np.int64)
    for s in range(far.K):
        ep_before = ob.episode.copy()
        ef = ob.rollout(acts[s][None], auto_reset=True, want_obs=False)[3][0]
        for e in np.nonzero(ef & EF_RESET)[0]:
            assert ob.episode[e] == ep_before[e] + 1
            xy = pool[pool_cursor(c.env_offset, c.total_envs, c.P, int(e), int(ob.episode[e]))]
            assert np.array_equal(ob.x[e], xy[:, 0]) and np.array_equal(ob.y[e], xy[:, 1]), (name, s, int(e))
            restarts[e] += 1
    assert restarts.min() >= far.RESTARTS, (name, int(restarts.min()))
    # the whole-rollout reference the GPU tests compare with is this run
    ref = far.tensor_reference(name)
    assert all(np.array_equal(ref.state[k], getattr(ob, k)) for k in ref.state) and ref.counters == ob.counters.as_dict()


# ------------------------------------------------------------------------------------------------ ccx_create
def _create(num_envs, env_offset, total_envs):
    from collectivecrossing_amd import _lib
    if not _lib.LIB_PATH.exists():
        pytest.skip("libccx.so not built (run __graft_entry__.build())")
    lib = _lib.load()
    handle = C.c_void_p()
    rc = lib.ccx_create(C.byref(far.params()), num_envs, env_offset, total_envs, 0, None, C.byref(handle))
    return lib, rc, handle


@pytest.mark.parametrize("num_envs,env_offset,total_envs", [
    (4, INT64_MAX - 2, INT64_MAX),         # env_offset + num_envs overflows i64: the sum form of the check let it through
    (4, INT64_MAX, INT64_MAX), (4, 1, 4), (4, 0, 3), (4, (1 << 32) - 3, 1 << 32)])
def test_ccx_create_refuses_a_shard_past_total_envs(num_envs, env_offset, total_envs):
    lib, rc, handle = _create(num_envs, env_offset, total_envs)
    assert rc != 0 and not handle.value
    msg = lib.ccx_last_error().decode()
    assert f"env_offset {env_offset} + num_envs {num_envs} exceeds total_envs {total_envs}" in msg, msg
