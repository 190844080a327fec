"""The step rule of csrc/ccx_step_rule.h -- the very source every stepping kernel inlines and build_cell_table loops over --
compiled for the host (-O2 -ffp-contract=off) and run against independent statements: the cell word against the reference's
predicates written out here and the spec's ``cell_ok``, the reward of a cell against what the CPU oracle pays an agent that
waits on it (u64 bit patterns), the flag bytes against include/ccx.h:81-94, the pool cursor against the spec.  No GPU."""

import ctypes as C
import itertools
import subprocess
from pathlib import Path

import _far_shard_cases as far
import _split_step_cases as cases
import _split_step_spec as spec
import numpy as np
import pytest
from test_mlp_host_rule import CSRC, _compiler, _p

from collectivecrossing_amd import configs as CFG
from collectivecrossing_amd._abi import REWARD_MODES
from collectivecrossing_amd.params import lower_config

U64 = C.c_ulonglong


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    cxx = _compiler()
    if cxx is None:
        pytest.skip("no host C++ compiler (c++, clang++ or ROCm's clang++)")
    so = tmp_path_factory.mktemp("step_rule_host") / "libstep_rule_host.so"
    subprocess.run([cxx, "-std=c++17", "-O2", "-ffp-contract=off", "-fPIC", "-shared", f"-I{CSRC}",
                    str(Path(__file__).with_name("step_rule_host.cpp")), "-o", str(so)], check=True)
    lib = C.CDLL(str(so))
    lib.host_cell_reward.restype = C.c_double
    lib.host_cell_reward.argtypes = [U64, C.c_int, C.c_int, C.c_int] + [C.c_double] * 6
    lib.host_cell_fields.argtypes = [U64, C.c_int, C.c_void_p]
    lib.host_agent_flag_byte.restype = lib.host_env_flag_byte.restype = C.c_uint32
    lib.host_pool_entry.restype = lib.host_pool_stride.restype = U64
    lib.host_pool_entry.argtypes = [U64] * 4
    lib.host_pool_stride.argtypes = [U64] * 2
    return lib


def bench_config(reward, nb=1, ne=1):
    """The benchmark's 12 x 8 geometry (bench.py), here with one agent of each type."""
    return CFG.CollectiveCrossingConfig(
        width=12, height=8, division_y=4, tram_door_left=5, tram_door_right=7, tram_length=9, num_boarding_agents=nb,
        num_exiting_agents=ne, exiting_destination_area_y=0, boarding_destination_area_y=8,
        reward_config=CFG.get_reward_config(reward), truncated_config=CFG.MaxStepsTruncatedConfig(max_steps=50))


def off_centre_config(reward):
    """Door columns 3 and 8: the door centre (3 + 8) / 2 rounds down to 5."""
    kw = dict(width=13, height=9, division_y=5, tram_door_left=2, tram_door_right=7, tram_length=11, num_boarding_agents=1,
              num_exiting_agents=1, exiting_destination_area_y=0, boarding_destination_area_y=9,
              reward_config=CFG.get_reward_config(reward), terminated_config=CFG.get_terminated_config("individual_at_destination"),
              truncated_config=CFG.MaxStepsTruncatedConfig(max_steps=50), strict_reference_limits=False)
    try:
        return CFG.CollectiveCrossingConfig(**kw)
    except ValueError:
        kw.setdefault("observation_config", CFG.DefaultObservationConfig())
        kw.setdefault("render_mode", None)
        return CFG.CollectiveCrossingConfig.model_construct(**kw)


def geometry_cases():
    """(name, params, terminated tables or None): both 12 x 8 geometries under each reward mode, one config with a user
    terminated table that differs from the destination rows, one whose door centre rounds."""
    out = []
    for mode in REWARD_MODES:
        out.append((f"bench-{mode}", lower_config(bench_config(mode)), None))
        out.append((f"smallest-{mode}", lower_config(cases.make_config(12, 8, 2, nb=1, reward=mode)), None))
    p = lower_config(cases.make_config(12, 8, 2, nb=1))
    rng = np.random.default_rng(11)
    tables = tuple((rng.random((p.height + 1, p.width + 1)) < 0.3).astype(np.uint8) * rng.integers(1, 255, dtype=np.uint8) for _ in range(2))
    assert any((t[dy] == 0).any() and t[np.arange(p.height + 1) != dy].any()
               for t, dy in zip(tables, (p.boarding_dest_y, p.exiting_dest_y)))
    out.append(("smallest-terminated-table", p, tables))
    q = lower_config(off_centre_config("default"))
    assert (q.door_left + q.door_right) % 2 == 1
    out.append(("off-centre-door", q, None))
    return out


GEOMETRIES = geometry_cases()


def cell_table(host, p, tables):
    geom = np.array([p.width, p.height, p.division_y, p.tram_left, p.tram_right, p.door_left, p.door_right, p.boarding_dest_y,
                     p.exiting_dest_y], np.int32)
    tab = np.full((p.height + 3, p.width + 3), 2**64 - 1, np.uint64)
    tb, te = (None, None) if tables is None else (np.ascontiguousarray(t, np.uint8) for t in tables)
    host.host_cell_table(_p(geom), p.reward_mode, _p(tb), _p(te), _p(tab))
    return tab, geom


def fields(host, word, boarding):
    out = np.zeros(10, np.int32)
    host.host_cell_fields(U64(int(word)), int(boarding), _p(out))
    return [int(v) for v in out]


@pytest.mark.parametrize("name, p, tables", GEOMETRIES, ids=[g[0] for g in GEOMETRIES])
def test_cell_words_equal_the_reference_predicates(host, name, p, tables):
    tab, geom = cell_table(host, p, tables)
    W, H, Wp = p.width, p.height, p.width + 3
    assert not tab[0].any() and not tab[-1].any() and not tab[:, 0].any() and not tab[:, -1].any()      # the border cells
    ys, xs = np.mgrid[0:H + 1, 0:W + 1]
    want_legal = sum(spec.cell_ok(p, xs + dx, ys + dy).astype(np.int64) << a for a, (dx, dy) in enumerate(((1, 0), (0, 1), (-1, 0), (0, -1))))
    for y in range(H + 1):
        for x in range(W + 1):
            word = tab[y + 1, x + 1]
            assert host.host_cell_index(x, y, Wp) == (y + 1) * Wp + x + 1
            assert host.host_cell_of_placement(x | (y << 8), Wp) == (y + 1) * Wp + x + 1
            assert host.host_cell_ok(_p(geom), x, y) == int(spec.cell_ok(p, np.int64(x), np.int64(y)))
            in_tram = y >= p.division_y and p.tram_left <= x <= p.tram_right                       # collectivecrossing.py:551-554
            at_door = y == p.division_y and (x == p.door_left - 1 or x == p.door_right + 1)        # :556-563
            for boarding in (1, 0):
                legal, legal4, info, fx, fy, dest, term, _, _, bytes_ok = fields(host, word, boarding)
                assert legal == legal4 == want_legal[y, x], (x, y)                                # bits 0-3; bit 4 (wait) is 0
                assert info == (spec.AF_IN_TRAM_AREA if in_tram else 0) | (spec.AF_AT_DOOR if at_door else 0), (x, y)
                assert (fx, fy, bytes_ok) == (x, y, 1)
                on_dest = y == (p.boarding_dest_y if boarding else p.exiting_dest_y)               # :663-683
                assert dest == int(on_dest), (x, y, boarding)
                want_term = on_dest if tables is None else bool(tables[0 if boarding else 1][y, x])   # terminateds.py:66-82
                assert term == int(want_term), (x, y, boarding)
    assert host.host_cell_origin(Wp) == Wp + 1
    for x, y in ((-1, 0), (0, -1), (W + 1, 0), (0, H + 1)):
        assert host.host_cell_ok(_p(geom), x, y) == 0


@pytest.mark.parametrize("name, p, tables", GEOMETRIES, ids=[g[0] for g in GEOMETRIES])
def test_cell_reward_equals_what_the_oracle_pays_a_waiting_agent(host, oracle, name, p, tables):
    """One env per legal cell: the boarding agent (slot 0) waits on the cell, the exiting agent (slot 1) on the next legal
    cell; both are live.  u64 bit patterns, the sign of zero included."""
    assert (p.num_boarding, p.num_exiting) == (1, 1)
    tab, _ = cell_table(host, p, tables)
    cells = cases.legal_cells(p)
    E = len(cells)
    other = np.roll(cells, -1, axis=0)
    ob = oracle.OracleBatch(p, E)
    ob.set_state(x=np.stack([cells[:, 0], other[:, 0]], 1), y=np.stack([cells[:, 1], other[:, 1]], 1))
    _, rew, af, _ = ob.step(np.full((E, 2), 4, np.uint8), None, want_obs=False)
    assert (af & spec.AF_LIVE).all()

    def paid(xy, boarding, live=1):
        return host.host_cell_reward(U64(int(tab[xy[1] + 1, xy[0] + 1])), boarding, live, p.reward_mode, p.boarding_destination_reward,
                                     p.tram_door_reward, p.tram_area_reward, p.distance_penalty_factor, p.no_goal_reward, p.step_penalty)

    got = np.array([[paid(cells[e], 1), paid(other[e], 0)] for e in range(E)], np.float64)
    np.testing.assert_array_equal(got.view(np.uint64), rew.view(np.uint64))
    done = np.array([paid(cells[e], b, live=0) for e in range(E) for b in (0, 1)], np.float64)
    assert not done.view(np.uint64).any()                                                         # rewards.py:64: +0.0 unless live
    if p.reward_mode == REWARD_MODES["default"]:
        assert (rew == 0.0).any() and len(np.unique(rew)) > 6                                      # distance 0, and every class


def test_flag_bytes_equal_the_header(host):
    """include/ccx.h:81-89, exhaustively: the flags this step raises x the flags before x active x at-destination x the two
    info bits (256 cases, for either agent type); :91-94 for the env byte (4 x 2)."""
    n = 0
    for out2, before, act, dest, in_tram, at_door in itertools.product(range(4), range(4), range(2), range(2), range(2), range(2)):
        live = before == 0
        emitted = live or bool(out2 & ~before)
        want = ((out2 & 1) * spec.AF_TERMINATED | (out2 >> 1) * spec.AF_TRUNCATED | live * spec.AF_LIVE | emitted * spec.AF_OBS |
                in_tram * spec.AF_IN_TRAM_AREA | at_door * spec.AF_AT_DOOR | act * spec.AF_ACTIVE | dest * spec.AF_AT_DEST)
        for boarding in (1, 0):
            mine, theirs = (8, 12) if boarding else (12, 8)
            lo = 0x0703000F | (in_tram << 5) | (at_door << 6) | (dest << mine) | ((1 - dest) << theirs) | (0b110 << mine)
            assert host.host_agent_flag_byte(out2, before, lo, boarding, act) == want, (out2, before, act, dest, in_tram, at_door)
        n += 1
    assert n == 256
    for ef, resets in itertools.product(range(4), range(2)):
        assert host.host_env_flag_byte(ef, resets) == ef | (spec.EF_RESET if ef and resets else 0)


def test_pool_cursor_equals_the_spec(host):
    globals_ = sorted({c.env_offset + e for c in far.CASES.values() for e in (0, 1, 29, 30, c.E - 1)} | {0, 1, 5})
    for P in (1, 2, 3, 7, 1024):
        for total in sorted({P, 7 * P, P + 1, 2 * P - 1, 1}):            # stride 0 -> the "1" rule (twice), 1, P - 1
            stride = host.host_pool_stride(total, P)
            assert stride == (total % P or 1) % P, (total, P)
            for episode in (0, 1, P, 2**31 - 2):
                for g in globals_:
                    want = spec.pool_entry(g, episode, P, total)
                    assert host.host_pool_entry(g, episode, stride, P) == want, (g, episode, total, P)
    for c in far.CASES.values():                                         # the far shards' own pools, strides and episodes
        stride = host.host_pool_stride(c.total_envs, c.P)
        assert stride == c.stride % c.P
        for e in (0, 29, 30, c.E - 1):
            for j in (c.episode0, c.episode0 + far.K):
                assert host.host_pool_entry(c.env_offset + e, j, stride, c.P) == spec.pool_cursor(c.env_offset, c.total_envs, c.P, e, j)
