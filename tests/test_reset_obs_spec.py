"""CCX_RESET_OBS_NEXT on the CPU: the NumPy spec (tests/_reset_obs_spec.py) against the oracle's own resets, and the
conditions the GPU cases rely on (enough restarts, one on a launch's last step, several per env in one launch)."""

import numpy as np
import pytest
from _reset_obs_spec import CASES, EF_RESET, SENTINEL, Case, compact_of, next_mode, pool_entry, restart_conditions

ORACLE_CASES = [n for n, c in CASES.items() if c.get("drive", "tensor") in ("tensor", "greedy")]


@pytest.fixture(scope="module")
def cases(oracle):
    return {n: Case(n, oracle) for n in ORACLE_CASES}


def _u32(a):
    return np.ascontiguousarray(a).view(np.uint32)


def test_cursor_formula():
    assert pool_entry(5, 0, 37, 67) == 5 and pool_entry(40, 2, 37, 67) == (40 + 2 * 30) % 37
    assert pool_entry(3, 4, 8, 64) == 7          # P divides total_envs: stride 1


@pytest.mark.parametrize("name", ORACLE_CASES)
def test_cases_restart_often_enough_and_on_a_last_step(cases, name):
    c = cases[name]
    restart_conditions(name, [ch["env_flags"] for ch in c.oracle_chunks])
    if name.startswith("greedy"):   # restarts from __all__ terminated as well as from truncation
        ef = np.concatenate([ch["env_flags"] for ch in c.oracle_chunks], 0)
        r = (ef & EF_RESET) != 0
        assert (r & ((ef & 1) != 0)).any() and (r & ((ef & 3) == 2)).any()


@pytest.mark.parametrize("name", ORACLE_CASES)
def test_restart_on_a_last_step_equals_the_oracles_observe(cases, name):
    c = cases[name]
    seen = 0
    for ch in c.oracle_chunks:
        obs, compact, _, _, ep = c.spec(ch)
        assert np.array_equal(ep, ch["episode_after"])
        last = (ch["env_flags"][-1] & EF_RESET) != 0
        seen += int(last.sum())
        assert np.array_equal(_u32(obs[-1][last]), _u32(ch["observe_after"][last]))
        assert np.array_equal(compact[-1][last][..., 3], np.ones_like(compact[-1][last][..., 3]))
    assert seen > 0


@pytest.mark.parametrize("name", ["k1_n5", "k16_n8_five_restarts", "k40_n33"])
def test_rows_without_reset_are_untouched_and_finals_hold_the_terminal_rows(cases, name):
    c = cases[name]
    for ch in c.oracle_chunks:
        obs, compact, fo, fc, _ = c.spec(ch)
        r = (ch["env_flags"] & EF_RESET) != 0
        t_cmp = compact_of(ch["obs"], ch["agent_flags"], c.params.num_boarding)
        assert np.array_equal(_u32(obs[~r]), _u32(ch["obs"][~r])) and np.array_equal(_u32(compact[~r]), _u32(t_cmp[~r]))
        assert (fo[~r].view(np.uint8) == SENTINEL).all() and (fc[~r].view(np.uint8) == SENTINEL).all()
        assert np.array_equal(_u32(fo[r]), _u32(ch["obs"][r])) and np.array_equal(_u32(fc[r]), _u32(t_cmp[r]))
        assert r.any() and not np.array_equal(_u32(obs[r]), _u32(ch["obs"][r]))


@pytest.mark.parametrize("cut", [1, 3, 16])
def test_the_same_steps_cut_into_launches_give_the_same_arrays(oracle, cases, cut):
    c = cases["k40_n8"]
    ref = [c.spec(ch) for ch in c.oracle_chunks]
    whole = [np.concatenate([r[q] for r in ref], 0) for q in range(4)]
    ob = c.new_oracle(oracle)
    acts = np.concatenate(c.actions, 0)
    parts = []
    for k0 in range(0, len(acts), cut):
        ep0 = ob.episode.copy()
        obs, _, af, ef = ob.rollout(acts[k0:k0 + cut], None, auto_reset=True)
        z = np.frombuffer(bytes([SENTINEL]) * obs.nbytes, np.float32).reshape(obs.shape)
        cmp_ = compact_of(obs, af, c.params.num_boarding)
        zc = np.frombuffer(bytes([SENTINEL]) * cmp_.nbytes, np.float32).reshape(cmp_.shape)
        parts.append(next_mode(obs, cmp_, ef, c.pool, c.env_offset, c.total_envs, ep0, c.params, z, zc))
    for q in range(4):
        assert np.array_equal(_u32(np.concatenate([p[q] for p in parts], 0)), _u32(whole[q])), q
