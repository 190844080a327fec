"""The NumPy / Python-integer spec of CCX_NSTEP (tests/_nstep_spec.py) checked against its second, independent statement
(``brute_force``: steps and flags walked directly, no slots and no head) on oracle trajectories, against CCX_REPLAY's spec at
n = 1, against the constants the library states, and on a synthetic ring whose arrays are written directly so that every
edge of the rule sits at a known record.  No GPU."""

import re
from pathlib import Path

import numpy as np
import pytest
from _nstep_cases import BLOCKS, CAUSES, E, EPSILON, POOL, S, config, count_causes, stagger, synthetic, synthetic_states
from _nstep_spec import (EF_CUT, NSTEP_MAX, avail_spec, brute_force, cut_push_spec, mark_cut_spec, new_cut, nstep_fetch_spec,
                         window_spec)
from _qlearn_spec import make_td_case, td_args, td_loss_backward_spec, td_loss_spec
from _replay_spec import fetch_spec, new_ring, push_spec

from collectivecrossing_amd import _abi

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "collectivecrossing_amd" / "csrc"
CONSTS = (6.0, 4.0, 5.0, 7.0)
SEED = 0x0123_4567_89AB_CDEF
OUT = ("obs", "next_obs", "actions", "reward", "done", "valid", "masks_next", "index")


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint8).reshape(a.shape + (a.itemsize,)) if a.dtype.itemsize > 1 else a


def same(got, want, msg=""):
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, (msg, got.dtype, want.dtype, got.shape, want.shape)
    np.testing.assert_array_equal(_bits(got), _bits(want), err_msg=msg)


def test_constants_are_the_headers():
    text = (CSRC / "ccx_nstep.h").read_text()
    header = (ROOT / "include" / "ccx.h").read_text()
    assert int(re.search(r"kMax = (\d+);", text).group(1)) == NSTEP_MAX == _abi.NSTEP_MAX
    assert int(re.search(r"#define CCX_NSTEP_MAX (\d+)", header).group(1)) == NSTEP_MAX
    flags = {k: int(v, 16) for k, v in re.findall(r"#define (CCX_EF_\w+)\s+(0x[0-9A-Fa-f]+)u", header)}
    assert flags["CCX_EF_ALL_TERMINATED"] | flags["CCX_EF_ALL_TRUNCATED"] | flags["CCX_EF_RESET"] == EF_CUT


def _rollout_blocks(oracle, N, blocks=BLOCKS):
    from collectivecrossing_amd.params import lower_config
    from collectivecrossing_amd.reset import build_reset_pool

    cfg = config(N)
    ob = oracle.OracleBatch(lower_config(cfg), E, 0, E)
    ob.set_reset_pool(build_reset_pool(cfg, POOL["seed0"], POOL["size"]))
    ob.reset_from_pool()
    ob.set_state(step_count=stagger(E))
    ob.set_rng_seed(SEED)
    ob.set_policy_epsilon(EPSILON)
    rng = np.random.default_rng(N)
    out = []
    try:
        for K in blocks:
            acts, _obs, rew, af, ef = ob.rollout_greedy(K, auto_reset=True)
            out.append(dict(obs0_compact=rng.standard_normal((E, N, 4)).astype(np.float32), actions=acts, reward=rew, agent_flags=af,
                            env_flags=ef, obs_compact=rng.standard_normal((K, E, N, 4)).astype(np.float32),
                            final_compact=rng.standard_normal((K, E, N, 4)).astype(np.float32),
                            masks_next=rng.integers(0, 16, (K, E, N), dtype=np.uint8) | 0x10))
    finally:
        ob.set_policy_epsilon(0.0)
    return out


@pytest.mark.parametrize("N", [8, 3])
def test_spec_equals_the_brute_force_on_oracle_trajectories(oracle, N):
    """One block of K = S steps pushed into an empty ring: record (s, e) is slot s * E + e."""
    blk, = _rollout_blocks(oracle, N, blocks=(S,))
    ring, cut = new_ring(S, E, N), new_cut(S, E)
    push_spec(ring, **blk)
    cut_push_spec(cut, int(ring["state"][0]), S, E, blk["env_flags"])
    assert cut.any() and not cut.all() and (blk["agent_flags"] & 1).any()
    index = np.arange(S * E)
    for n in (1, 2, 3, 5, 6):
        for gamma in (0.99, 1.0, 0.0):
            got = nstep_fetch_spec(ring, cut, index, n, gamma, CONSTS, details=True)
            want = brute_force(blk["reward"], blk["agent_flags"], blk["env_flags"], n, gamma)
            for k in ("reward", "discount", "span", "done", "valid"):
                same(got[k], want[k].reshape((S * E,) + want[k].shape[2:]), f"n {n} gamma {gamma}: {k}")
            last = np.array([w["last"] for w in got["windows"]])
            same(last, (want["last"] * E + np.arange(E)[None, :]).reshape(-1), f"n {n}: the record the window ends on")
            same(got["next_obs"], fetch_spec(ring, last, CONSTS)["next_obs"])
            same(got["masks_next"], ring["masks_next"][last])


@pytest.mark.parametrize("N", [8, 3])
def test_n1_is_the_rings_own_fetch_and_the_case_holds_every_ending(oracle, N):
    ring, cut = new_ring(S, E, N), new_cut(S, E)
    total = dict.fromkeys(CAUSES, 0)
    index = np.concatenate([np.arange(S * E), [-1, S * E, 5, 5]])
    for blk in _rollout_blocks(oracle, N):
        push_spec(ring, **blk)
        cut_push_spec(cut, int(ring["state"][0]), S, E, blk["env_flags"])
        got, want = nstep_fetch_spec(ring, cut, index, 1, 0.99, CONSTS), fetch_spec(ring, index, CONSTS)
        for k in OUT:
            same(got[k], want[k], f"n = 1: {k}")
        assert (got["span"] == 1).all() and (got["discount"] == np.float32(0.99)).all()
        for k, v in count_causes(ring, cut, index, 3).items():
            total[k] += v
    print(N, total)
    assert all(total[k] > 0 for k in CAUSES), total              # what tests/test_gpu_nstep.py asks of the same case on the device


def test_cut_bytes():
    S_, E_ = 4, 3
    cut = new_cut(S_, E_)
    ef = np.array([[0, 1, 2], [4, 8, 0x10], [6, 0, 0xF8]], np.uint8)
    cut_push_spec(cut, 3, S_, E_, ef)                                    # pushed at head 0
    assert cut.tolist() == [0, 1, 1, 1, 0, 0, 1, 0, 0, 0, 0, 0]
    cut_push_spec(cut, 6, S_, E_, ef)                                    # pushed at head 3: ring steps 3, 0, 1
    assert cut.tolist() == [1, 0, 0, 1, 0, 0, 1, 0, 0, 0, 1, 1]
    mark_cut_spec(cut, 0, S_, E_)                                        # an empty ring: nothing
    assert cut.sum() == 5
    mark_cut_spec(cut, 6, S_, E_, np.array([0, 7, 0], np.uint8))         # newest step: (6 - 1) mod 4 = 1
    assert cut[3:6].tolist() == [1, 1, 0]
    mark_cut_spec(cut, 9, S_, E_)                                        # step 0, every env
    assert cut[0:3].tolist() == [1, 1, 1]


def test_availability():
    assert [avail_spec(0, p, 5) for p in range(5)] == [0] * 5
    assert [avail_spec(3, p, 5) for p in range(5)] == [2, 1, 0, 0, 0]
    assert [avail_spec(5, p, 5) for p in range(5)] == [4, 3, 2, 1, 0]
    assert [avail_spec(7, p, 5) for p in range(5)] == [1, 0, 4, 3, 2]
    assert [avail_spec(5 * 10**12 + 2, p, 5) for p in range(5)] == [1, 0, 4, 3, 2]


def test_synthetic_ring_holds_every_edge():
    ring, cut, where = synthetic()
    N, R = ring["N"], 10
    w = {k: window_spec(ring, cut, i, 3, 0.5) for k, i in where.items()}
    assert w["by_n"]["why"] == "n" and w["by_n"]["m_env"] == 3 and not w["by_n"]["wraps"]
    assert w["wraps"]["why"] == "n" and w["wraps"]["wraps"] and w["wraps"]["last"] == 0 * 2 + 0
    assert w["by_avail"]["why"] == "avail" and w["by_avail"]["m_env"] == 2
    assert w["newest"]["why"] == "avail" and w["newest"]["m_env"] == 1 and (w["newest"]["span"] == 1).all()
    assert w["by_cut"]["why"] == "cut" and w["by_cut"]["m_env"] == 2
    e = w["agent_early"]
    assert e["m_env"] == 3 and e["span"].tolist() == [1, 1, 3] and e["done"].tolist() == [1, 0, 0]
    assert e["dropped"].tolist() == [False, True, False] and e["valid"].tolist() == [4, 0, 4]
    assert e["discount"].tolist() == [0.5, 0.5, 0.125]
    assert np.isnan(e["reward"][2]) and not np.isnan(e["reward"][:2]).any()          # a NaN inside the window goes through
    assert not np.isnan(w["nan_just_beyond"]["reward"]).any()                        # one just beyond it reaches nothing
    assert np.isnan(ring["reward"][((0 + 2) % 5) * 2 + 0, 2])
    # the f64 chain of a full window, by hand
    r = ring["reward"][[4, 6, 8], 0]
    assert w["by_n"]["reward"][0] == np.float64(r[0] + np.float64(0.5) * r[1]) + np.float64(0.25) * r[2]
    # heads: rewritten, empty, partly filled (p >= head), full
    seen = set()
    for head, what in synthetic_states():
        ring["state"][0] = head
        mb = nstep_fetch_spec(ring, cut, np.array([-1, R] + list(range(R))), 3, 0.5, CONSTS, details=True)
        assert (mb["span"][:2] == 1).all() and (mb["discount"][:2] == np.float32(0.5)).all() and (mb["actions"][:2] == 255).all()
        assert not mb["valid"][:2].any() and not _bits(mb["reward"][:2]).any()
        for i, wdw in enumerate(mb["windows"][2:]):
            p = i // 2
            if head == 0 or (head < 5 and p >= head):
                assert wdw["m_env"] == 1, (what, i)
                seen.add("nothing behind it")
            seen.add(what)
    assert len(seen) == 6
    one = nstep_fetch_spec(ring, cut, np.arange(R), 1, 0.5, CONSTS)
    plain = fetch_spec(ring, np.arange(R), CONSTS)
    for k in OUT:
        same(one[k], plain[k], k)


def test_a_discount_per_row_in_the_td_rule():
    """tests/_qlearn_spec.py takes ``gamma`` as an array [M] as it stands: one value everywhere gives the scalar's bits, and
    every row of a mixed array gives the bits of a call with that row's own value."""
    M = 300
    case = make_td_case(M, seed=4)
    kw = td_args(case, True, True, True, True)
    full = np.full(M, 0.99, np.float32)
    s0, t0 = td_loss_spec(**kw, gamma=0.99)
    s1, t1 = td_loss_spec(**kw, gamma=full)
    same(s0, s1), same(t0, t1)
    same(td_loss_backward_spec(**kw, gamma=0.99, stats=s0), td_loss_backward_spec(**kw, gamma=full, stats=s0))
    mixed = np.random.default_rng(2).choice(np.array([0.0, 0.99, 0.9801, 1.0, 0.5], np.float32), M)
    _, tm = td_loss_spec(**kw, gamma=mixed)
    for g in np.unique(mixed):
        _, tg = td_loss_spec(**kw, gamma=float(g))
        same(tm[mixed == g], tg[mixed == g], f"rows with discount {g}")
