"""The NumPy restatement of CCX_GAE (tests/_gae_spec.py) against the header's pseudo-code run literally, and the
properties the header states: lam = 0 gives TD errors, gamma = lam = 1 with zero values gives rewards-to-go, nothing the rule
does not read reaches a result, an episode boundary stops the carry.  No GPU."""

import numpy as np
import pytest
from _gae_spec import F32, bits32, gae_scalar, gae_spec, make_gae_case, step_classes

# (K, E, N): one step, two, odd lengths, every env-flag layout of the generator (E >= 7), one agent, many agents
SHAPES = [(1, 7, 3), (2, 7, 1), (3, 9, 2), (5, 8, 3), (9, 14, 1), (12, 7, 8), (17, 9, 5), (20, 15, 2), (33, 7, 3), (40, 8, 4)]
CASES = [(K, E, N, seed, bool((seed + n) % 2)) for n, (K, E, N) in enumerate(SHAPES) for seed in (1, 2)]


def _args(case):
    return (case["reward"], case["agent_flags"], case["env_flags"], case["values"], case["last_values"], case["final_values"])


@pytest.mark.parametrize("K,E,N,seed,with_final", CASES)
def test_vectorised_spec_equals_the_scalar_loop(K, E, N, seed, with_final):
    case = make_gae_case(K, E, N, seed, with_final)
    for gamma, lam in ((0.99, 0.95), (1.0, 1.0), (0.9, 0.0), (0.0, 0.5)):
        got = gae_spec(*_args(case), gamma=gamma, lam=lam)
        want = gae_scalar(*_args(case), gamma=gamma, lam=lam)
        for g, w, name in zip(got, want, ("advantages", "returns", "valid")):
            np.testing.assert_array_equal(bits32(g), bits32(w), err_msg=f"{name} gamma {gamma} lam {lam}")


def test_generator_covers_the_rule_and_no_nan_reaches_an_output():
    seen = np.zeros(4, np.int64)
    for K, E, N, seed, with_final in CASES:
        case = make_gae_case(K, E, N, seed, with_final)
        live, term, cut, cont = step_classes(case["agent_flags"], case["env_flags"])
        seen += [int((~live).sum()), int(term.sum()), int(cut.sum()), int(cont.sum())]
        assert np.isnan(case["reward"]).any() or live.all()
        assert np.isnan(case["values"]).any() or K * E * N < 30
        if with_final:
            assert np.isnan(case["final_values"][~cut]).all() and not np.isnan(case["final_values"][cut]).any()
        adv, ret, valid = gae_spec(*_args(case))
        assert not np.isnan(adv).any() and not np.isnan(ret).any()
        assert np.array_equal(valid, live.astype(np.uint8))
        assert not bits32(adv)[~live].any() and not bits32(ret)[~live].any()          # +0.0, not -0.0
    assert (seen > 100).all(), seen
    big = make_gae_case(40, 8, 4, 1, True)
    sub = np.abs(big["values"][np.isfinite(big["values"])])
    assert ((sub > 0) & (sub < 1.17e-38)).any() and (sub > 1.0).any()                    # subnormals and ordinary values
    assert np.signbit(big["values"][big["values"] == 0]).any()                           # -0.0


def test_lam_zero_gives_td_errors():
    """With lam = 0 the carry never matters: every step is (r + gamma * nv) - v, then + (+0.0 * c).  Computed here for all
    steps at once from shifted arrays, without a backward loop."""
    K, E, N = 33, 9, 5
    case = make_gae_case(K, E, N, 5, True)
    gamma = 0.97
    adv, ret, _ = gae_spec(*_args(case), gamma=gamma, lam=0.0)
    live, term, cut, cont = step_classes(case["agent_flags"], case["env_flags"])
    nxt = np.concatenate([case["values"][1:], case["last_values"][None]])
    nv = np.zeros((K, E, N), F32)
    nv[cont] = nxt[cont]
    nv[cut] = case["final_values"][cut]
    r = np.zeros((K, E, N), F32)
    v = np.zeros((K, E, N), F32)
    r[live] = case["reward"][live].astype(F32)
    v[live] = case["values"][live]
    td = ((r + F32(gamma) * nv) - v) + F32(0.0)
    td[~live] = 0.0
    np.testing.assert_array_equal(bits32(adv), bits32(td))
    np.testing.assert_array_equal(bits32(ret[live]), bits32((td + v)[live]))


def test_gamma_lam_one_and_zero_values_give_rewards_to_go():
    """An f32 left fold over the rewards of an episode in reverse step order: (1e16, 1, -1e16) patterns show any other order."""
    K, E, N = 40, 15, 2
    case = make_gae_case(K, E, N, 7, False)
    zeros = np.zeros((K, E, N), F32)
    adv, ret, valid = gae_spec(case["reward"], case["agent_flags"], case["env_flags"], zeros, zeros[0], None, gamma=1.0, lam=1.0)
    live, term, cut, cont = step_classes(case["agent_flags"], case["env_flags"])
    want = np.zeros((K, E, N), F32)
    for e in range(E):
        for a in range(N):
            acc = F32(0.0)
            for s in range(K - 1, -1, -1):
                if not live[s, e, a]:
                    acc = F32(0.0)
                    continue
                if not cont[s, e, a]:
                    acc = F32(0.0)                                 # the last step of its episode
                acc = F32(F32(case["reward"][s, e, a]) + acc)
                want[s, e, a] = acc
    # (delta = (r + 1 * 0) - 0 turns a reward of -0.0 into +0.0; so does the fold's r + (+0.0))
    np.testing.assert_array_equal(bits32(adv), bits32(want))
    np.testing.assert_array_equal(bits32(ret), bits32(want))
    assert (np.abs(want) >= 1e15).any() and ((np.abs(want) > 0) & (np.abs(want) < 10)).any()


def test_an_episode_boundary_stops_the_carry():
    K, E, N = 33, 14, 3
    case = make_gae_case(K, E, N, 9, True)
    base = gae_spec(*_args(case))
    live, term, cut, cont = step_classes(case["agent_flags"], case["env_flags"])
    ends = term | cut
    first_end = np.where(ends.any(0), ends.argmax(0), K)                 # first boundary of every column ([E, N]); K: none
    behind = np.arange(K)[:, None, None] > first_end[None]              # the steps behind it
    moved = case["reward"].copy()
    moved[behind & live] += 1000.0
    assert (behind & live).sum() > 100
    other = gae_spec(moved, *_args(case)[1:])
    for b, o in zip(base, other):
        np.testing.assert_array_equal(bits32(b)[~behind], bits32(o)[~behind])
    # (the change is not a no-op: it shows wherever a column's rewards are not the 1e16 patterns, which absorb + 1000 in f32)
    assert (bits32(base[0])[behind & live] != bits32(other[0])[behind & live]).mean() > 0.5
    # the same change inside an episode does travel backwards: a step that continues sees the reward of the step behind it
    # (in a column of ordinary magnitudes, where + 1000 is not absorbed)
    ordinary = ((np.arange(E)[:, None] * N + np.arange(N)[None, :]) % 4 == 3)[None]
    s, e, a = (int(x[0]) for x in np.nonzero(cont[:-1] & live[1:] & ordinary))
    inside = case["reward"].copy()
    inside[s + 1, e, a] += 1000.0
    assert bits32(gae_spec(inside, *_args(case)[1:])[0])[s, e, a] != bits32(base[0])[s, e, a]
