"""The NumPy restatement of CCX_SAMPLE (tests/_sample_spec.py) checked on the CPU: vector against scalar form, the key
against the oracle's CCX_POLICY_RANDOM, the identities the rule leans on, accuracy against f64, the distribution of the
sampled actions, and the deterministic mode.  No GPU."""

import math

import numpy as np
import pytest
from _fixtures import Golden
from _sample_spec import (D_MIN, ENTROPY_ABS_BOUND, EXP_REL_BOUND, F32, K_EPS_STREAM, K_SAMPLE_STREAM, LOGP_ABS_BOUND, bits32,
                          exp_spec, log_spec, make_sample_case, random_word, reference_f64, sample_scalar, sample_spec)

SEED = 0x1234_5678_9ABC_DEF0
FAR_OFFSET = (1 << 32) - 11              # global env indices that cross 2^32 inside the batch


def _args(case, masked: bool):
    return (case["logits_masked"] if masked else case["logits"], case["masks"] if masked else None, case["terminated"],
            case["truncated"], case["step_count"], case["episode"])


@pytest.fixture(scope="module")
def big_case():
    case = make_sample_case(4096, 8, seed=7)
    runs = {masked: sample_spec(*_args(case, masked), env_offset=FAR_OFFSET, seed=SEED, details=True) for masked in (True, False)}
    return case, runs


# ------------------------------------------------------------------------------------------------- vector against scalar
@pytest.mark.parametrize("masked", (True, False))
@pytest.mark.parametrize("deterministic", (False, True))
def test_vector_spec_equals_the_scalar_pseudo_code(masked, deterministic):
    case = make_sample_case(41, 8, seed=1)
    kw = dict(env_offset=FAR_OFFSET, seed=SEED, deterministic=deterministic)
    vec = sample_spec(*_args(case, masked), **kw)
    sca = sample_scalar(*_args(case, masked), **kw)
    for v, s, name in zip(vec, sca, ("actions", "logp", "entropy")):
        np.testing.assert_array_equal(bits32(v), bits32(s), err_msg=name)
    assert len(np.unique(case["classes"])) == 10                      # every slot class of the generator occurs


# ------------------------------------------------------------------------------------------------- the key
def test_stream_zero_reproduces_the_oracles_random_policy():
    """random_word with stream constant 0 is the word of CCX_POLICY_RANDOM: action = word * 5 >> 32, pinned by the oracle."""
    from oracle import oracle

    from collectivecrossing_amd.params import lower_config

    params = lower_config(Golden("g8_rollout_c1").config)
    E, N, K, offset, seed = 6, params.num_agents, 12, (1 << 32) - 3, 0xDEAD_BEEF_0000_0042
    ob = oracle.OracleBatch(params, E, offset, offset + E)
    pool = oracle.seeded_placements(params, np.arange(5, 5 + 16, dtype=np.uint64))
    ob.set_reset_pool(pool)
    ob.set_state(episode=np.arange(E) * 1000 + 3)
    ob.reset_from_pool()
    oracle.OracleBatch.set_rng_seed(seed)
    try:
        compared = 0
        for _ in range(K):
            g = offset + np.arange(E, dtype=np.int64)[:, None]
            j, t = ob.episode.copy()[:, None], ob.step_count.copy()[:, None]
            alive = (ob.terminated == 0) & (ob.truncated == 0)
            acts = ob.rollout_greedy(1, policy="random", want_obs=False)[0][0]
            word = random_word(seed, 0, g, j, t, np.arange(N)[None, :])
            mine = ((word.astype(np.uint64) * np.uint64(5)) >> np.uint64(32)).astype(np.uint8)
            np.testing.assert_array_equal(acts[alive], mine[alive])
            assert (acts[~alive] == 255).all()
            compared += int(alive.sum())
        assert compared > E * N * 3
    finally:
        oracle.OracleBatch.set_rng_seed(0)
    assert K_SAMPLE_STREAM not in (0, K_EPS_STREAM)
    other = random_word(seed, K_SAMPLE_STREAM, g, j, t, np.arange(N)[None, :])
    assert (other != word).mean() > 0.99


# ------------------------------------------------------------------------------------------------- identities
def test_the_two_exact_identities():
    assert bits32(np.array([exp_spec(F32(0.0))], F32))[0] == bits32(np.array([1.0], F32))[0]
    assert bits32(np.array([log_spec(F32(1.0))], F32))[0] == 0          # +0.0
    assert bits32(exp_spec(np.zeros(3, F32))).tolist() == [0x3F800000] * 3
    assert not bits32(log_spec(np.ones(3, F32))).any()


@pytest.mark.parametrize("masked", (True, False))
def test_identities_of_a_batch(big_case, masked):
    case, runs = big_case
    actions, logp, entropy, d = runs[masked]
    live = ~d["dead"]
    w, S, legal = d["w"], d["S"], d["legal"]
    tiny = np.finfo(F32).tiny
    assert ((w == 0) | (w >= tiny)).all() and (w <= 1).all()            # never subnormal, never above the maximum's 1
    assert (S[live] >= 1).all() and (S[live] <= 5).all()
    assert (w.max(-1)[live] == 1).all()
    a = np.where(live, actions, 4).astype(np.int64)[..., None]
    assert np.take_along_axis(legal, a, -1)[..., 0][live].all()         # the action is legal ...
    assert (np.take_along_axis(w, a, -1)[..., 0][live] > 0).all()       # ... and has weight
    assert (actions[~live] == 255).all() and not bits32(logp)[~live].any() and not bits32(entropy)[~live].any()
    # NaN sits at every place the rule does not read, and in no output
    lg = _args(case, masked)[0]
    assert np.isnan(lg[~live]).all() and (not masked or np.isnan(lg[live][~legal[live]]).all())
    assert not np.isnan(logp).any() and not np.isnan(entropy).any()
    assert (logp <= 0).all() and (entropy >= 0).all()
    single = live & (legal.sum(-1) == 1)
    assert (not masked) or (single.any() and not bits32(logp)[single].any() and not bits32(entropy)[single].any())
    assert d["degenerate"][live].any() and (actions[live] < 5).all()


# ------------------------------------------------------------------------------------------------- accuracy
def _exp_points():
    x = [np.linspace(-80.0, 0.0, (1 << 22) + 1).astype(F32)]
    near = []
    for n in range(-116, 1):                                            # where n changes, and where r is largest
        for h in (n * math.log(2.0), (n + 0.5) * math.log(2.0)):
            lo = hi = F32(h)
            for _ in range(4):
                near += [lo, hi]
                lo, hi = np.nextafter(lo, F32(-np.inf)), np.nextafter(hi, F32(np.inf))
    pow2 = -np.ldexp(1.0, np.arange(-149, 7)).astype(F32)
    pow2 = np.concatenate([pow2, np.nextafter(pow2, F32(0.0)), np.nextafter(pow2, F32(-np.inf))])
    edge = np.array([D_MIN, np.nextafter(D_MIN, F32(0.0)), 0.0, -0.0], F32)
    x = np.concatenate(x + [np.array(near, F32), pow2, edge])
    return x[(x >= D_MIN) & (x <= 0)]


def test_accuracy_against_f64(big_case):
    x = _exp_points()
    assert len(x) >= 1 << 22
    y = exp_spec(x)
    ref = np.exp(x.astype(np.float64))
    rel = float((np.abs(y.astype(np.float64) - ref) / ref).max())
    worst = {"exp_rel": rel, "logp_abs": 0.0, "entropy_abs": 0.0}
    case, runs = big_case
    for masked in (True, False):
        actions, logp, entropy, d = runs[masked]
        ok = ~d["dead"] & ~d["degenerate"]
        assert ok.sum() > 20000
        ref_lp, ref_ent = reference_f64(*_args(case, masked)[:2])
        a = np.where(ok, actions, 4).astype(np.int64)[..., None]
        ref_a = np.take_along_axis(ref_lp, a, -1)[..., 0]
        worst["logp_abs"] = max(worst["logp_abs"], float(np.abs(logp.astype(np.float64) - ref_a)[ok].max()))
        worst["entropy_abs"] = max(worst["entropy_abs"], float(np.abs(entropy.astype(np.float64) - ref_ent)[ok].max()))
    print("measured maxima against f64:", worst)
    assert rel <= EXP_REL_BOUND and worst["logp_abs"] <= LOGP_ABS_BOUND and worst["entropy_abs"] <= ENTROPY_ABS_BOUND
    # the constants are the measured maxima doubled, not something looser
    assert EXP_REL_BOUND <= 2.1 * rel and LOGP_ABS_BOUND <= 2.1 * worst["logp_abs"]
    assert ENTROPY_ABS_BOUND <= 2.1 * worst["entropy_abs"]


# ------------------------------------------------------------------------------------------------- distribution
VECTORS = {
    "uniform": (np.zeros(5, F32), 0x1F),
    "peaked": (np.array([3.0, 0.0, -1.0, 0.5, 1.0], F32), 0x1F),
    "two_illegal": (np.array([0.5, 2.0, -0.5, 1.0, 0.0], F32), 0x1F & ~0x0A),       # actions 1 and 3 ruled out
}


def _chi_square_limit(dof: int) -> float:
    """The x whose upper tail under chi-square with `dof` degrees of freedom equals that of 30 under 4 degrees:
    sf_4(x) = e^(-x/2) (1 + x/2), sf_2(x) = e^(-x/2)."""
    tail = math.exp(-15.0) * 16.0
    assert 4e-6 < tail < 6e-6
    return {4: 30.0, 2: -2.0 * math.log(tail)}[dof]


@pytest.mark.parametrize("seed", range(8))
@pytest.mark.parametrize("name", sorted(VECTORS))
def test_sampled_actions_follow_the_softmax(name, seed):
    vec, mask = VECTORS[name]
    E = 1 << 16                                                          # 2^16 keys: g = e, t = e >> 7 both vary
    logits = np.broadcast_to(vec, (E, 1, 5))
    masks = np.full((E, 1), mask, np.uint8)
    zeros = np.zeros((E, 1), np.uint8)
    actions, _, _ = sample_spec(logits, masks, zeros, zeros, np.arange(E) >> 7, np.full(E, 3), env_offset=1000, seed=seed)
    legal = np.array([(mask | 0x10) >> k & 1 for k in range(5)], bool)
    x = np.where(legal, vec.astype(np.float64), -np.inf)
    p = np.exp(x - x.max())
    p /= p.sum()
    counts = np.bincount(actions.ravel(), minlength=5)[:5]
    assert counts.sum() == E and not counts[~legal].any()
    chi2 = float((((counts - E * p) ** 2)[legal] / (E * p)[legal]).sum())
    assert chi2 < _chi_square_limit(int(legal.sum()) - 1), (name, seed, chi2, counts)


# ------------------------------------------------------------------------------------------------- deterministic mode
@pytest.mark.parametrize("masked", (True, False))
def test_deterministic_mode_is_the_masked_argmax(big_case, masked):
    case, runs = big_case
    actions, logp, entropy = sample_spec(*_args(case, masked), env_offset=FAR_OFFSET, seed=SEED, deterministic=True)
    _, _, sampled_entropy, d = runs[masked]
    live, legal, deg = ~d["dead"], d["legal"], d["degenerate"]
    with np.errstate(invalid="ignore"):
        lg = np.where(legal, _args(case, masked)[0], -np.inf)
    plain = live & ~deg
    want = np.nanargmax(np.where(np.isnan(lg), -np.inf, lg), -1)        # np.argmax: the lowest index on ties
    np.testing.assert_array_equal(actions[plain], want[plain])
    np.testing.assert_array_equal(actions[live & deg], legal.argmax(-1)[live & deg])     # degenerate: the lowest legal k
    assert (case["classes"][plain] == 4).any()                          # (slots with exact ties at the maximum)
    np.testing.assert_array_equal(bits32(entropy), bits32(sampled_entropy))              # the entropy does not depend on the mode
    np.testing.assert_array_equal(bits32(logp)[plain], bits32(-log_spec(d["S"]) + F32(0.0))[plain])     # d = +0 at the maximum
    other = sample_spec(*_args(case, masked), env_offset=5, seed=1, deterministic=True)
    np.testing.assert_array_equal(actions, other[0])                    # no draw: no key
