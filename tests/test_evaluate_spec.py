"""The NumPy restatement of CCX_EVALUATE (tests/_evaluate_spec.py) checked on the CPU: vector against scalar form, the
sampler's own logp / entropy bits on the rows that store the sampler's action, the identities the rule leans on, and the
accuracy of the forward and of the two Jacobians against f64.  No GPU."""

import numpy as np
import pytest
from _evaluate_spec import (EVAL_ENTROPY_BOUND, EVAL_JAC_ENTROPY_BOUND, EVAL_JAC_LOGP_BOUND, EVAL_LOGP_BOUND, _steps_2_to_6,
                            case_args, evaluate_backward_scalar, evaluate_backward_spec, evaluate_scalar, evaluate_spec,
                            make_evaluate_case)
from _sample_spec import F32, bits32, make_sample_case, reference_f64, sample_spec

GRADS = ((True, True), (True, False), (False, True))


@pytest.fixture(scope="module")
def big_case():
    return make_evaluate_case(2048, 8, seed=7)


# ------------------------------------------------------------------------------------------------- vector against scalar
@pytest.mark.parametrize("masked", (True, False))
def test_vector_spec_equals_the_scalar_pseudo_code(masked):
    case = make_evaluate_case(41, 8, seed=1)
    logits, actions, masks, glp, gent = case_args(case, masked)
    vec, sca = evaluate_spec(logits, actions, masks), evaluate_scalar(logits, actions, masks)
    for v, s, name in zip(vec, sca, ("logp", "entropy")):
        np.testing.assert_array_equal(bits32(v), bits32(s), err_msg=name)
    assert evaluate_spec(logits, actions, masks, want_entropy=False)[1] is None
    for with_lp, with_ent in GRADS:
        a, b = glp if with_lp else None, gent if with_ent else None
        np.testing.assert_array_equal(bits32(evaluate_backward_spec(logits, actions, masks, a, b)),
                                      bits32(evaluate_backward_scalar(logits, actions, masks, a, b)), err_msg=f"{with_lp} {with_ent}")
    assert len(np.unique(case["classes"])) == 10                      # every slot class of the generator occurs


# ------------------------------------------------------------------------------------------------- the sampler's bits
@pytest.mark.parametrize("masked", (True, False))
def test_rows_that_store_the_samplers_action_get_the_samplers_bits(big_case, masked):
    tag = "" if masked else "_nomask"
    logits, actions, masks, _, _ = case_args(big_case, masked)
    logp, entropy = evaluate_spec(logits, actions, masks)
    acts, lp, ent = big_case["spec" + tag]
    same = actions == acts                                              # the sampled share, the dead slots, chance hits
    assert big_case["sampled" + tag].sum() > 0.5 * big_case["M"] and same[big_case["sampled" + tag]].all()
    np.testing.assert_array_equal(bits32(logp)[same], bits32(lp)[same])
    np.testing.assert_array_equal(bits32(entropy)[same], bits32(ent)[same])
    live = actions != 255
    np.testing.assert_array_equal(bits32(entropy)[live], bits32(ent)[live])     # the entropy does not depend on the action


def test_deterministic_actions_get_the_samplers_bits():
    E, N = 256, 8
    c = make_sample_case(E, N, seed=3)
    for masked in (True, False):
        lg, mk = (c["logits_masked"], c["masks"]) if masked else (c["logits"], None)
        acts, lp, ent = sample_spec(lg, mk, c["terminated"], c["truncated"], c["step_count"], c["episode"], deterministic=True)
        logp, entropy = evaluate_spec(lg.reshape(-1, 5), acts.reshape(-1), None if mk is None else mk.reshape(-1))
        np.testing.assert_array_equal(bits32(logp), bits32(lp.reshape(-1)))
        np.testing.assert_array_equal(bits32(entropy), bits32(ent.reshape(-1)))
        assert (acts == 255).any()


# ------------------------------------------------------------------------------------------------- identities
@pytest.mark.parametrize("masked", (True, False))
def test_identities_of_a_batch(big_case, masked):
    logits, actions, masks, glp, gent = case_args(big_case, masked)
    s = _steps_2_to_6(logits, masks)
    legal, deg = s["legal"], s["degenerate"]
    logp, entropy = evaluate_spec(logits, actions, masks)
    absent = actions == 255
    a_ok = (actions <= 4) & np.take_along_axis(legal, np.minimum(actions, 4).astype(np.int64)[:, None], -1)[:, 0]
    junk = ~absent & ~a_ok
    assert absent.any() and deg.any() and (actions[junk] > 4).any() and (not masked or (actions[junk] <= 4).any())
    # absent rows: +0.0 everywhere; out-of-range or illegal actions: logp = -inf
    assert not bits32(logp)[absent].any() and not bits32(entropy)[absent].any()
    assert np.isneginf(logp[junk]).all() and not np.isnan(logp).any() and not np.isnan(entropy).any()
    # NaN sits in the logits of absent rows and (masked) of illegal places, NaN / inf in the gradients the rule selects away
    assert np.isnan(logits[absent]).any() and (not masked or np.isnan(logits[~absent][~legal[~absent]]).all())
    assert not np.isfinite(glp[absent | junk]).all() and not np.isfinite(gent[absent]).all()
    assert np.isfinite(glp[a_ok]).all() and np.isfinite(gent[~absent]).all()
    single = ~absent & (legal.sum(-1) == 1)
    for with_lp, with_ent in GRADS:
        g = evaluate_backward_spec(logits, actions, masks, glp if with_lp else None, gent if with_ent else None)
        assert np.isfinite(g).all()
        assert not bits32(g)[absent | deg].any()                        # exactly +0.0
        assert not bits32(g)[~legal].any()
        if masked:
            assert single.any() and not (bits32(g)[single] & 0x7FFFFFFF).any()      # one legal action: +-0
    if masked:
        assert not bits32(logp)[single & a_ok].any() and not bits32(entropy)[single].any()
    # no logp term where the action is out of range or illegal: grad_logp does not matter there
    both = evaluate_backward_spec(logits, actions, masks, glp, gent)
    only = evaluate_backward_spec(logits, actions, masks, None, gent)
    plain = junk & ~deg
    assert plain.any()
    np.testing.assert_array_equal(both[plain], F32(0.0) - (F32(0.0) - only[plain]))      # A = +0: A - B against 0 - B, up to the sign of zero
    assert not bits32(evaluate_backward_spec(logits, actions, masks, glp, None))[junk].any()


# ------------------------------------------------------------------------------------------------- accuracy
def _torch_jacobians(logits, masks, actions):
    """f64 autograd on the CPU: d logp_a / d logits and d entropy / d logits of the masked log-softmax, [M, 5] each."""
    import torch

    m = np.full(len(logits), 0x1F, np.uint8) if masks is None else masks
    legal = torch.from_numpy((((m[:, None] | 0x10) >> np.arange(5, dtype=np.uint8)) & 1).astype(bool))
    x = torch.from_numpy(logits.astype(np.float64)).requires_grad_(True)
    lp = torch.log_softmax(x.masked_fill(~legal, -np.inf), -1)
    p = lp.exp()
    ent = -torch.where(p > 0, p * torch.where(p > 0, lp, torch.zeros_like(lp)), torch.zeros_like(lp)).sum(-1)
    lpa = lp.gather(-1, torch.from_numpy(actions.astype(np.int64))[:, None])[:, 0]
    j_lp, = torch.autograd.grad(lpa.sum(), x, retain_graph=True)
    j_ent, = torch.autograd.grad(ent.sum(), x)
    return lpa.detach().numpy(), ent.detach().numpy(), j_lp.numpy(), j_ent.numpy()


def test_accuracy_against_f64(big_case):
    worst = {"logp": 0.0, "entropy": 0.0, "jac_logp": 0.0, "jac_entropy": 0.0}
    for masked in (True, False):
        logits, actions, masks, _, _ = case_args(big_case, masked)
        s = _steps_2_to_6(logits, masks)
        a = np.minimum(actions, 4).astype(np.int64)
        a_ok = (actions <= 4) & np.take_along_axis(s["legal"], a[:, None], -1)[:, 0]
        covered = (actions != 255) & ~s["degenerate"] & a_ok & (np.take_along_axis(s["w"], a[:, None], -1)[:, 0] > 0)
        share = covered.mean()
        print(f"masked {masked}: covered rows {covered.sum()} of {len(covered)} ({share:.3f})")
        assert share >= 0.5
        lg, ac, mk = logits[covered], actions[covered], None if masks is None else masks[covered]
        logp, entropy = evaluate_spec(lg, ac, mk)
        ones = np.ones(len(lg), F32)
        jac_lp = evaluate_backward_spec(lg, ac, mk, ones, None)
        jac_ent = evaluate_backward_spec(lg, ac, mk, None, ones)
        # the forward against reference_f64, the Jacobians against torch f64 autograd of the masked log-softmax and entropy
        ref_lp, ref_ent = reference_f64(lg[:, None, :], None if mk is None else mk[:, None])
        ref_lpa = np.take_along_axis(ref_lp[:, 0], ac.astype(np.int64)[:, None], -1)[:, 0]
        t_lpa, t_ent, t_jlp, t_jent = _torch_jacobians(np.where(np.isnan(lg), 0.0, lg).astype(F32), mk, ac)
        np.testing.assert_allclose(t_lpa, ref_lpa, rtol=0, atol=1e-12)               # the two f64 references agree
        np.testing.assert_allclose(t_ent, ref_ent[:, 0], rtol=0, atol=1e-12)
        for name, got, ref in (("logp", logp, ref_lpa), ("entropy", entropy, ref_ent[:, 0]), ("jac_logp", jac_lp, t_jlp),
                               ("jac_entropy", jac_ent, t_jent)):
            err = np.abs(got.astype(np.float64) - ref) / np.maximum(1.0, np.abs(ref))
            assert np.isfinite(err).all(), name
            worst[name] = max(worst[name], float(err.max()))
    print("measured maxima against f64:", worst)
    bounds = {"logp": EVAL_LOGP_BOUND, "entropy": EVAL_ENTROPY_BOUND, "jac_logp": EVAL_JAC_LOGP_BOUND, "jac_entropy": EVAL_JAC_ENTROPY_BOUND}
    for name, bound in bounds.items():
        assert worst[name] <= bound, (name, worst[name], bound)
        assert bound <= 2.1 * worst[name], (name, worst[name], bound)      # the measured maximum doubled, not something looser
