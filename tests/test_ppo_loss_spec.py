"""The NumPy spec of CCX_PPO_LOSS (tests/_ppo_loss_spec.py) against itself and against f64, on the CPU: the vectorised rule
equals the header's text row by row, the tree equals an explicit loop, rows that do not count reach no output bit, the
n == 0 and n == 1 cases, the identities on the logits an action was sampled from, exp_spec on [-80, 80], and the measured
accuracy against the textbook composition in torch f64 (the bounds the header quotes are these maxima doubled)."""

import numpy as np
import pytest
from _ppo_loss_spec import (EXCLUDED_CAP, EXP_REL_BOUND_80, MOMENTS_MEAN_BOUND, MOMENTS_STD_BOUND, PPO_GRAD_LOGITS_BOUND, PPO_GRAD_LOGITS_NEAR_BOUND,
                            PPO_GRAD_VALUES_BOUND, PPO_STAT_BOUNDS, case_args, clean_case, counted, make_ppo_case,
                            masked_moments_spec, ppo_loss_backward_spec, ppo_loss_scalar, ppo_loss_spec, row_terms, tree_sum,
                            tree_sum_loop)
from _sample_spec import bits32, exp_spec, make_sample_case, sample_spec

HYPER = dict(clip=0.2, vf_coef=0.5, ent_coef=0.01, adv_eps=1e-8)
NORM = np.array([0.125, 0.75], np.float32)


def _bits64(x):
    return np.asarray(x, np.float64).view(np.uint64)


# ------------------------------------------------------------------------------------------------- the rule against its text
@pytest.mark.parametrize("density", (0.0, 0.02, 0.7, 1.0))
def test_vectorised_spec_equals_the_scalar_form(density):
    M = 700                                                              # three blocks, the last one of 188 rows
    case = make_ppo_case(M, seed=3, density=density)
    for masked, with_valid, norm, gloss in ((True, True, NORM, None), (False, True, None, -0.5), (True, False, None, 3.0)):
        kw = case_args(case, masked) if with_valid else clean_case(case, masked)
        stats = ppo_loss_spec(**kw, norm=norm, **HYPER)
        gl, gv = ppo_loss_backward_spec(**kw, norm=norm, **HYPER, stats=stats, grad_loss=gloss)
        s_stats, s_gl, s_gv = ppo_loss_scalar(**kw, norm=norm, **HYPER, grad_loss=gloss)
        np.testing.assert_array_equal(bits32(stats), bits32(s_stats))
        np.testing.assert_array_equal(bits32(gl), bits32(s_gl))
        np.testing.assert_array_equal(bits32(gv), bits32(s_gv))
        n = int(counted(kw["actions"], kw["valid"]).sum())
        assert stats[6] == n and bits32(stats)[7] == 0
        if n == 0:
            assert not bits32(stats).any() and not bits32(gl).any() and not bits32(gv).any()


@pytest.mark.parametrize("M", (1, 64, 65, 256, 257, 1023, 16389))
def test_tree_equals_an_explicit_loop(M):
    rng = np.random.default_rng(M)
    terms = rng.standard_normal(M) * np.exp(rng.uniform(-30, 30, M))
    assert _bits64(tree_sum(terms)) == _bits64(tree_sum_loop(terms))
    if M > 256:                                                          # the order matters: this is not numpy's sum
        assert any(_bits64(tree_sum(rng.permutation(terms))) != _bits64(tree_sum(terms)) for _ in range(4))
    ints = rng.integers(0, 2, M).astype(np.float64)
    assert tree_sum(ints) == ints.sum()


def test_case_generator_covers_what_it_promises():
    case = make_ppo_case(4000, seed=11, density=0.7)
    kw = case_args(case, True)
    t = row_terms(**kw, norm=None, clip=0.2, adv_eps=1e-8)
    c = t["counts"]
    a = kw["actions"]
    assert (a == 255).any() and ((a > 4) & (a < 255)).any() and np.isneginf(t["logp"][c]).any()
    assert (t["x"][c] == 0).any() and t["clipped"][c].any() and (~t["clipped"][c]).any()
    assert (t["ratio"][c] < 0.8).any() and (t["ratio"][c] > 1.2).any() and (t["x"][c] > 80).any() and (t["x"][c] < -80).any()
    assert (kw["advantages"][c] > 0).any() and (kw["advantages"][c] < 0).any()
    assert np.isnan(kw["logits"][c]).any() and np.isnan(kw["logits"][~c]).any()          # illegal places; rows that do not count
    for name in ("logp_old", "advantages", "returns", "values"):
        assert np.isnan(kw[name][~c]).any() and np.isfinite(kw[name][c]).all()
    assert np.isfinite(t["ratio"][c]).all() and (t["xc"][c & np.isneginf(t["logp"])] == -80).all()


# ------------------------------------------------------------------------------------------------- rows that do not count
def test_rows_that_do_not_count_reach_no_output_bit():
    M = 900
    case = make_ppo_case(M, seed=7, density=0.6)
    kw = case_args(case, True)
    c = counted(kw["actions"], kw["valid"])
    stats = ppo_loss_spec(**kw, norm=NORM, **HYPER)
    gl, gv = ppo_loss_backward_spec(**kw, norm=NORM, **HYPER, stats=stats, grad_loss=2.0)
    assert not bits32(gl)[~c].any() and not bits32(gv)[~c].any()         # exactly +0.0f
    rng = np.random.default_rng(1)
    for name in ("logits", "values", "logp_old", "advantages", "returns", "masks"):
        other = dict(kw)
        a = kw[name].copy()
        if a.dtype == np.uint8:
            a[~c] = rng.integers(0, 256, size=int((~c).sum()))
        else:
            junk = rng.choice(np.array([np.nan, np.inf, -np.inf, 1e30, -3.5, 0.0], np.float32), size=a.shape)
            a[~c] = junk[~c]
        other[name] = a
        s2 = ppo_loss_spec(**other, norm=NORM, **HYPER)
        g2 = ppo_loss_backward_spec(**other, norm=NORM, **HYPER, stats=s2, grad_loss=2.0)
        np.testing.assert_array_equal(bits32(s2), bits32(stats), err_msg=name)
        np.testing.assert_array_equal(bits32(g2[0]), bits32(gl), err_msg=name)
        np.testing.assert_array_equal(bits32(g2[1]), bits32(gv), err_msg=name)
    # a NaN incoming gradient reaches the rows that count and no other
    gl3, gv3 = ppo_loss_backward_spec(**kw, norm=NORM, **HYPER, stats=stats, grad_loss=np.nan)
    assert not bits32(gl3)[~c].any() and not bits32(gv3)[~c].any() and np.isnan(gv3[c]).all()
    x = kw["advantages"].copy()
    m = masked_moments_spec(x, kw["valid"])
    x[kw["valid"] == 0] = -np.inf
    np.testing.assert_array_equal(bits32(masked_moments_spec(x, kw["valid"])), bits32(m))


def test_no_row_and_one_row():
    M = 300
    case = make_ppo_case(M, seed=9, density=1.0)
    kw = case_args(case, True)
    kw["valid"] = np.zeros(M, np.uint8)
    stats = ppo_loss_spec(**kw, norm=None, **HYPER)
    assert not bits32(stats).any()
    gl, gv = ppo_loss_backward_spec(**kw, norm=None, **HYPER, stats=stats, grad_loss=np.nan)
    assert not bits32(gl).any() and not bits32(gv).any()
    np.testing.assert_array_equal(bits32(masked_moments_spec(kw["advantages"], kw["valid"])),
                                  bits32(np.array([0, 0, 1, 0], np.float32)))
    i = int(np.flatnonzero((kw["actions"] < 5) & np.isfinite(kw["logp_old"]))[5])
    kw["valid"][i] = 1
    stats = ppo_loss_spec(**kw, norm=None, **HYPER)
    t = row_terms(**kw, norm=None, clip=0.2, adv_eps=1e-8)
    assert stats[6] == 1 and stats[1] == -t["surr"][i] and stats[2] == t["vl"][i] and stats[3] == t["H"][i] and stats[4] == t["kl"][i]
    gl, gv = ppo_loss_backward_spec(**kw, norm=None, **HYPER, stats=stats)
    assert not bits32(np.delete(gl, i, 0)).any() and not bits32(np.delete(gv, i)).any()
    assert gv[i] == np.float32(0.5) * (t["ve"][i] + t["ve"][i])
    np.testing.assert_array_equal(bits32(masked_moments_spec(kw["advantages"], kw["valid"])),
                                  bits32(np.array([1, 0, 1, 0], np.float32)))


# ------------------------------------------------------------------------------------------------- on the sampler's own logits
def test_on_the_logits_the_actions_were_sampled_from():
    E, N = 96, 8
    c = make_sample_case(E, N, seed=13)
    M = E * N
    rng = np.random.default_rng(2)
    adv, ret, val = (rng.standard_normal(M).astype(np.float32) for _ in range(3))
    for masked in (True, False):
        logits, masks = (c["logits_masked"], c["masks"]) if masked else (c["logits"], None)
        actions, logp, _ = sample_spec(logits, masks, c["terminated"], c["truncated"], c["step_count"], c["episode"], seed=99)
        kw = dict(logits=logits.reshape(M, 5), values=val, actions=actions.reshape(M), logp_old=logp.reshape(M), advantages=adv,
                  returns=ret, masks=None if masks is None else masks.reshape(M), valid=None)
        norm = masked_moments_spec(adv, (actions.reshape(M) != 255).astype(np.uint8))[1:3]
        stats, t, _ = ppo_loss_spec(**kw, norm=norm, **HYPER, details=True)
        cnt = t["counts"]
        assert cnt.any() and not cnt.all()
        assert (bits32(t["x"][cnt]) == 0).all() and (t["ratio"][cnt] == 1).all()
        assert bits32(stats)[4] == 0 and bits32(stats)[5] == 0            # approx_kl = clip_frac = +0.0f
        mean_an = tree_sum(np.where(cnt, t["an"].astype(np.float64), 0.0)) / cnt.sum()
        assert stats[1] == np.float32(-mean_an)                          # policy == -mean(an)


# ------------------------------------------------------------------------------------------------- against f64
def test_exp_spec_on_minus_80_to_80():
    rng = np.random.default_rng(0)
    xs = np.concatenate([rng.uniform(-80, 80, 2_000_000), np.linspace(-80, 80, 500_001), [-80.0, 80.0, 0.0, -0.0]]).astype(np.float32)
    n = np.rint(xs * np.float32(1.4426950408889634))
    assert np.abs(n).max() <= 115                                        # n * 0x1.62e4p-1f (15 significant bits) stays exact
    e = exp_spec(xs)
    ref = np.exp(xs.astype(np.float64))
    rel = np.abs(e.astype(np.float64) - ref) / ref
    print(f"exp_spec on [-80, 80]: max rel err {rel.max():.3e} (negative half {rel[xs <= 0].max():.3e}, positive half {rel[xs >= 0].max():.3e})")
    assert rel.max() <= EXP_REL_BOUND_80
    assert np.isfinite(e).all() and (e >= np.float32(2.0) ** -126).all() and exp_spec(np.float32(0.0)) == 1 and exp_spec(np.float32(-0.0)) == 1


def _torch_f64(kw, norm, hyper, select):
    """The textbook composition in torch f64 on the same f32 inputs, over the rows of `select`: stats (5) and the two
    gradients of the loss."""
    import torch

    M = len(kw["actions"])
    lo, hi = float(np.float32(1) - np.float32(hyper["clip"])), float(np.float32(1) + np.float32(hyper["clip"]))
    vf, ent, eps = (float(np.float32(hyper[k])) for k in ("vf_coef", "ent_coef", "adv_eps"))
    x = torch.from_numpy(np.nan_to_num(kw["logits"][select], nan=0.0).astype(np.float64)).requires_grad_(True)
    v = torch.from_numpy(kw["values"][select].astype(np.float64)).requires_grad_(True)
    m = np.full(M, 0x1F, np.uint8) if kw["masks"] is None else kw["masks"]
    legal = torch.from_numpy(((((m[select] & 0x1F) | 0x10)[:, None] >> np.arange(5, dtype=np.uint8)) & 1).astype(bool))
    a = torch.from_numpy(kw["actions"][select].astype(np.int64))
    lpo, adv, ret = (torch.from_numpy(kw[k][select].astype(np.float64)) for k in ("logp_old", "advantages", "returns"))
    lp = torch.log_softmax(x.masked_fill(~legal, -torch.inf), -1)
    p = lp.exp()
    zero = torch.zeros_like(lp)
    H = -torch.where(p > 0, p * torch.where(p > 0, lp, zero), zero).sum(-1)
    logp = lp.gather(-1, a[:, None])[:, 0]
    logr = logp - lpo
    ratio = logr.exp()
    an = adv if norm is None else (adv - float(norm[0])) / (float(norm[1]) + eps)
    surr = torch.minimum(ratio * an, ratio.clamp(lo, hi) * an)
    policy, value, entropy = -surr.mean(), ((v - ret) ** 2).mean(), H.mean()
    loss = policy + vf * value - ent * entropy
    kl = ((ratio - 1) - logr).mean()
    gx, gvv = torch.autograd.grad(loss, (x, v))
    return (np.array([loss.item(), policy.item(), value.item(), entropy.item(), kl.item()]), gx.numpy(), gvv.numpy())


def test_accuracy_against_the_f64_composition():
    M = 16389
    worst = dict.fromkeys(("loss", "policy", "value", "entropy", "approx_kl", "grad_logits", "grad_logits_near", "grad_values"), 0.0)
    share = 0.0
    for seed, masked, norm_on in ((41, True, True), (42, False, True), (43, True, False)):
        case = make_ppo_case(M, seed=seed, density=0.8)
        kw = case_args(case, masked)
        norm = masked_moments_spec(kw["advantages"], kw["valid"])[1:3] if norm_on else None
        t = row_terms(**kw, norm=norm, clip=0.2, adv_eps=1e-8)
        c = t["counts"]
        # rows where the two sides legitimately differ: ratio within one ulp of lo / hi, s1 == s2 outside the range,
        # |x| > 80, logp = -inf; and the rows CCX_SAMPLE calls degenerate, which f64 softmax has no answer for
        lo, hi = np.float32(1) - np.float32(0.2), np.float32(1) + np.float32(0.2)
        near = (np.abs(t["ratio"] - lo) <= np.spacing(lo)) | (np.abs(t["ratio"] - hi) <= np.spacing(hi))
        lg = np.where(_legal(kw), kw["logits"], -np.inf)
        degenerate = np.isnan(lg).any(-1) | (lg == np.inf).any(-1) | (lg.max(-1) == -np.inf)
        with np.errstate(invalid="ignore"):
            out = near | (t["clipped"] & (t["s1"] == t["s2"])) | (np.abs(t["x"]) > 80) | np.isneginf(t["logp"]) | degenerate
        excluded = c & out
        frac = excluded.sum() / c.sum()
        share = max(share, frac)
        assert frac <= EXCLUDED_CAP, f"{frac:.3f} of the counted rows are left out"
        select = c & ~out
        kw2 = dict(kw, valid=select.astype(np.uint8))
        stats = ppo_loss_spec(**kw2, norm=norm, **HYPER)
        gl, gv = ppo_loss_backward_spec(**kw2, norm=norm, **HYPER, stats=stats)
        f_stats, f_gl, f_gv = _torch_f64(kw2, norm, HYPER, select)
        n = float(stats[6])
        assert n == select.sum()
        for k, name in enumerate(("loss", "policy", "value", "entropy", "approx_kl")):
            worst[name] = max(worst[name], abs(float(stats[k]) - f_stats[k]) / max(1.0, abs(f_stats[k])))
        for name, ours, ref in (("grad_logits", gl[select], f_gl), ("grad_values", gv[select], f_gv)):
            ours, ref = ours.astype(np.float64) * n, ref * n
            err = np.abs(ours - ref) / np.maximum(1.0, np.abs(ref))
            worst[name] = max(worst[name], float(err.max()))
            if name == "grad_logits":                                    # rows whose stored action is not far down the tail
                worst["grad_logits_near"] = max(worst["grad_logits_near"], float(err[t["logp"][select] >= -10].max()))
    print("against torch f64, max |err| / max(1, |f64|):", {k: f"{v:.3e}" for k, v in worst.items()},
          f"largest share of counted rows left out {share:.3f}")
    for name, bound in PPO_STAT_BOUNDS.items():
        assert worst[name] <= bound, name
    assert worst["grad_logits"] <= PPO_GRAD_LOGITS_BOUND and worst["grad_values"] <= PPO_GRAD_VALUES_BOUND
    assert worst["grad_logits_near"] <= PPO_GRAD_LOGITS_NEAR_BOUND


def _legal(kw):
    M = len(kw["actions"])
    m = np.full(M, 0x1F, np.uint8) if kw["masks"] is None else kw["masks"]
    return ((((m & 0x1F) | 0x10)[:, None] >> np.arange(5, dtype=np.uint8)) & 1).astype(bool)


def test_moments_against_f64():
    import torch

    rng = np.random.default_rng(4)
    worst = [0.0, 0.0]
    for M, scale, shift in ((16389, 1.0, 0.0), (5000, 0.01, 3.0), (777, 50.0, -20.0), (2, 1.0, 0.0)):
        x = (rng.standard_normal(M) * scale + shift).astype(np.float32)
        valid = (rng.random(M) < 0.7).astype(np.uint8)
        valid[:2] = 1
        out = masked_moments_spec(x, valid)
        sel = torch.from_numpy(x.astype(np.float64))[torch.from_numpy(valid != 0)]
        mean, std = sel.mean().item(), sel.std().item()                  # torch.std: unbiased
        assert out[0] == sel.numel()
        worst[0] = max(worst[0], abs(float(out[1]) - mean) / max(1.0, abs(mean)))
        worst[1] = max(worst[1], abs(float(out[2]) - std) / max(1.0, abs(std)))
    print(f"moments against torch f64: mean {worst[0]:.3e}, std {worst[1]:.3e}")
    assert worst[0] <= MOMENTS_MEAN_BOUND and worst[1] <= MOMENTS_STD_BOUND
