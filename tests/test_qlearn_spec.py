"""The NumPy statement of CCX_QLEARN (tests/_qlearn_spec.py) against independent statements: the textbook double-DQN Huber
loss in torch f64 with autograd (accuracy, with the bounds the header quotes), properties of the rule, and the statistics
of the exploration draws.  No GPU."""

import numpy as np
import pytest
from _qlearn_spec import (TD_GRAD_BOUND, TD_LOSS_BOUND, TD_MEAN_ABS_BOUND, TD_VARIANTS, legal_bits, make_q_case, make_td_case,
                          q_actions_spec, td_args, td_loss_backward_spec, td_loss_spec)
from _sample_spec import bits32

SEED = 0x0123_4567_89AB_CDEF
GAMMA = 0.97


@pytest.fixture(scope="module")
def case():
    return make_td_case(16389, seed=41)


def _textbook_f64(kw, gamma, delta):
    """(loss, mean |td|, n * d loss / d q) of the textbook composition in torch f64 on the same f32 inputs, over the rows
    that count; rows that do not count are replaced by zeros first (torch has no select that stops a NaN's gradient)."""
    import torch

    M = len(kw["actions"])
    a = kw["actions"].astype(np.int64)
    counts = (a <= 4) & (np.ones(M, bool) if kw["valid"] is None else kw["valid"] != 0)
    sel = torch.from_numpy(counts)

    def clean(x, fill=0.0):
        return torch.where(sel.reshape((M,) + (1,) * (x.ndim - 1)), torch.from_numpy(x).double(), torch.tensor(fill, dtype=torch.float64))

    q = clean(kw["q"]).requires_grad_()
    legal = torch.from_numpy(legal_bits(kw["masks_next"], (M,)))
    qt = clean(kw["q_next_target"])
    chooser = qt if kw["q_next_online"] is None else clean(kw["q_next_online"])
    chooser = torch.where(legal & ~torch.isnan(chooser), chooser, torch.tensor(-np.inf, dtype=torch.float64))
    kstar = chooser.argmax(-1)                                           # (the generator's ties are exact in f32 and in f64)
    boot = qt.gather(-1, kstar[:, None])[:, 0]
    done = torch.from_numpy(kw["done"] != 0)
    g = float(np.float32(gamma))
    y = clean(kw["reward"].astype(np.float32)) + torch.where(done, torch.zeros((), dtype=torch.float64), g * boot)
    qa = q.gather(-1, torch.from_numpy(np.minimum(a, 4))[:, None])[:, 0]
    d = qa - y
    h = torch.nn.functional.huber_loss(qa, y, reduction="none", delta=delta) if np.isfinite(delta) else 0.5 * d * d
    w = torch.ones(M, dtype=torch.float64) if kw["weights"] is None else clean(kw["weights"])
    n = float(counts.sum())
    loss = torch.where(sel, w * h, torch.zeros((), dtype=torch.float64)).sum() / n
    (grad,) = torch.autograd.grad(loss, q)
    mad = torch.where(sel, d.abs(), torch.zeros((), dtype=torch.float64)).sum() / n
    return float(loss.detach()), float(mad.detach()), (grad * n).numpy(), counts, kstar.numpy()


def test_against_torch_f64(case):
    worst = dict(loss=0.0, mean_abs=0.0, grad=0.0)
    for variant in TD_VARIANTS:
        for M in (1023, 16389):
            for delta in (1.0, float("inf")):
                kw = td_args(case, *variant, M=M)
                stats, td, t = td_loss_spec(**kw, gamma=GAMMA, huber_delta=delta, details=True)
                gq = td_loss_backward_spec(**kw, gamma=GAMMA, huber_delta=delta, stats=stats)
                loss, mad, grad, counts, kstar = _textbook_f64(kw, GAMMA, delta)
                assert stats[6] == counts.sum() > M // 2
                live = counts & (kw["done"] == 0)
                np.testing.assert_array_equal(t["kstar"][live], kstar[live])          # the same bootstrap action
                n = float(stats[6])
                # |d| within an ulp of huber_delta: the two sides may sit on different branches of the derivative
                near = np.abs(np.abs(td.astype(np.float64)) - delta) < 1e-6 if np.isfinite(delta) else np.zeros(M, bool)
                keep = counts & ~near
                assert near.sum() < 0.1 * counts.sum()
                err = np.abs(gq.astype(np.float64) * n - grad) / np.maximum(1.0, np.abs(grad))
                worst["loss"] = max(worst["loss"], abs(float(stats[0]) - loss) / max(1.0, abs(loss)))
                worst["mean_abs"] = max(worst["mean_abs"], abs(float(stats[1]) - mad) / max(1.0, abs(mad)))
                worst["grad"] = max(worst["grad"], float(err[keep].max()))
                assert not gq[~counts].any()
    print("measured against torch f64:", {k: f"{v:.3g}" for k, v in worst.items()})
    assert worst["loss"] <= TD_LOSS_BOUND and worst["mean_abs"] <= TD_MEAN_ABS_BOUND and worst["grad"] <= TD_GRAD_BOUND
    assert worst["loss"] > 0 and worst["grad"] > 0                       # (the comparison compared something)


def test_the_gradient_sits_at_the_taken_action_only(case):
    kw = td_args(case, True, True, True, True, M=1023)
    stats, td, t = td_loss_spec(**kw, gamma=GAMMA, details=True)
    gq = td_loss_backward_spec(**kw, gamma=GAMMA, stats=stats)
    off = np.arange(5)[None, :] != np.minimum(t["a"], 4)[:, None]
    assert not bits32(gq)[off].any() and not bits32(gq)[~t["counts"]].any()
    assert (gq[t["counts"], t["a"][t["counts"]]] != 0).mean() > 0.8
    assert not bits32(td)[~t["counts"]].any() and t["bad"].sum() == stats[7] > 0
    # |d| == delta exactly takes the quadratic branch, its upper neighbour the linear one: both gradients are +-delta * gw
    exact = t["counts"] & (t["ad"] == np.float32(1.0))
    assert exact.sum() >= 3
    np.testing.assert_array_equal(bits32(t["h"][exact]), bits32(np.full(exact.sum(), 0.5, np.float32)))


def test_huber_delta_inf_is_the_half_squared_error(case):
    kw = td_args(case, False, True, False, False, M=1023)
    stats, td, t = td_loss_spec(**kw, gamma=GAMMA, huber_delta=float("inf"), details=True)
    d = t["d"]
    np.testing.assert_array_equal(bits32(t["h"][t["counts"]]), bits32((np.float32(0.5) * (d * d).astype(np.float32))[t["counts"]]))
    gq = td_loss_backward_spec(**kw, gamma=GAMMA, huber_delta=float("inf"), stats=stats)
    sc = np.float32(np.float32(1.0) / stats[6])
    np.testing.assert_array_equal(bits32(gq[t["counts"], t["a"][t["counts"]]]), bits32((sc * d).astype(np.float32)[t["counts"]]))
    assert np.isfinite(stats).all()


def test_gamma_zero_ignores_the_next_state(case):
    kw = td_args(case, True, True, True, True, M=1023)
    want = td_loss_spec(**kw, gamma=0.0)
    rng = np.random.default_rng(3)
    other = dict(kw)
    for name in ("q_next_target", "q_next_online"):
        junk = rng.standard_normal(kw[name].shape).astype(np.float32)
        junk[rng.random(junk.shape) < 0.3] = np.nan
        junk[rng.random(junk.shape) < 0.1] = np.inf
        other[name] = junk
    other["masks_next"] = rng.integers(0, 256, size=kw["masks_next"].shape).astype(np.uint8)
    other["done"] = (rng.random(len(kw["done"])) < 0.5).astype(np.uint8)
    got = td_loss_spec(**other, gamma=0.0)
    np.testing.assert_array_equal(bits32(got[0]), bits32(want[0]))
    np.testing.assert_array_equal(bits32(got[1]), bits32(want[1]))
    np.testing.assert_array_equal(bits32(td_loss_backward_spec(**other, gamma=0.0, stats=got[0])),
                                  bits32(td_loss_backward_spec(**kw, gamma=0.0, stats=want[0])))
    assert np.isfinite(want[0]).all()


def test_a_nan_td_error_goes_through_loudly():
    M = 8
    q = np.ones((M, 5), np.float32)
    q[3] = np.nan
    kw = dict(q=q, actions=np.full(M, 2, np.uint8), reward=np.zeros(M), done=np.ones(M, np.uint8),
              q_next_target=np.zeros((M, 5), np.float32))
    stats, td = td_loss_spec(**kw)
    assert np.isnan(stats[0]) and np.isnan(td[3]) and stats[6] == M
    gq = td_loss_backward_spec(**kw, stats=stats)
    assert np.isnan(gq[3, 2]) and np.isfinite(np.delete(gq, 3, 0)).all()


# ------------------------------------------------------------------------------------------------- exploration
def _plain_batch(E, N, seed):
    rng = np.random.default_rng(seed)
    q = rng.standard_normal((E, N, 5)).astype(np.float32)
    zeros = np.zeros((E, N), np.uint8)
    step = rng.integers(0, 200, size=E).astype(np.int32)
    episode = rng.integers(0, 1000, size=E).astype(np.int32)
    return q, zeros, step, episode


def test_rates_zero_and_one_and_none():
    case = make_q_case(67, 8, seed=5)
    state = (case["terminated"], case["truncated"], case["step_count"], case["episode"])
    live = (case["terminated"] | case["truncated"]) == 0
    greedy = q_actions_spec(case["q_masked"], case["masks"], *state, seed=SEED, epsilon=None)
    zero = q_actions_spec(case["q_masked"], case["masks"], *state, seed=SEED, epsilon=0.0)
    np.testing.assert_array_equal(greedy[0], zero[0])
    assert not greedy[1].any() and not zero[1].any()
    one = q_actions_spec(case["q_masked"], case["masks"], *state, seed=SEED, epsilon=1.0)
    assert one[1][live].all() and not one[1][~live].any() and (one[0][~live] == 255).all()
    assert ((((case["masks"][live] & 0x1F) | 0x10) >> one[0][live]) & 1).all()        # the choice is legal
    nan = q_actions_spec(case["q_masked"], case["masks"], *state, seed=SEED, epsilon=float("nan"))
    np.testing.assert_array_equal(nan[0], greedy[0])
    # a row of NaNs gives the lowest legal action, a tie the lowest index
    rows = np.isnan(case["q_masked"]).all(-1) & live
    assert rows.any()
    lowest = legal_bits(case["masks"], (67, 8)).argmax(-1)
    np.testing.assert_array_equal(greedy[0][rows], lowest[rows])


def test_exploration_statistics():
    E, N, eps = 25_000, 8, 0.25                                          # 200 000 live slots
    q, zeros, step, episode = _plain_batch(E, N, seed=11)
    acts, expl = q_actions_spec(q, None, zeros, zeros, step, episode, seed=SEED, epsilon=eps)
    n = E * N
    share = expl.mean()
    sd = np.sqrt(eps * (1 - eps) / n)
    print(f"explored share {share:.5f} (eps {eps}, 4 sd = {4 * sd:.5f})")
    assert abs(share - eps) <= 4 * sd
    chosen = acts[expl != 0]
    m = len(chosen)
    sd5 = np.sqrt(0.2 * 0.8 / m)
    shares = np.bincount(chosen, minlength=5) / m
    print("shares of the five actions among explored slots:", shares, f"4 sd = {4 * sd5:.5f}")
    assert (np.abs(shares - 0.2) <= 4 * sd5).all()
    # the two draws of a slot are independent words: exploring says nothing about the choice made
    greedy = q_actions_spec(q, None, zeros, zeros, step, episode, seed=SEED, epsilon=None)[0]
    np.testing.assert_array_equal(acts[expl == 0], greedy[expl == 0])
    # under masks: uniform over each legal set (here: three legal actions, 0, 2 and wait)
    masks = np.full((E, N), 0x05, np.uint8)
    acts, expl = q_actions_spec(q, masks, zeros, zeros, step, episode, seed=SEED, epsilon=1.0)
    assert expl.all()
    shares = np.bincount(acts.reshape(-1), minlength=5) / n
    assert shares[1] == 0 and shares[3] == 0
    assert (np.abs(shares[[0, 2, 4]] - 1 / 3) <= 4 * np.sqrt((1 / 3) * (2 / 3) / n)).all()
