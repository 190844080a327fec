"""The TD loss with a discount per row (include/ccx.h CCX_NSTEP: ``ccx_td_loss_discounted`` and its backward) on the device: a
discount array filled with one value against ``td_loss(gamma=)`` -- kernel against kernel, bit for bit: stats, td_error and
grad_q -- with double-Q on and off, on row counts around the group, block and final-wave boundaries of the tree, for every
NULL combination ``tests/test_gpu_qlearn.py`` walks; a mixed array, with values from an actual n-step fetch and zeros among
them, against the NumPy rule of tests/_qlearn_spec.py applied with each row's own discount; and the autograd path."""

import numpy as np
import pytest
from _nstep_cases import synthetic
from _qlearn_spec import TD_VARIANTS, make_td_case, td_args, td_loss_backward_spec, td_loss_spec
from _replay_spec import ARRAYS
from _reset_obs_spec import make_config
from _sample_spec import bits32

pytestmark = pytest.mark.gpu

ROWS = (1, 63, 64, 65, 255, 256, 257, 1025)
GAMMA, DELTA = 0.97, 1.0
KEYS = ("q", "actions", "reward", "done", "q_next_target", "q_next_online", "masks_next", "valid", "weights")


@pytest.fixture(scope="module")
def ql8():
    import torch

    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    from collectivecrossing_amd import QLearning
    from collectivecrossing_amd.batched import BatchedCollectiveCrossing

    b = BatchedCollectiveCrossing(make_config(8, max_steps=12), 4)
    yield b, QLearning(b)
    b.close()


@pytest.fixture(scope="module")
def td_case():
    return make_td_case(max(ROWS), seed=43, huber_delta=DELTA)


@pytest.fixture(scope="module")
def fetched_discounts():
    """The discounts of an actual n-step fetch (the synthetic ring of tests/_nstep_cases.py on the device, n = 3, gamma =
    0.97: gamma, gamma^2 and gamma^3 occur), with zeros put among them."""
    import torch

    from collectivecrossing_amd import NStepReplay, ReplayRing
    from collectivecrossing_amd.batched import BatchedCollectiveCrossing

    spec, cut, _ = synthetic(N=3)
    b = BatchedCollectiveCrossing(make_config(3, max_steps=12), spec["E"])
    try:
        ns = NStepReplay(ReplayRing(b, steps=spec["S"]), n=3, gamma=GAMMA)
        for k in ARRAYS:
            getattr(ns.ring, k).copy_(torch.from_numpy(spec[k]))
        ns.ring.state.copy_(torch.from_numpy(spec["state"]))
        ns.cut.copy_(torch.from_numpy(cut))
        disc = ns.fetch(torch.arange(spec["S"] * spec["E"], device="cuda")).discount.cpu().numpy().reshape(-1)
    finally:
        b.close()
    assert len(np.unique(disc)) == 3
    tiled = np.resize(disc, max(ROWS)).astype(np.float32)
    tiled[np.random.default_rng(5).random(len(tiled)) < 0.15] = 0.0
    return tiled


def _cuda(kw):
    import torch

    return {k: None if v is None else torch.from_numpy(v).cuda() for k, v in kw.items()}


def _same(a, b, msg):
    np.testing.assert_array_equal(bits32(a.cpu().numpy()), bits32(b if isinstance(b, np.ndarray) else b.cpu().numpy()), err_msg=msg)


@pytest.mark.parametrize("M", ROWS)
def test_one_value_everywhere_has_the_bits_of_gamma(ql8, td_case, M):
    import torch

    batch, ql = ql8
    gloss = torch.tensor([-1.75], device="cuda")
    for gamma in (GAMMA, 0.0, 1.0):
        disc = torch.full((M,), gamma, dtype=torch.float32, device="cuda")
        for variant in TD_VARIANTS:
            tag = f"M {M} gamma {gamma} masked {variant[0]} double {variant[1]} valid {variant[2]} weights {variant[3]}"
            d = _cuda(td_args(td_case, *variant, M=M))
            args = [d[k] for k in KEYS]
            a = ql.td_loss(*args, gamma=gamma, huber_delta=DELTA, out=ql.alloc_td_loss((M,)))
            b = ql.td_loss(*args, discount=disc, huber_delta=DELTA, out=ql.alloc_td_loss((M,)))
            _same(b.stats, a.stats, "stats " + tag)
            _same(b.td_error, a.td_error, "td_error " + tag)
            for gl in (None, gloss):
                ga = ql.td_loss_backward(*args, gamma=gamma, huber_delta=DELTA, stats=a.stats, grad_loss=gl)
                gb = ql.td_loss_backward(*args, discount=disc, huber_delta=DELTA, stats=b.stats, grad_loss=gl, out=b)
                assert gb is b.grad_q
                _same(gb, ga, "grad_q " + tag)
            if gamma != GAMMA:
                break                                                    # (the edges of the range: one variant)
    assert float(a.stats[6]) > 0 or M < 3


@pytest.mark.parametrize("M", ROWS)
def test_mixed_discounts_equal_the_rule_with_each_rows_own(ql8, td_case, fetched_discounts, M):
    import torch

    batch, ql = ql8
    disc = np.ascontiguousarray(fetched_discounts[:M])
    dd = torch.from_numpy(disc).cuda()
    for variant in TD_VARIANTS:
        tag = f"M {M} masked {variant[0]} double {variant[1]} valid {variant[2]} weights {variant[3]}"
        kw = td_args(td_case, *variant, M=M)
        d = _cuda(kw)
        want_stats, want_td = td_loss_spec(**kw, gamma=disc, huber_delta=DELTA)
        r = ql.td_loss(*(d[k] for k in KEYS), discount=dd, huber_delta=DELTA, want_td_error=True)
        g = ql.td_loss_backward(*(d[k] for k in KEYS), discount=dd, huber_delta=DELTA, stats=r.stats)
        _same(r.stats, want_stats, "stats " + tag)
        _same(r.td_error, want_td, "td_error " + tag)
        _same(g, td_loss_backward_spec(**kw, gamma=disc, huber_delta=DELTA, stats=want_stats), "grad_q " + tag)
    if M >= 255:
        assert (disc == 0).any() and len(np.unique(disc)) == 4


def test_autograd_with_a_discount_and_the_refusals(ql8, td_case, fetched_discounts):
    import torch

    batch, ql = ql8
    M = 257
    d = _cuda(td_args(td_case, True, True, True, True, M=M))
    dd = torch.from_numpy(np.ascontiguousarray(fetched_discounts[:M])).cuda()
    static = ql.td_loss(*(d[k] for k in KEYS), discount=dd, want_td_error=True)
    want = ql.td_loss_backward(*(d[k] for k in KEYS), discount=dd, stats=static.stats)
    q = d["q"].clone().requires_grad_()
    r = ql.td_loss(q, *(d[k] for k in KEYS[1:]), discount=dd, want_td_error=True)
    assert r.loss.requires_grad
    (r.loss * 1.0).backward()
    batch.synchronize()
    _same(r.stats, static.stats, "stats")
    _same(r.td_error, static.td_error, "td_error")
    _same(q.grad, want, "grad_q")
    assert q.grad.abs().sum() > 0
    other = ql.td_loss(*(d[k] for k in KEYS), gamma=GAMMA)
    assert not torch.equal(other.stats, static.stats)                    # the discount is read
    lead3 = {k: (None if v is None else v[:256].reshape((4, 8, 8) + tuple(v.shape[1:]))) for k, v in d.items()}
    r3 = ql.td_loss(*(lead3[k] for k in KEYS), discount=dd[:256].reshape(4, 8, 8), want_td_error=True)
    flat = ql.td_loss(*(None if d[k] is None else d[k][:256] for k in KEYS), discount=dd[:256].contiguous(), want_td_error=True)
    _same(r3.stats, flat.stats, "leading shape")
    empty = ql.td_loss(*(None if d[k] is None else d[k][:0] for k in KEYS), discount=dd[:0])
    assert not empty.stats.any()
    args = [d[k] for k in KEYS]
    bad = [dict(discount=dd, gamma=0.9), dict(discount=dd.double()), dict(discount=dd[:-1]), dict(discount=dd.cpu()),
           dict(discount=torch.stack([dd, dd], 1)[:, 0]), dict(discount=dd.clone().requires_grad_()), dict(discount=[0.9] * M)]
    for n, kw in enumerate(bad):
        with pytest.raises(ValueError):
            ql.td_loss(*args, **kw)
            pytest.fail(f"refusal {n} did not raise")
        with pytest.raises(ValueError):
            ql.td_loss_backward(*args, **kw, stats=static.stats)
            pytest.fail(f"backward refusal {n} did not raise")
    again = ql.td_loss(*args, discount=dd)
    _same(again.stats, static.stats, "after the refusals")
