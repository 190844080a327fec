"""CCX_C51 on the device (include/ccx.h): ``q_values``, ``loss`` and ``loss_backward`` of ``CategoricalQ`` against the NumPy
spec (tests/_c51_spec.py) bit for bit -- q, stats, row_loss, proj and grad_logits -- on atom counts 2 (the minimum), 3, 33
(across the half wave), 51 (the default) and 64 (no padding lanes) and on row counts at every boundary of the tree; every NULL
combination of the optional inputs; the selects (done rows and rows that do not count full of NaN, a zero discount, loud
non-finite inputs, rewards beyond the support); identities that hold exactly on a support with dz = 0.5; leading shapes, zero
rows, autograd, a replayed graph, the refusals and the example.  f32 values are compared as bit patterns (NaN payloads
excepted: tests/_mlp_spec.bits32c)."""

import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
from _c51_spec import (ATOMS, C51_VARIANTS, c51_args, c51_loss_backward_spec, c51_loss_spec, dist, make_c51_case, q_values_spec)
from _mlp_spec import bits32c
from _qlearn_spec import greedy_spec, legal_bits
from _reset_obs_spec import make_config

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
FILL = 0xA5
ROWS = (1, 63, 64, 65, 255, 256, 257, 1000)
BIG = 16385                                                             # more than 64 block partials: the final wave strides twice
KEYS = ("logits", "actions", "reward", "done", "next_target", "next_online", "masks_next", "valid", "weights")


@pytest.fixture(scope="module")
def batch():
    import torch

    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    from collectivecrossing_amd.batched import BatchedCollectiveCrossing

    b = BatchedCollectiveCrossing(make_config(8, max_steps=12), 4)
    yield b
    b.close()


@pytest.fixture(scope="module")
def cases():
    made = {}

    def get(A, M=1000):
        if (A, M) not in made:
            made[A, M] = make_c51_case(M, A, seed=7 + A, special=M <= 1000)
        return made[A, M]
    return get


def own(kw):
    """A private copy of a case's arrays (the cases are shared among the tests and stay unchanged)."""
    return {k: (None if v is None else v.copy()) for k, v in kw.items()}


def cuda(kw):
    import torch

    return {k: (None if v is None else torch.from_numpy(np.ascontiguousarray(v)).cuda()) for k, v in kw.items()}


def run_device(cq, kw, gamma=None, want_row_loss=True, grad_loss=None):
    """(q, stats, row_loss, proj, grad_logits) as NumPy arrays from prefilled static buffers."""
    import torch

    d = cuda(kw)
    M = kw["actions"].shape
    out = cq.alloc_loss(M, want_row_loss=want_row_loss)
    q = torch.empty(tuple(M) + (5,), device="cuda")
    for t in (out.stats, out.row_loss, out.proj, out.grad_logits, q):
        if t is not None:
            t.view(torch.uint8).fill_(FILL)
    assert cq.q_values(d["logits"], out=q) is q
    got = cq.loss(*(d[k] for k in KEYS), gamma=gamma, discount=d["discount"], out=out)
    assert got is out
    gl = None if grad_loss is None else torch.tensor([grad_loss], device="cuda")
    g = cq.loss_backward(d["logits"], d["actions"], out.proj, d["valid"], d["weights"], stats=out.stats, grad_loss=gl, out=out)
    assert g is out.grad_logits
    cq.batch.synchronize()
    return (q.cpu().numpy(), out.stats.cpu().numpy(), None if out.row_loss is None else out.row_loss.cpu().numpy(),
            out.proj.cpu().numpy(), out.grad_logits.cpu().numpy())


def compare(cq, kw, gamma=None, want_row_loss=True, grad_loss=None):
    q, stats, row_loss, proj, grad = run_device(cq, kw, gamma, want_row_loss, grad_loss)
    g = 0.99 if gamma is None else gamma
    want_stats, want_rl, want_proj = c51_loss_spec(**kw, gamma=g, vmin=cq.vmin, vmax=cq.vmax)
    want_grad = c51_loss_backward_spec(kw["logits"], kw["actions"], want_proj, kw["valid"], kw["weights"], want_stats, grad_loss)
    np.testing.assert_array_equal(bits32c(q), bits32c(q_values_spec(kw["logits"], cq.vmin, cq.vmax)), err_msg="q_values")
    np.testing.assert_array_equal(bits32c(stats), bits32c(want_stats), err_msg="stats")
    if want_row_loss:
        np.testing.assert_array_equal(bits32c(row_loss), bits32c(want_rl), err_msg="row_loss")
    else:
        assert row_loss is None
    np.testing.assert_array_equal(bits32c(proj), bits32c(want_proj), err_msg="proj")
    np.testing.assert_array_equal(bits32c(grad), bits32c(want_grad), err_msg="grad_logits")
    return stats, want_rl, proj, grad


# ------------------------------------------------------------------------------------------------- 1. bits
@pytest.mark.parametrize("M", ROWS)
@pytest.mark.parametrize("A", ATOMS)
def test_kernels_equal_the_spec(batch, cases, A, M):
    from collectivecrossing_amd import CategoricalQ

    cq = CategoricalQ(batch, atoms=A)
    variant = C51_VARIANTS[(ATOMS.index(A) + ROWS.index(M)) % len(C51_VARIANTS)]
    kw = c51_args(cases(A), *variant, M=M)
    stats, _rl, _proj, _grad = compare(cq, kw, gamma=None if variant[4] else 0.97, want_row_loss=M % 2 == 1, grad_loss=-1.75)
    assert np.isfinite(stats).all()


@pytest.mark.parametrize("A", (3, 51))
def test_more_than_64_block_partials(batch, cases, A):
    from collectivecrossing_amd import CategoricalQ

    kw = c51_args(cases(A, BIG), True, True, True, True, True)
    stats, _rl, _proj, _grad = compare(CategoricalQ(batch, atoms=A), kw)
    assert np.isfinite(stats).all() and stats[6] > 10_000 and stats[7] > 100   # the bad actions 5..254 are tallied


@pytest.mark.parametrize("want_row_loss", (True, False))
@pytest.mark.parametrize("variant", C51_VARIANTS, ids=lambda v: "".join("1" if x else "0" for x in v))
def test_every_optional_input_given_and_not(batch, cases, variant, want_row_loss):
    from collectivecrossing_amd import CategoricalQ

    kw = c51_args(cases(51), *variant, M=257)
    stats, row_loss, proj, grad = compare(CategoricalQ(batch), kw, gamma=None if variant[4] else 0.9, want_row_loss=want_row_loss)
    assert np.isfinite(stats).all(), "a NaN of a row that does not count, or of a done row's next state, reached a sum"
    gone = (kw["actions"] > 4) | ((kw["valid"] == 0) if kw["valid"] is not None else False)
    assert gone.any() and np.isnan(kw["logits"][gone]).all()
    assert not row_loss[gone].view(np.uint32).any() and not proj[gone].view(np.uint32).any()      # +0.0, the sign bit included
    assert not grad[gone].view(np.uint32).any()
    bad = ((kw["valid"] != 0) if kw["valid"] is not None else True) & (kw["actions"] > 4) & (kw["actions"] != 255)
    assert stats[7] == bad.sum() > 0
    done_nan = (kw["done"] != 0) & np.isnan(kw["next_target"]).all((-1, -2)) & ~gone
    assert done_nan.any() and np.isfinite(proj[done_nan]).all() and np.isfinite(grad[done_nan]).all()


def test_gamma_zero_reads_no_next_state(batch, cases):
    from collectivecrossing_amd import CategoricalQ

    kw = own(c51_args(cases(33), False, True, False, False, False, M=300))
    kw["next_target"][:], kw["next_online"][:] = np.nan, np.nan
    stats, _rl, proj, grad = compare(CategoricalQ(batch, atoms=33), kw, gamma=0.0)
    assert np.isfinite(stats).all() and np.isfinite(proj).all() and np.isfinite(grad).all()


def test_non_finite_inputs_of_a_counting_row_are_loud(batch, cases):
    from collectivecrossing_amd import CategoricalQ

    kw = own(c51_args(cases(51), False, True, False, False, True, M=64))
    kw["actions"][:], kw["done"][:] = 2, 0
    kw["discount"][:], kw["reward"][:] = np.float32(0.99), 0.5
    for k in ("logits", "next_target", "next_online"):
        kw[k] = np.nan_to_num(kw[k], nan=0.25, posinf=0.25, neginf=0.25)
    kstar = c51_loss_spec(**kw, details=True)[3]["kstar"]
    kw["reward"][0], kw["reward"][1], kw["reward"][2] = np.nan, np.inf, -np.inf
    kw["discount"][3], kw["discount"][4] = np.nan, np.inf
    kw["logits"][5, 2, 7], kw["logits"][6, 2, 0], kw["logits"][7, 2, 50] = np.nan, np.inf, -np.inf
    kw["next_target"][8, kstar[8], 9], kw["next_target"][9, kstar[9], 1] = np.nan, -np.inf
    stats, row_loss, _proj, _grad = compare(CategoricalQ(batch), kw)
    assert not np.isfinite(row_loss[:10]).any() and np.isfinite(row_loss[10:]).all()
    assert np.isnan(row_loss[0]) and not np.isfinite(stats[0])


# ------------------------------------------------------------------------------------------------- 2. identities, no spec
def _exact(M=300, seed=9):
    rng = np.random.default_rng(seed)
    A = 33
    lg, nt, no = ((rng.standard_normal((M, 5, A)) * 2.0).astype(np.float32) for _ in range(3))
    return dict(logits=lg, actions=rng.integers(0, 5, size=M).astype(np.uint8), reward=np.zeros(M), done=np.zeros(M, np.uint8),
                next_target=nt, next_online=no, masks_next=rng.integers(0, 32, size=M).astype(np.uint8), valid=None, weights=None,
                discount=None), A


def test_identities_on_a_support_with_an_exact_spacing(batch):
    """vmin = -8, vmax = 8, A = 33: dz = 0.5 and every b_j is exact."""
    import torch

    from collectivecrossing_amd import CategoricalQ

    kw, A = _exact()
    cq = CategoricalQ(batch, atoms=A, vmin=-8.0, vmax=8.0)
    np.testing.assert_array_equal(cq.support.cpu().numpy(), np.linspace(-8.0, 8.0, A, dtype=np.float32))
    M = len(kw["actions"])
    # the greedy action of q_values(next_online) under masks_next is the k* whose distribution was projected
    qsel = cq.q_values(torch.from_numpy(kw["next_online"]).cuda()).cpu().numpy()
    kstar = greedy_spec(qsel, legal_bits(kw["masks_next"], (M,)))
    _d, e, S = dist(kw["next_target"][np.arange(M), kstar], A)
    p = (e / S[:, None]).astype(np.float32)[:, :A]
    _q, _stats, _rl, proj, _g = run_device(cq, kw, gamma=1.0)
    np.testing.assert_array_equal(proj.view(np.uint32), p.view(np.uint32), err_msg="reward 0, gamma 1: proj is the target itself")
    kw["reward"][:] = 1.0
    _q, _stats, _rl, proj, _g = run_device(cq, kw, gamma=1.0)
    np.testing.assert_array_equal(proj[:, 2:A - 1].view(np.uint32), p[:, :A - 3].view(np.uint32), err_msg="reward 1: two atoms up")
    assert not proj[:, :2].view(np.uint32).any()
    kw["reward"][::2], kw["reward"][1::2] = 100.0, -100.0
    _q, stats, row_loss, proj, _g = run_device(cq, kw, gamma=0.5)
    assert (np.abs(proj[::2, A - 1] - 1.0) < 1e-6).all() and not proj[::2, :A - 1].any(), "all mass on the top atom"
    assert (np.abs(proj[1::2, 0] - 1.0) < 1e-6).all() and not proj[1::2, 1:].any(), "all mass on the bottom atom"
    assert np.isfinite(stats).all() and (row_loss > 0).all()


# ------------------------------------------------------------------------------------------------- 3. shapes, autograd, graphs
def test_leading_shapes_and_zero_rows(batch, cases):
    import torch

    from collectivecrossing_amd import CategoricalQ

    cq = CategoricalQ(batch)
    kw = c51_args(cases(51), True, True, True, True, False, M=6 * 8)
    flat = run_device(cq, kw, gamma=0.97)
    shaped = {k: (None if v is None else v.reshape((6, 8) + v.shape[1:])) for k, v in kw.items()}
    got = run_device(cq, shaped, gamma=0.97)
    assert got[0].shape == (6, 8, 5) and got[2].shape == (6, 8) and got[3].shape == (6, 8, 51) and got[4].shape == (6, 8, 5, 51)
    for a, b in zip(flat, got):
        np.testing.assert_array_equal(bits32c(a).reshape(-1), bits32c(b).reshape(-1))
    d = cuda({k: (None if v is None else v[:0]) for k, v in kw.items()})
    r = cq.loss(*(d[k] for k in KEYS), want_row_loss=True)
    assert r.row_loss.shape == (0,) and r.proj.shape == (0, 51) and not r.stats.view(torch.int32).any()
    assert cq.q_values(d["logits"]).shape == (0, 5)
    assert cq.loss_backward(d["logits"], d["actions"], r.proj, stats=r.stats).shape == (0, 5, 51)
    x = d["logits"].clone().requires_grad_()
    cq.loss(x, *(d[k] for k in KEYS[1:])).loss.backward()
    assert x.grad.shape == (0, 5, 51)


def test_autograd_equals_loss_backward_and_two_runs_are_equal(batch, cases):
    import torch

    from collectivecrossing_amd import CategoricalQ

    cq = CategoricalQ(batch)
    kw = c51_args(cases(51), True, True, True, True, False, M=1000)
    d = cuda(kw)
    x = d["logits"].clone().requires_grad_()
    r = cq.loss(x, *(d[k] for k in KEYS[1:]), gamma=0.97, want_row_loss=True)
    (r.loss * 3.0).backward()
    ref = cq.loss_backward(d["logits"], d["actions"], r.proj, d["valid"], d["weights"], stats=r.stats,
                           grad_loss=torch.tensor([3.0], device="cuda"))
    again = cq.loss(d["logits"], *(d[k] for k in KEYS[1:]), gamma=0.97, want_row_loss=True)
    batch.synchronize()
    assert torch.equal(x.grad.view(torch.int32), ref.view(torch.int32)) and x.grad.abs().sum() > 0
    for a, b in ((r.stats, again.stats), (r.row_loss, again.row_loss), (r.proj, again.proj)):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    with pytest.raises(ValueError, match="out="):
        cq.loss(x, *(d[k] for k in KEYS[1:]), out=cq.alloc_loss((1000,)))
    with pytest.raises(ValueError, match="must not require a gradient"):
        cq.loss(x, *(d[k] for k in KEYS[1:4]), d["next_target"].clone().requires_grad_())


FRAME_ROWS = (1, 63, 257, 513)                                           # inside a wave, across one, a block + a row, two + a row


@pytest.mark.parametrize("present", (False, True), ids=("optional-absent", "optional-present"))
@pytest.mark.parametrize("M", FRAME_ROWS)
def test_the_three_call_forms_agree(batch, cases, M, present):
    """Fresh outputs, ``out=`` of ``alloc_loss`` and autograd write the spec's bits, so the same ones; the gradient that
    ``r.loss.backward()`` leaves is ``loss_backward(out=)``'s with ``grad_loss`` absent and with a 1.0f."""
    import torch

    from collectivecrossing_amd import CategoricalQ

    cq = CategoricalQ(batch)
    kw = c51_args(cases(51), present, present, present, present, present, M=M)
    gamma = None if present else 0.97                                    # (with a discount per row there is no gamma)
    d = cuda(kw)
    want_stats, want_rl, want_proj = c51_loss_spec(**kw, gamma=0.99 if gamma is None else gamma, vmin=cq.vmin, vmax=cq.vmax)
    want_grad = c51_loss_backward_spec(kw["logits"], kw["actions"], want_proj, kw["valid"], kw["weights"], want_stats, None)
    fresh = cq.loss(*(d[k] for k in KEYS), gamma=gamma, discount=d["discount"], want_row_loss=True)
    static = cq.alloc_loss((M,))
    for t in (static.stats, static.row_loss, static.proj, static.grad_logits):
        t.view(torch.uint8).fill_(FILL)
    assert cq.loss(*(d[k] for k in KEYS), gamma=gamma, discount=d["discount"], out=static) is static
    x = d["logits"].clone().requires_grad_()
    auto = cq.loss(x, *(d[k] for k in KEYS[1:]), gamma=gamma, discount=d["discount"], want_row_loss=True)
    auto.loss.backward()
    one = torch.ones(1, device="cuda")
    grads = [cq.loss_backward(d["logits"], d["actions"], static.proj, d["valid"], d["weights"], stats=static.stats, grad_loss=gl, out=o)
             for gl, o in ((None, static), (one, None))]
    batch.synchronize()
    assert fresh.workspace is None and auto.workspace is None and grads[0] is static.grad_logits
    for form, r in (("fresh", fresh), ("out=", static), ("autograd", auto)):
        np.testing.assert_array_equal(bits32c(r.stats.cpu().numpy()), bits32c(want_stats), err_msg="stats " + form)
        np.testing.assert_array_equal(bits32c(r.row_loss.cpu().numpy()), bits32c(want_rl), err_msg="row_loss " + form)
        np.testing.assert_array_equal(bits32c(r.proj.cpu().numpy()), bits32c(want_proj), err_msg="proj " + form)
    for form, g in (("autograd", x.grad), ("grad_loss None", grads[0]), ("grad_loss 1.0f", grads[1])):
        np.testing.assert_array_equal(bits32c(g.cpu().numpy()), bits32c(want_grad), err_msg="grad_logits " + form)


@pytest.mark.parametrize("why", ("valid all zero", "every action 255"))
def test_no_row_counts(batch, cases, why):
    """n = 0: the eight stats, every gradient element, row_loss and proj are +0.0f (all 32 bits clear), as the spec has them."""
    from collectivecrossing_amd import CategoricalQ

    cq = CategoricalQ(batch)
    M = 257
    kw = own(c51_args(cases(51), True, True, True, True, False, M=M))
    if why == "valid all zero":
        kw["valid"][:] = 0
    else:
        kw["actions"][:] = 255
    want_stats, want_rl, want_proj = c51_loss_spec(**kw, gamma=0.97, vmin=cq.vmin, vmax=cq.vmax)
    want_grad = c51_loss_backward_spec(kw["logits"], kw["actions"], want_proj, kw["valid"], kw["weights"], want_stats, None)
    for want in (want_stats, want_rl, want_proj, want_grad):
        assert not bits32c(want).any()
    _q, stats, row_loss, proj, grad = run_device(cq, kw, gamma=0.97)      # (every output prefilled with a sentinel)
    assert stats.shape == (8,) and row_loss.shape == (M,) and proj.shape == (M, 51) and grad.shape == (M, 5, 51)
    for name, a in (("stats", stats), ("row_loss", row_loss), ("proj", proj), ("grad_logits", grad)):
        assert not bits32c(a).any(), name


def test_zero_rows_in_the_three_call_forms(batch, cases, monkeypatch):
    import torch

    from collectivecrossing_amd import CategoricalQ

    cq = CategoricalQ(batch)
    d = {k: (None if v is None else v[:0]) for k, v in cuda(c51_args(cases(51), True, True, True, True, False, M=4)).items()}
    static = cq.alloc_loss((0,))
    static.stats.fill_(float("nan"))

    def called(*args, **kwargs):
        raise AssertionError("zero rows must not reach the library")

    monkeypatch.setattr(batch, "_enqueue", called)
    fresh = cq.loss(*(d[k] for k in KEYS), want_row_loss=True)
    assert cq.loss(*(d[k] for k in KEYS), out=static) is static
    x = d["logits"].clone().requires_grad_()
    auto = cq.loss(x, *(d[k] for k in KEYS[1:]), want_row_loss=True)
    assert auto.loss.requires_grad and not auto.stats.requires_grad
    auto.loss.backward()
    for r in (fresh, static, auto):
        assert r.stats.shape == (8,) and not r.stats.view(torch.int32).any()
        assert r.row_loss.shape == (0,) and r.proj.shape == (0, 51)
    assert x.grad.shape == (0, 5, 51)
    assert cq.loss_backward(d["logits"], d["actions"], static.proj, stats=static.stats, out=static) is static.grad_logits


def test_static_buffers_captured_and_replayed(cases):
    import torch

    from collectivecrossing_amd import CategoricalQ
    from collectivecrossing_amd.batched import BatchedCollectiveCrossing

    M, A = 700, 51
    env = BatchedCollectiveCrossing(make_config(8, max_steps=12), 4)
    side = torch.cuda.Stream()
    env.use_stream(side)
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        cq = CategoricalQ(env, atoms=A)
        kw = c51_args(cases(A), True, True, True, True, True, M=M)
        d = cuda(kw)
        eager = cq.alloc_loss((M,))
        cq.loss(*(d[k] for k in KEYS), discount=d["discount"], out=eager)
        cq.loss_backward(d["logits"], d["actions"], eager.proj, d["valid"], d["weights"], stats=eager.stats, out=eager)
        out = cq.alloc_loss((M,))
        side.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            cq.loss(*(d[k] for k in KEYS), discount=d["discount"], out=out)
            cq.loss_backward(d["logits"], d["actions"], out.proj, d["valid"], d["weights"], stats=out.stats, out=out)
        for _ in range(2):
            for t in (out.stats, out.row_loss, out.proj, out.grad_logits):
                t.view(torch.uint8).fill_(FILL)
            graph.replay()
            side.synchronize()
            for name in ("stats", "row_loss", "proj", "grad_logits"):
                assert torch.equal(getattr(out, name).view(torch.int32), getattr(eager, name).view(torch.int32)), name
    env.use_stream(None)
    env.close()


# ------------------------------------------------------------------------------------------------- 4. refusals
def test_refusals_leave_the_batch_usable(batch, cases):
    import torch

    from collectivecrossing_amd import CategoricalQ, _abi

    for bad in (dict(atoms=1), dict(atoms=65), dict(atoms=51.0), dict(vmin=1.0, vmax=1.0), dict(vmin=2.0, vmax=1.0),
                dict(vmax=float("inf")), dict(vmin=float("nan")), dict(vmin=-3e38, vmax=3e38)):
        with pytest.raises(ValueError):
            CategoricalQ(batch, **bad)
    with pytest.raises(ValueError):
        CategoricalQ(object())
    A, M = 51, 65
    cq = CategoricalQ(batch)
    kw = c51_args(cases(A), True, True, True, True, True, M=M)
    d = cuda(kw)
    good = cq.loss(*(d[k] for k in KEYS), discount=d["discount"], want_row_loss=True)
    batch.synchronize()
    shifted = torch.empty(M * 5 * A + 1, device="cuda")[1:].view(M, 5, A)
    assert shifted.data_ptr() % 16 == 4
    cq.loss(shifted.copy_(d["logits"]), *(d[k] for k in KEYS[1:]))       # f32 alignment is all the logits need
    for name, bad in (("logits", d["logits"].double()), ("logits", d["logits"][:, :, :50]), ("logits", d["logits"].cpu()),
                      ("logits", d["logits"].transpose(0, 1)), ("logits", None), ("actions", d["actions"].long()),
                      ("actions", d["actions"][:-1]), ("reward", d["reward"].float()), ("done", d["done"].bool()),
                      ("next_target", d["next_target"][:, :4]), ("next_online", d["next_online"].half()),
                      ("masks_next", d["masks_next"].int()), ("valid", d["valid"].bool()), ("weights", d["weights"].double())):
        args = dict(d, **{name: bad})
        with pytest.raises(ValueError):
            cq.loss(*(args[k] for k in KEYS))
    for kwargs in (dict(gamma=0.9, discount=d["discount"]), dict(gamma=1.5), dict(gamma=float("nan")), dict(gamma="x"),
                   dict(discount=d["discount"].double()), dict(out=batch.alloc_sample())):
        with pytest.raises(ValueError):
            cq.loss(*(d[k] for k in KEYS), **kwargs)
    q_shift = torch.empty(M * 5 + 1, device="cuda")[1:].view(M, 5)
    for kwargs in (dict(out=q_shift), dict(out=torch.empty((M, 6), device="cuda"))):
        with pytest.raises(ValueError):
            cq.q_values(d["logits"], **kwargs)
    for kwargs in (dict(stats=good.stats[:7]), dict(stats=good.stats, grad_loss=torch.ones(2, 2, device="cuda")),
                   dict(stats=good.stats, out=torch.empty((M, 5, 50), device="cuda"))):
        with pytest.raises(ValueError):
            cq.loss_backward(d["logits"], d["actions"], good.proj, **kwargs)
    # the library's own refusals (the wrapper refuses first, so they are reached through the bindings)
    lib, h = batch._lib, batch._h
    p = {k: (None if v is None else v.data_ptr()) for k, v in d.items()}
    ws, st = cq._workspace_arg(None, M), torch.empty(8, device="cuda")
    q, proj = torch.empty((M, 5), device="cuda"), torch.empty((M, A), device="cuda")

    def loss_args(**over):
        a = dict(h=h, rows=M, atoms=A, vmin=-10.0, vmax=10.0, logits=p["logits"], actions=p["actions"], reward=p["reward"],
                 done=p["done"], nt=p["next_target"], no=p["next_online"], masks=p["masks_next"], valid=p["valid"],
                 weights=p["weights"], discount=None, gamma=0.99, ws=ws.data_ptr(), stats=st.data_ptr(), row_loss=None,
                 proj=proj.data_ptr())
        a.update(over)
        return tuple(a.values())
    assert lib.ccx_c51_loss(*loss_args()) == _abi.OK
    inf, nan = float("inf"), float("nan")
    for over, word in ((dict(h=None), "NULL handle"), (dict(logits=None), "NULL"), (dict(proj=None), "NULL"), (dict(ws=None), "NULL"),
                       (dict(rows=0), "rows"), (dict(atoms=1), "atoms"), (dict(atoms=65), "atoms"), (dict(vmin=nan), "finite"),
                       (dict(vmax=inf), "finite"), (dict(vmin=10.0), "finite"), (dict(gamma=1.5), "gamma"), (dict(gamma=nan), "gamma"),
                       (dict(logits=p["logits"] + 2), "aligned"), (dict(ws=ws.data_ptr() + 4), "aligned"),
                       (dict(reward=p["reward"] + 4), "aligned")):
        assert lib.ccx_c51_loss(*loss_args(**over)) == _abi.EINVAL, (over, word)
        assert word in lib.ccx_last_error().decode(), (word, lib.ccx_last_error())
    assert lib.ccx_c51_loss(*loss_args(discount=p["discount"], gamma=nan)) == _abi.OK     # with discount, gamma is not read
    for args, word in (((None, M, A, -10.0, 10.0, p["logits"], q.data_ptr()), "NULL handle"),
                       ((h, M, A, -10.0, 10.0, p["logits"], None), "NULL"), ((h, -1, A, -10.0, 10.0, p["logits"], q.data_ptr()), "rows"),
                       ((h, M, 0, -10.0, 10.0, p["logits"], q.data_ptr()), "atoms"),
                       ((h, M, A, -10.0, 10.0, p["logits"], q_shift.data_ptr()), "aligned")):
        assert lib.ccx_c51_q_values(*args) == _abi.EINVAL, word
        assert word in lib.ccx_last_error().decode(), (word, lib.ccx_last_error())
    g = torch.empty((M, 5, A), device="cuda")
    tail = (p["valid"], p["weights"], good.stats.data_ptr(), None, g.data_ptr())
    for args, word in (((None, M, A, p["logits"], p["actions"], good.proj.data_ptr(), *tail), "NULL handle"),
                       ((h, M, A, p["logits"], p["actions"], None, *tail), "NULL"),
                       ((h, 0, A, p["logits"], p["actions"], good.proj.data_ptr(), *tail), "rows"),
                       ((h, M, 66, p["logits"], p["actions"], good.proj.data_ptr(), *tail), "atoms"),
                       ((h, M, A, p["logits"], p["actions"], good.proj.data_ptr() + 1, *tail), "aligned")):
        assert lib.ccx_c51_loss_backward(*args) == _abi.EINVAL, word
        assert word in lib.ccx_last_error().decode(), (word, lib.ccx_last_error())
    assert lib.ccx_c51_workspace_bytes(0) == 0 and lib.ccx_c51_workspace_bytes(257) == 2 * 6 * 8
    batch.synchronize()
    again = cq.loss(*(d[k] for k in KEYS), discount=d["discount"], want_row_loss=True)
    batch.synchronize()
    for a, b in ((good.stats, again.stats), (good.row_loss, again.row_loss), (good.proj, again.proj)):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))


# ------------------------------------------------------------------------------------------------- 5. the example
def test_the_example_runs_with_a_tiny_configuration():
    code = ("import sys; sys.path.insert(0, 'examples'); import c51_dqn as ex; "
            "stats, (ours, theirs, close) = ex.train(num_envs=32, updates=6, ring_steps=8, batch=64, warmup_steps=4, target_every=3, "
            "anneal_updates=4, atoms=51, hidden=16, log_every=2); "
            "assert ours and len(stats) == 6 and all(s[6] > 0 and s[0] == s[0] for s in stats) and close < 1e-4; print('ok', ours, theirs)")
    run = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True, timeout=300)
    print(run.stdout[-1500:])
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-4000:]
    assert "ok True" in run.stdout and run.stdout.count("update ") == 3
