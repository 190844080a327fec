"""Stored actions under new logits on the device (include/ccx.h: CCX_EVALUATE) against the NumPy spec
(tests/_evaluate_spec.py): forward and backward bits on row counts that cross every boundary of the kernels' layout, every
output element written and nothing behind it, the live sampling kernel against the live evaluate kernel, the autograd
Function, other streams and graph capture, and the refusals.  f32 values are compared as bit patterns throughout."""

import numpy as np
import pytest
from _evaluate_spec import (EVAL_JAC_ENTROPY_BOUND, EVAL_JAC_LOGP_BOUND, case_args, evaluate_backward_spec, evaluate_spec,
                            make_evaluate_case)
from _reset_obs_spec import make_config
from _sample_spec import bits32, make_sample_case

pytestmark = pytest.mark.gpu

# rows: every 5 M % 4 (1, 3, 4, 63 ...), the wave boundary (63 / 64 / 65), the 80-piece boundary of a wave's second load
# (79 / 80 / 81), two waves and one row (129), and a multi-wave tail (6500 = 101 waves and 36 rows)
ROWS = (1, 3, 4, 63, 64, 65, 79, 80, 81, 129, 6500)
LEADING = (3, 7, 5)                                                      # a [3, 7, 5, 5] logits tensor: 105 rows
GRADS = ((True, True), (True, False), (False, True))
SENTINEL = 0xEE
GUARD = 64                                                               # elements behind every output that must stay untouched
E, N = 8, 8                                                              # the batch: 8 envs x 8 agents on the 12 x 8 grid


@pytest.fixture(scope="module")
def batch():
    import torch

    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    from collectivecrossing_amd.batched import BatchedCollectiveCrossing

    b = BatchedCollectiveCrossing(make_config(N, max_steps=12), E)
    assert b.num_agents == N
    yield b
    b.close()


@pytest.fixture(scope="module")
def reference():
    """One generator case of max(ROWS) rows and the spec's answers on it, computed once: rows are independent, so the
    answers for M rows are the first M of each array.  Keys: (masked) -> logp, entropy; (masked, with_lp, with_ent) -> grad."""
    case = make_evaluate_case(max(ROWS), 1, seed=21)
    want = {}
    for masked in (True, False):
        logits, actions, masks, glp, gent = case_args(case, masked)
        want[masked] = evaluate_spec(logits, actions, masks)
        for with_lp, with_ent in GRADS:
            want[masked, with_lp, with_ent] = evaluate_backward_spec(logits, actions, masks, glp if with_lp else None,
                                                                     gent if with_ent else None)
    return case, want


def _dev(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _guarded(shape):
    """A sentinel-filled f32 buffer and its leading view of `shape`; GUARD elements lie behind the view."""
    import torch

    n = int(np.prod(shape))
    buf = torch.empty(n + GUARD, dtype=torch.float32, device="cuda")
    buf.view(torch.uint8).fill_(SENTINEL)
    return buf, buf[:n].view(shape)


def _guard_intact(buf, n):
    import torch

    return bool((buf[n:].view(torch.uint8) == SENTINEL).all())


def _device_inputs(case, masked, M, lead=None):
    logits, actions, masks, glp, gent = (None if a is None else a[:M] for a in case_args(case, masked))
    lead = (M,) if lead is None else lead
    return (_dev(logits).view(lead + (5,)), _dev(actions).view(lead), None if masks is None else _dev(masks).view(lead),
            _dev(glp).view(lead), _dev(gent).view(lead))


def _check_bits(batch, case, want, M, lead=None):
    import torch

    from collectivecrossing_amd import EvalResult

    lead = (M,) if lead is None else lead
    for masked in (True, False):
        logits, actions, masks, glp, gent = _device_inputs(case, masked, M, lead)
        for want_entropy in (True, False):
            b1, logp = _guarded(lead)
            b2, entropy = _guarded(lead) if want_entropy else (None, None)
            got = batch.evaluate_actions(logits, actions, masks, out=EvalResult(logp, entropy))
            batch.synchronize()
            assert got.logp is logp and got.entropy is entropy
            tag = f"M {M} lead {lead} masked {masked} entropy {want_entropy}"
            np.testing.assert_array_equal(bits32(logp.cpu().numpy().reshape(M)), bits32(want[masked][0][:M]), err_msg="logp " + tag)
            assert _guard_intact(b1, M), tag
            if want_entropy:
                np.testing.assert_array_equal(bits32(entropy.cpu().numpy().reshape(M)), bits32(want[masked][1][:M]),
                                              err_msg="entropy " + tag)
                assert _guard_intact(b2, M), tag
        for with_lp, with_ent in GRADS:
            b3, grad = _guarded(lead + (5,))
            got = batch.evaluate_actions_backward(logits, actions, masks, glp if with_lp else None, gent if with_ent else None,
                                                  out=grad)
            batch.synchronize()
            assert got is grad
            tag = f"M {M} lead {lead} masked {masked} grad_logp {with_lp} grad_entropy {with_ent}"
            np.testing.assert_array_equal(bits32(grad.cpu().numpy().reshape(M, 5)), bits32(want[masked, with_lp, with_ent][:M]),
                                          err_msg="grad_logits " + tag)
            assert _guard_intact(b3, 5 * M), tag
    # fresh outputs and the default arguments
    logits, actions, masks, glp, gent = _device_inputs(case, True, M, lead)
    res = batch.evaluate_actions(logits, actions, masks)
    g = batch.evaluate_actions_backward(logits, actions, masks, glp, gent)
    batch.synchronize()
    assert res.logp.shape == lead and res.entropy.shape == lead and g.shape == lead + (5,) and g.dtype is torch.float32
    np.testing.assert_array_equal(bits32(res.logp.cpu().numpy().reshape(M)), bits32(want[True][0][:M]))
    np.testing.assert_array_equal(bits32(g.cpu().numpy().reshape(M, 5)), bits32(want[True, True, True][:M]))
    assert batch.evaluate_actions(logits, actions, masks, want_entropy=False).entropy is None


# ------------------------------------------------------------------------------------------------- 1. bits against the spec
@pytest.mark.parametrize("M", ROWS)
def test_bits_against_the_spec_every_element_written(batch, reference, M):
    case, want = reference
    _check_bits(batch, case, want, M)
    if M == max(ROWS):                                                   # what the case holds (the smaller ones are its head)
        actions = case["actions"]
        assert (actions == 255).any() and ((actions > 4) & (actions < 255)).any() and np.isneginf(want[True][0]).any()
        assert np.isnan(case["logits_masked"]).any() and not np.isfinite(case["grad_logp"]).all()
        assert all(np.isfinite(want[True, a, b]).all() for a, b in GRADS)


def test_bits_with_a_leading_shape(batch, reference):
    case, want = reference
    _check_bits(batch, case, want, int(np.prod(LEADING)), LEADING)


# ------------------------------------------------------------------------------------------------- 2. kernel against kernel
def test_evaluate_reproduces_the_sampling_kernels_bits(batch):
    case = make_sample_case(E, N, seed=5)
    dead = (case["terminated"] | case["truncated"]) != 0
    assert dead.any() and not dead.all()
    batch.set_state(terminated=case["terminated"], truncated=case["truncated"], step_count=case["step_count"],
                    episode=case["episode"])
    batch.set_rng_seed(0x1234_5678_9ABC_DEF0)
    for masked in (True, False):
        logits = _dev(case["logits_masked"] if masked else case["logits"])
        masks = _dev(case["masks"]) if masked else None
        for det in (False, True):
            s = batch.sample_actions(logits, masks, deterministic=det, want_logp=True, want_entropy=True)
            r = batch.evaluate_actions(logits, s.actions, masks)
            batch.synchronize()
            acts = s.actions.cpu().numpy()
            assert (acts[dead] == 255).all() and (acts[~dead] < 5).all()
            for name, a, b in (("logp", r.logp, s.logp), ("entropy", r.entropy, s.entropy)):
                np.testing.assert_array_equal(bits32(a.cpu().numpy()), bits32(b.cpu().numpy()),
                                              err_msg=f"{name} masked {masked} deterministic {det}")
            assert not bits32(r.logp.cpu().numpy())[dead].any() and not bits32(r.entropy.cpu().numpy())[dead].any()
    batch.set_state(terminated=np.zeros((E, N), np.uint8), truncated=np.zeros((E, N), np.uint8))


# ------------------------------------------------------------------------------------------------- 3. autograd
AUTOGRAD_M = 645                                                         # ten waves and five rows; 5 M % 4 == 1


def torch_composition(logits, actions, masks, c1, c2):
    """The gradient of (c1 * logp + c2 * entropy).sum() as a user writes it with torch alone, in the dtype and on the device
    of `logits` (rows with a legal stored action only)."""
    import torch

    from collectivecrossing_amd import unpack_action_masks

    x = logits.detach().clone().requires_grad_(True)
    legal = unpack_action_masks(masks | 0x10)
    lp = torch.log_softmax(x.masked_fill(~legal, -torch.inf), -1)
    p = lp.exp()
    zero = torch.zeros_like(lp)
    entropy = -torch.where(p > 0, p * torch.where(p > 0, lp, zero), zero).sum(-1)
    logp = lp.gather(-1, actions.long()[..., None])[..., 0]
    loss = (c1 * logp + c2 * entropy).sum()
    return torch.autograd.grad(loss, x)[0]


def test_autograd_matches_the_backward_spec_and_torchs_composition(batch, reference):
    import torch

    case, _ = reference
    M = AUTOGRAD_M
    logits_np, actions_np, masks_np, _, _ = (a[:M] for a in case_args(case, True))
    rng = np.random.default_rng(3)
    c1_np, c2_np = rng.standard_normal(M).astype(np.float32), rng.standard_normal(M).astype(np.float32)
    actions, masks, c1, c2 = _dev(actions_np), _dev(masks_np), _dev(c1_np), _dev(c2_np)
    logits = _dev(logits_np).requires_grad_(True)
    assert np.isnan(logits_np).any() and (actions_np == 255).any()       # NaN at illegal places and in absent rows

    r = batch.evaluate_actions(logits, actions, masks)
    assert r.logp.requires_grad and r.entropy.requires_grad and r.logp.grad_fn is not None
    fwd = evaluate_spec(logits_np, actions_np, masks_np)
    np.testing.assert_array_equal(bits32(r.logp.detach().cpu().numpy()), bits32(fwd[0]))
    np.testing.assert_array_equal(bits32(r.entropy.detach().cpu().numpy()), bits32(fwd[1]))
    g, = torch.autograd.grad((c1 * r.logp + c2 * r.entropy).sum(), logits)
    want = evaluate_backward_spec(logits_np, actions_np, masks_np, c1_np, c2_np)
    np.testing.assert_array_equal(bits32(g.cpu().numpy()), bits32(want), err_msg="both outputs in the loss")
    assert np.isfinite(g.cpu().numpy()).all()                            # no NaN from the logits reaches a gradient

    # a loss that uses one output only: the other's gradient arrives as None and goes to the library as NULL
    r = batch.evaluate_actions(logits, actions, masks)
    g_lp, = torch.autograd.grad((c1 * r.logp).sum(), logits)
    np.testing.assert_array_equal(bits32(g_lp.cpu().numpy()), bits32(evaluate_backward_spec(logits_np, actions_np, masks_np, c1_np, None)))
    r = batch.evaluate_actions(logits, actions, masks)
    g_ent, = torch.autograd.grad((c2 * r.entropy).sum(), logits)
    np.testing.assert_array_equal(bits32(g_ent.cpu().numpy()), bits32(evaluate_backward_spec(logits_np, actions_np, masks_np, None, c2_np)))
    r = batch.evaluate_actions(logits, actions, masks, want_entropy=False)
    assert r.entropy is None
    g_lp2, = torch.autograd.grad((c1 * r.logp).sum(), logits)
    assert torch.equal(g_lp2, g_lp)
    # a non-contiguous incoming gradient (an expanded scalar) is made contiguous
    r = batch.evaluate_actions(logits, actions, masks)
    ok = torch.isfinite(r.logp.detach())
    g_sum, = torch.autograd.grad(torch.where(ok, r.logp, torch.zeros_like(r.logp)).sum(), logits)
    np.testing.assert_array_equal(bits32(g_sum.cpu().numpy()),
                                  bits32(evaluate_backward_spec(logits_np, actions_np, masks_np, ok.cpu().numpy().astype(np.float32), None)))

    # no graph is built when no gradient is asked for
    plain = batch.evaluate_actions(logits.detach(), actions, masks)
    assert not plain.logp.requires_grad and plain.logp.grad_fn is None and plain.entropy.grad_fn is None
    with torch.no_grad():
        quiet = batch.evaluate_actions(logits, actions, masks)
    assert not quiet.logp.requires_grad and quiet.logp.grad_fn is None
    batch.synchronize()
    np.testing.assert_array_equal(bits32(quiet.logp.cpu().numpy()), bits32(fwd[0]))

    # against torch's own f32 composition on well-conditioned rows: class "plain" (logits ~ N(0, 3)), the stored action
    # legal.  Both are f32 approximations of the same exact gradient c1 J_logp + c2 J_entropy.  Ours lies within its
    # measured bounds of it (tests/test_evaluate_spec.py, per unit incoming gradient, relative to max(1, |J|), |J| <= ~20
    # here); torch's composition is allowed 8 f32 roundings (8 x 2^-24 = 4.8e-7) on the same scale -- its exp, log and
    # five-term sums are not correctly rounded step by step.
    legal_a = (actions_np < 5) & (((masks_np | 0x10) >> np.minimum(actions_np, 4)) & 1).astype(bool)
    rows = (case["classes"][:M] <= 2) & legal_a
    assert rows.sum() > 100
    idx = _dev(np.flatnonzero(rows))
    t = torch_composition(torch.nan_to_num(logits.detach()[idx]), actions[idx], masks[idx], c1[idx], c2[idx]).cpu().numpy()
    ours = g.cpu().numpy()[rows]
    scale = np.maximum(1.0, np.abs(ours.astype(np.float64)))
    tol = (np.abs(c1_np[rows]) * (EVAL_JAC_LOGP_BOUND + 8 * 2.0 ** -24) + np.abs(c2_np[rows]) * (EVAL_JAC_ENTROPY_BOUND + 8 * 2.0 ** -24))
    err = np.abs(ours.astype(np.float64) - t) / scale
    print(f"against torch's f32 composition: max err / tol {float((err / tol[:, None]).max()):.3f}, max err {float(err.max()):.3e}")
    assert (err <= tol[:, None]).all()


# ------------------------------------------------------------------------------------------------- 4. streams and capture
def test_another_current_stream(batch, reference):
    """torch's current stream is not the handle's stream, and a blocker (tests/_stream_order.py) keeps one of the two
    busy: first the current one, so the launches must wait for inputs produced behind it; then the handle's, so the torch
    ops that consume the results at once must wait for the launches."""
    import torch
    from _stream_order import Blocker

    case, want = reference
    M = 129
    logits, actions, masks, glp, gent = _device_inputs(case, True, M)
    lg, ac, mk, _, _ = (a[:M] for a in case_args(case, True))
    blocker = Blocker()
    handle = batch._stream                                               # (where the batch launches)
    other = torch.cuda.Stream()
    blocker.warm(other, handle)
    for busy in (None, other, handle):                                   # (None: once without a blocker, the one-off host work)
        torch.cuda.synchronize()
        with torch.cuda.stream(other):                                   # torch's current stream is not the handle's stream
            ev = None if busy is None else blocker.run(busy)
            x = (logits * 1.0).requires_grad_(True)                      # produced on `other`
            r = batch.evaluate_actions(x, actions, masks)
            ok = torch.isfinite(glp) & torch.isfinite(gent)
            c1, c2 = torch.where(ok, glp, 0.5), torch.where(ok, gent, -0.25)
            g, = torch.autograd.grad((c1 * r.logp + c2 * r.entropy).sum(), x)
            early = [t.detach().clone() for t in (r.logp, r.entropy, g)]  # consumers enqueued at once, on `other`
            still_running = ev is None or not ev.query()
            got = [t.cpu().numpy() for t in early]
            c1_np, c2_np = c1.cpu().numpy(), c2.cpu().numpy()
        assert still_running, "blocker too short: it had ended before the consumers were enqueued"
        np.testing.assert_array_equal(bits32(got[0]), bits32(want[True][0][:M]))
        np.testing.assert_array_equal(bits32(got[1]), bits32(want[True][1][:M]))
        np.testing.assert_array_equal(bits32(got[2]), bits32(evaluate_backward_spec(lg, ac, mk, c1_np, c2_np)))


def test_captured_autograd_and_static_buffers(batch, reference):
    import torch

    case, want = reference
    M = 129
    lg, ac, mk, _, _ = (a[:M] for a in case_args(case, True))
    other_case = make_evaluate_case(M, 1, seed=77)
    lg2 = case_args(other_case, True)[0]
    lg2 = np.where(np.isnan(lg), lg, np.where(np.isnan(lg2), np.float32(0.5), lg2)).astype(np.float32)    # NaN where the first has it
    rng = np.random.default_rng(9)
    c1_np, c2_np = rng.standard_normal(M).astype(np.float32), rng.standard_normal(M).astype(np.float32)
    specs = [(evaluate_spec(x, ac, mk), evaluate_backward_spec(x, ac, mk, c1_np, c2_np)) for x in (lg, lg2)]
    side = torch.cuda.Stream()
    batch.use_stream(side)
    torch.cuda.synchronize()
    try:
        with torch.cuda.stream(side):
            actions, masks, c1, c2 = _dev(ac), _dev(mk), _dev(c1_np), _dev(c2_np)
            new = [_dev(lg), _dev(lg2)]
            static = _dev(lg).requires_grad_(True)
            static_plain = _dev(lg)
            out = batch.alloc_evaluate((M,))
            gout = torch.empty((M, 5), dtype=torch.float32, device="cuda")

            def autograd_body():
                r = batch.evaluate_actions(static, actions, masks)
                g, = torch.autograd.grad((c1 * r.logp + c2 * r.entropy).sum(), static)
                return r.logp.detach(), r.entropy.detach(), g

            def static_body():
                batch.evaluate_actions(static_plain, actions, masks, out=out)
                batch.evaluate_actions_backward(static_plain, actions, masks, c1, c2, out=gout)
                return out.logp, out.entropy, gout

            for body, inp in ((autograd_body, static), (static_body, static_plain)):
                body()                                                   # warm-up outside the capture
                side.synchronize()
                graph = torch.cuda.CUDAGraph()
                with torch.cuda.graph(graph, stream=side):
                    held = body()
                side.synchronize()
                for x, (fwd, bwd) in zip((new[1], new[0]), (specs[1], specs[0])):
                    with torch.no_grad():
                        inp.copy_(x)
                    graph.replay()
                    side.synchronize()
                    for got, w, name in zip(held, (fwd[0], fwd[1], bwd), ("logp", "entropy", "grad_logits")):
                        np.testing.assert_array_equal(bits32(got.cpu().numpy()), bits32(w), err_msg=f"{body.__name__}: {name}")
                del graph
    finally:
        batch.use_stream(None)
    assert not np.array_equal(bits32(specs[0][1]), bits32(specs[1][1]))


# ------------------------------------------------------------------------------------------------- 5. refusals
def test_refusals_leave_the_batch_usable(batch, reference):
    import torch

    from collectivecrossing_amd import EvalResult, _abi

    case, want = reference
    M = 65
    lg, ac, mk, glp, gent = _device_inputs(case, True, M)
    shifted = torch.empty(M * 5 + 1, dtype=torch.float32, device="cuda")[1:].view(M, 5)
    assert shifted.is_contiguous() and shifted.data_ptr() % 16
    good_out = batch.alloc_evaluate((M,))
    bad = [
        dict(logits=lg.double()), dict(logits=lg.half()), dict(logits=lg.bfloat16()), dict(logits=lg[:, :4].contiguous()),
        dict(logits=lg.reshape(M * 5)), dict(logits=lg.cpu()), dict(logits=lg.t().contiguous().t()), dict(logits=shifted),
        dict(logits=case["logits"][:M]),
        dict(actions=ac.long()), dict(actions=ac.to(torch.int32)), dict(actions=ac[:-1]), dict(actions=ac.cpu()),
        dict(actions=torch.empty(2 * M, dtype=torch.uint8, device="cuda")[::2]), dict(actions=ac.view(M, 1)),
        dict(masks=mk.to(torch.int32)), dict(masks=mk[:-1]), dict(masks=mk.cpu()),
        dict(out=(1, 2)), dict(out=EvalResult(good_out.logp[:-1], None)), dict(out=EvalResult(good_out.logp.double(), None)),
        dict(out=EvalResult(good_out.logp, good_out.entropy.view(M, 1))),
        dict(logits=lg.clone().requires_grad_(True), out=good_out),     # the autograd path allocates its outputs
    ]
    for kw in bad:
        with pytest.raises(ValueError):
            batch.evaluate_actions(**{**dict(logits=lg, actions=ac, masks=mk), **kw})
    bad_bwd = [
        dict(grad_logp=None, grad_entropy=None), dict(grad_logp=glp.double()), dict(grad_entropy=gent[:-1]),
        dict(grad_logp=glp.cpu()), dict(grad_logp=torch.empty(2 * M, device="cuda")[::2]), dict(out=shifted),
        dict(out=torch.empty((M, 4), device="cuda")), dict(out=torch.empty((M, 5), dtype=torch.float64, device="cuda")),
        dict(logits=shifted), dict(actions=ac.long()),
    ]
    for kw in bad_bwd:
        with pytest.raises(ValueError):
            batch.evaluate_actions_backward(**{**dict(logits=lg, actions=ac, masks=mk, grad_logp=glp, grad_entropy=gent), **kw})
    # zero rows: empty tensors, the library is not called
    empty = batch.evaluate_actions(lg[:0], ac[:0], mk[:0])
    assert empty.logp.shape == (0,) and empty.entropy.shape == (0,)
    assert batch.evaluate_actions_backward(lg[:0], ac[:0], mk[:0], glp[:0], None).shape == (0, 5)
    # the library's own refusals (the wrapper refuses first, so they are reached through the bindings)
    lib, h = batch._lib, batch._h
    grad = torch.empty((M, 5), dtype=torch.float32, device="cuda")
    p = dict(lg=lg.data_ptr(), ac=ac.data_ptr(), mk=mk.data_ptr(), lp=good_out.logp.data_ptr(), ent=good_out.entropy.data_ptr(),
             glp=glp.data_ptr(), gent=gent.data_ptr(), grad=grad.data_ptr())
    assert lib.ccx_evaluate_actions_backward(h, M, p["lg"], p["ac"], p["mk"], None, None, p["grad"]) == _abi.EINVAL
    assert "both gradients" in lib.ccx_last_error().decode()
    for args, word in (((None, M, p["lg"], p["ac"], p["mk"], p["lp"], p["ent"]), "NULL handle"),
                       ((h, M, None, p["ac"], p["mk"], p["lp"], p["ent"]), "NULL"),
                       ((h, M, p["lg"], None, p["mk"], p["lp"], p["ent"]), "NULL"),
                       ((h, M, p["lg"], p["ac"], p["mk"], None, p["ent"]), "NULL"),
                       ((h, 0, p["lg"], p["ac"], p["mk"], p["lp"], p["ent"]), "rows"),
                       ((h, (1 << 37) + 1, p["lg"], p["ac"], p["mk"], p["lp"], p["ent"]), "workgroups"),
                       ((h, M, shifted.data_ptr(), p["ac"], p["mk"], p["lp"], p["ent"]), "aligned")):
        assert lib.ccx_evaluate_actions(*args) == _abi.EINVAL
        assert word in lib.ccx_last_error().decode()
    for args, word in (((None, M, p["lg"], p["ac"], p["mk"], p["glp"], p["gent"], p["grad"]), "NULL handle"),
                       ((h, M, p["lg"], p["ac"], p["mk"], p["glp"], p["gent"], None), "NULL"),
                       ((h, -3, p["lg"], p["ac"], p["mk"], p["glp"], p["gent"], p["grad"]), "rows"),
                       ((h, (1 << 37) + 1, p["lg"], p["ac"], p["mk"], p["glp"], p["gent"], p["grad"]), "workgroups"),
                       ((h, M, p["lg"], p["ac"], p["mk"], p["glp"], p["gent"], shifted.data_ptr()), "aligned")):
        assert lib.ccx_evaluate_actions_backward(*args) == _abi.EINVAL
        assert word in lib.ccx_last_error().decode()
    r = batch.evaluate_actions(lg, ac, mk)
    batch.synchronize()
    np.testing.assert_array_equal(bits32(r.logp.cpu().numpy()), bits32(want[True][0][:M]), err_msg="after the refusals")
