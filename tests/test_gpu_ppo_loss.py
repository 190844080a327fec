"""The PPO loss on the device (include/ccx.h: CCX_PPO_LOSS) against the NumPy spec (tests/_ppo_loss_spec.py): bits of stats,
both gradients and the masked moments on row counts that cross every boundary of the kernels' layout and of the tree, every
output element written, the live sampling kernel against the live loss kernel, the autograd Function, other streams, graph
capture, static buffers and the refusals.  f32 values are compared as bit patterns throughout."""

import numpy as np
import pytest
from _ppo_loss_spec import (PPO_GRAD_LOGITS_NEAR_BOUND, PPO_GRAD_VALUES_BOUND, case_args, clean_case, make_ppo_case,
                            masked_moments_spec, ppo_loss_backward_spec, ppo_loss_spec, row_terms)
from _reset_obs_spec import make_config
from _sample_spec import bits32, make_sample_case

pytestmark = pytest.mark.gpu

# rows: the single-row tail, 5 M % 4 != 0, the wave / group (63, 64, 65) and block (255, 256, 257) boundaries, several blocks
# with a ragged tail (1023), and B = 65 > 64 blocks (16389), where a place of the final wave takes a second partial
ROWS = (1, 3, 63, 64, 65, 255, 256, 257, 1023, 16389)
LEADING = (3, 7, 5)
HYPER = dict(clip=0.2, vf_coef=0.5, ent_coef=0.01, adv_eps=1e-8)
NORM = np.array([7.0, 0.125, 0.75, 0.0], np.float32)                     # the [4] form: n, mean, std, 0
E, N = 8, 8


@pytest.fixture(scope="module")
def batch():
    import torch

    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    from collectivecrossing_amd.batched import BatchedCollectiveCrossing

    b = BatchedCollectiveCrossing(make_config(N, max_steps=12), E)
    yield b
    b.close()


@pytest.fixture(scope="module")
def case():
    return make_ppo_case(max(ROWS), seed=23, density=0.7)


def _dev(a):
    import torch

    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _dev_kw(kw, lead=None):
    out = {}
    for k, v in kw.items():
        t = _dev(v)
        if t is not None and lead is not None:
            t = t.view(lead + (5,)) if k == "logits" else t.view(lead)
        out[k] = t
    return out


def _live(kw):
    """valid for the moments: the rows that count for the loss (a row with action 255 may hold a NaN advantage)."""
    return ((kw["valid"] != 0) & (kw["actions"] != 255)).astype(np.uint8)


def _nan(shape):
    import torch

    return torch.full(shape, float("nan"), dtype=torch.float32, device="cuda")


def _variants(case, M):
    for masked in (True, False):
        for with_valid in (True, False):
            kw = case_args(case, masked, True, M) if with_valid else clean_case(case, masked, M)
            for norm in (NORM, None):
                yield f"M {M} masked {masked} valid {with_valid} norm {norm is not None}", kw, norm


def _check_bits(batch, case, M, lead=None):
    import torch

    lead = (M,) if lead is None else lead
    gloss_np = np.float32(-1.75)
    gloss = _dev(np.array([gloss_np]))
    for tag, kw, norm in _variants(case, M):
        d = _dev_kw(kw, lead)
        dn = _dev(norm)
        snorm = None if norm is None else norm[1:3]
        want = ppo_loss_spec(**kw, norm=snorm, **HYPER)
        out = batch.alloc_ppo_loss(lead)
        out.stats.fill_(float("nan"))
        r = batch.ppo_loss(**d, norm=dn, **HYPER, out=out)
        assert r is out
        np.testing.assert_array_equal(bits32(out.stats.cpu().numpy()), bits32(want), err_msg="stats " + tag)
        wl, wv = ppo_loss_backward_spec(**kw, norm=snorm, **HYPER, stats=want, grad_loss=gloss_np)
        for which in (3, 1, 2):
            buf = type(out)(out.loss, out.stats, None, _nan(lead + (5,)) if which & 1 else None, _nan(lead) if which & 2 else None)
            gl, gv = batch.ppo_loss_backward(**d, norm=dn, **HYPER, stats=out.stats, grad_loss=gloss, out=buf)
            assert gl is buf.grad_logits and gv is buf.grad_values
            if which & 1:
                np.testing.assert_array_equal(bits32(gl.cpu().numpy().reshape(M, 5)), bits32(wl), err_msg=f"grad_logits {which} " + tag)
            if which & 2:
                np.testing.assert_array_equal(bits32(gv.cpu().numpy().reshape(M)), bits32(wv), err_msg=f"grad_values {which} " + tag)
    # fresh outputs, the default arguments and grad_loss = None (1.0f)
    kw = case_args(case, True, True, M)
    d = _dev_kw(kw, lead)
    r = batch.ppo_loss(**d)
    want = ppo_loss_spec(**kw)
    gl, gv = batch.ppo_loss_backward(**d, stats=r.stats)
    wl, wv = ppo_loss_backward_spec(**kw, stats=want)
    np.testing.assert_array_equal(bits32(r.stats.cpu().numpy()), bits32(want))
    assert r.loss.dim() == 0 and r.loss.data_ptr() == r.stats.data_ptr() and gl.shape == lead + (5,) and gv.shape == lead
    assert float(r.count) == want[6] and bits32(np.float32(float(r.approx_kl))) == bits32(want[4])
    np.testing.assert_array_equal(bits32(gl.cpu().numpy().reshape(M, 5)), bits32(wl))
    np.testing.assert_array_equal(bits32(gv.cpu().numpy().reshape(M)), bits32(wv))
    assert batch.ppo_loss_backward(**d, stats=r.stats, want_logits_grad=False)[0] is None
    assert batch.ppo_loss_backward(**d, stats=r.stats, want_values_grad=False)[1] is None
    assert torch.isfinite(gl).all() and torch.isfinite(gv).all()          # no NaN of a row that does not count got through


# ------------------------------------------------------------------------------------------------- 1. bits against the spec
@pytest.mark.parametrize("M", ROWS)
def test_bits_against_the_spec_every_element_written(batch, case, M):
    _check_bits(batch, case, M)


def test_bits_with_a_leading_shape(batch, case):
    _check_bits(batch, case, int(np.prod(LEADING)), LEADING)


@pytest.mark.parametrize("M", ROWS)
def test_masked_moments_bits_and_the_square_root(batch, case, M):
    """The device takes the f64 square root; its bits equal IEEE sqrt on the host (np.sqrt in the spec), at every M, for
    three scales of the data: it is the correctly rounded one."""
    rng = np.random.default_rng(M)
    for scale, shift in ((1.0, 0.0), (0.003, 5.0), (300.0, -40.0)):
        x = (rng.standard_normal(M) * scale + shift).astype(np.float32)
        for valid in (None, case["valid"][:M].copy(), np.zeros(M, np.uint8)):
            xx = x.copy()
            if valid is not None:
                xx[valid == 0] = np.nan
            out = _nan((4,))
            got = batch.masked_moments(_dev(xx), _dev(valid), out=out)
            assert got is out
            np.testing.assert_array_equal(bits32(out.cpu().numpy()), bits32(masked_moments_spec(xx, valid)),
                                          err_msg=f"M {M} scale {scale} valid {valid is not None}")
    x3 = _dev(x).view(M, 1, 1)
    np.testing.assert_array_equal(bits32(batch.masked_moments(x3).cpu().numpy()), bits32(masked_moments_spec(x)))


def test_no_row_counts(batch, case):
    M = 300
    kw = case_args(case, True, True, M)
    kw["valid"] = np.zeros(M, np.uint8)
    d = _dev_kw(kw)
    out = batch.alloc_ppo_loss((M,))
    out.stats.fill_(float("nan"))
    out.grad_logits.fill_(float("nan"))
    out.grad_values.fill_(float("nan"))
    batch.ppo_loss(**d, out=out)
    batch.ppo_loss_backward(**d, stats=out.stats, grad_loss=_dev(np.array([np.nan], np.float32)), out=out)
    for t in (out.stats, out.grad_logits, out.grad_values):
        assert not bits32(t.cpu().numpy()).any()                         # +0.0f everywhere


# ------------------------------------------------------------------------------------------------- 2. kernel against kernel
def test_loss_on_the_sampling_kernels_own_logits(batch):
    import torch

    c = make_sample_case(E, N, seed=5)
    batch.set_state(terminated=c["terminated"], truncated=c["truncated"], step_count=c["step_count"], episode=c["episode"])
    batch.set_rng_seed(0x0123_4567_89AB_CDEF)
    rng = np.random.default_rng(8)
    adv, ret, val = (_dev(rng.standard_normal((E, N)).astype(np.float32)) for _ in range(3))
    for masked in (True, False):
        logits = _dev(c["logits_masked"] if masked else c["logits"])
        masks = _dev(c["masks"]) if masked else None
        s = batch.sample_actions(logits, masks, want_logp=True)
        valid = (s.actions != 255).to(torch.uint8)
        norm = batch.masked_moments(adv, valid)
        r = batch.ppo_loss(logits, val, s.actions, s.logp, adv, ret, masks=masks, valid=valid, norm=norm)
        st = r.stats.cpu().numpy()
        assert bits32(st)[4] == 0 and bits32(st)[5] == 0 and st[6] == int(valid.sum())      # approx_kl = clip_frac = +0.0f
        t = row_terms(logits.cpu().numpy().reshape(-1, 5), val.cpu().numpy().ravel(), s.actions.cpu().numpy().ravel(),
                      s.logp.cpu().numpy().ravel(), adv.cpu().numpy().ravel(), ret.cpu().numpy().ravel(),
                      None if masks is None else masks.cpu().numpy().ravel(), valid.cpu().numpy().ravel(), norm.cpu().numpy()[1:3])
        assert (t["ratio"][t["counts"]] == 1).all()
    batch.set_state(terminated=np.zeros((E, N), np.uint8), truncated=np.zeros((E, N), np.uint8))


# ------------------------------------------------------------------------------------------------- 3. autograd
AUTOGRAD_M = 2053                                                        # nine blocks; 5 M % 4 == 1


def _torch_composition(d, norm, hyper, dtype):
    """The loss as a user writes it with torch alone (boolean indexing and all), in `dtype`, and its two gradients."""
    import torch

    from collectivecrossing_amd import unpack_action_masks

    keep = (d["valid"] != 0) & (d["actions"] != 255)
    x = torch.nan_to_num(d["logits"][keep]).to(dtype).requires_grad_(True)
    v = d["values"][keep].to(dtype).requires_grad_(True)
    legal = unpack_action_masks(d["masks"][keep] | 0x10)
    lp = torch.log_softmax(x.masked_fill(~legal, -torch.inf), -1)
    p = lp.exp()
    zero = torch.zeros_like(lp)
    H = -torch.where(p > 0, p * torch.where(p > 0, lp, zero), zero).sum(-1)
    logp = lp.gather(-1, d["actions"][keep].long()[:, None])[:, 0]
    ratio = (logp - d["logp_old"][keep].to(dtype)).exp()
    an = (d["advantages"][keep].to(dtype) - norm[1].to(dtype)) / (norm[2].to(dtype) + hyper["adv_eps"])
    lo, hi = float(np.float32(1) - np.float32(hyper["clip"])), float(np.float32(1) + np.float32(hyper["clip"]))
    surr = torch.minimum(ratio * an, ratio.clamp(lo, hi) * an)
    loss = -surr.mean() + hyper["vf_coef"] * ((v - d["returns"][keep].to(dtype)) ** 2).mean() - hyper["ent_coef"] * H.mean()
    gx, gv = torch.autograd.grad(loss, (x, v))
    return loss.detach(), gx, gv, keep


def test_autograd_equals_the_backward_entry_point_and_torchs_composition(batch, case):
    import torch

    M = AUTOGRAD_M
    kw = case_args(case, True, True, M)
    d = _dev_kw(kw)
    norm = batch.masked_moments(d["advantages"], _dev(_live(kw)))
    logits = d["logits"].clone().requires_grad_(True)
    values = d["values"].clone().requires_grad_(True)
    args = {**d, "logits": logits, "values": values}
    r = batch.ppo_loss(**args, norm=norm, **HYPER)
    assert r.loss.requires_grad and r.loss.dim() == 0 and not r.stats.requires_grad
    r.loss.backward()
    plain = batch.ppo_loss(**d, norm=norm, **HYPER)
    assert plain.loss.grad_fn is None and torch.equal(plain.stats, r.stats)
    gl, gv = batch.ppo_loss_backward(**d, norm=norm, **HYPER, stats=plain.stats)
    np.testing.assert_array_equal(bits32(logits.grad.cpu().numpy()), bits32(gl.cpu().numpy()))
    np.testing.assert_array_equal(bits32(values.grad.cpu().numpy()), bits32(gv.cpu().numpy()))
    nn = norm.cpu().numpy()
    np.testing.assert_array_equal(bits32(nn), bits32(masked_moments_spec(kw["advantages"], _live(kw))))
    assert np.isfinite(nn).all() and np.isfinite(r.stats.cpu().numpy()).all()
    want = ppo_loss_spec(**kw, norm=nn[1:3], **HYPER)
    wl, wv = ppo_loss_backward_spec(**kw, norm=nn[1:3], **HYPER, stats=want)
    np.testing.assert_array_equal(bits32(r.stats.cpu().numpy()), bits32(want))
    np.testing.assert_array_equal(bits32(gl.cpu().numpy()), bits32(wl))
    np.testing.assert_array_equal(bits32(gv.cpu().numpy()), bits32(wv))
    # a scaled loss: the incoming gradient reaches the kernel as grad_loss
    logits.grad = values.grad = None
    (batch.ppo_loss(**args, norm=norm, **HYPER).loss * 3.0).backward()
    w3 = ppo_loss_backward_spec(**kw, norm=nn[1:3], **HYPER, stats=want, grad_loss=3.0)
    np.testing.assert_array_equal(bits32(logits.grad.cpu().numpy()), bits32(w3[0]))
    np.testing.assert_array_equal(bits32(values.grad.cpu().numpy()), bits32(w3[1]))
    # only one of the two requires grad: None goes to the other
    for which in ("logits", "values"):
        a2 = {**d, which: d[which].clone().requires_grad_(True)}
        r2 = batch.ppo_loss(**a2, norm=norm, **HYPER)
        r2.loss.backward()
        np.testing.assert_array_equal(bits32(a2[which].grad.cpu().numpy()), bits32((wl if which == "logits" else wv)))
        other = "values" if which == "logits" else "logits"
        assert a2[other].grad is None and not a2[other].requires_grad
    with torch.no_grad():
        quiet = batch.ppo_loss(**args, norm=norm, **HYPER)
    assert quiet.loss.grad_fn is None and torch.equal(quiet.stats, r.stats)

    # against torch's own composition on well-conditioned rows: class "plain" (logits ~ N(0, 3)), not degenerate, |x| <= 80,
    # logp >= -10 and the ratio away from the clip edges.  Against f64 the bound is the rule's own measured one
    # (tests/test_ppo_loss_spec.py).  torch's f32 composition is allowed, on top of that, 2 ulp of a logp of size up to 10
    # (2 x 2^-20: exp turns an absolute error of logp - logp_old into a relative one of the ratio and so of the row's
    # gradient) and 16 further f32 roundings (exp, the products, the clamp's branch, two means and their backward).
    t = row_terms(**kw, norm=nn[1:3], clip=0.2, adv_eps=1e-8)
    lo, hi = np.float32(0.8), np.float32(1.2)
    lg = np.where(((((kw["masks"] & 0x1F) | 0x10)[:, None] >> np.arange(5, dtype=np.uint8)) & 1).astype(bool), kw["logits"], -np.inf)
    with np.errstate(invalid="ignore"):
        ok = (t["counts"] & (np.abs(t["x"]) <= 80) & (t["logp"] >= -10) & (np.abs(t["ratio"] - lo) > 1e-5) & (np.abs(t["ratio"] - hi) > 1e-5)
              & ~(np.isnan(lg).any(-1) | (lg == np.inf).any(-1) | (lg.max(-1) == -np.inf)) & (case["classes"][:M] <= 2))
    sel = dict(d, valid=_dev(ok.astype(np.uint8)))
    r3 = batch.ppo_loss(**sel, norm=norm, **HYPER)
    g3l, g3v = batch.ppo_loss_backward(**sel, norm=norm, **HYPER, stats=r3.stats)
    n = float(r3.count)
    assert n == ok.sum() and n > 200
    for dtype, extra in ((torch.float64, 0.0), (torch.float32, 2 * 2.0 ** -20 + 16 * 2.0 ** -24)):
        loss, gx, gvv, keep = _torch_composition(sel, norm, HYPER, dtype)
        ours_l = g3l[keep].double().cpu().numpy() * n
        ref_l = gx.double().cpu().numpy() * n
        err_l = float((np.abs(ours_l - ref_l) / np.maximum(1.0, np.abs(ref_l))).max())
        ours_v, ref_v = g3v[keep].double().cpu().numpy() * n, gvv.double().cpu().numpy() * n
        err_v = float((np.abs(ours_v - ref_v) / np.maximum(1.0, np.abs(ref_v))).max())
        print(f"against torch {dtype}: n * grad_logits {err_l:.3e}, n * grad_values {err_v:.3e}, loss {abs(float(loss) - float(r3.loss)):.3e}")
        assert err_l <= PPO_GRAD_LOGITS_NEAR_BOUND + extra and err_v <= PPO_GRAD_VALUES_BOUND + extra


# ------------------------------------------------------------------------------------------------- 3b. the frame of the loss
FRAME_ROWS = (1, 63, 257, 513)                                           # inside a wave, across one, a block + a row, two + a row


@pytest.mark.parametrize("present", (False, True), ids=("optional-absent", "optional-present"))
@pytest.mark.parametrize("M", FRAME_ROWS)
def test_the_three_call_forms_agree(batch, case, M, present):
    """Fresh outputs, ``out=`` of ``alloc_ppo_loss`` and autograd write the spec's stats, so the same bits; the gradients that
    ``r.loss.backward()`` leaves are ``ppo_loss_backward(out=)``'s with ``grad_loss`` absent and with a 1.0f."""
    import torch

    kw = case_args(case, True, True, M) if present else clean_case(case, False, M)
    norm = NORM if present else None
    d, dn = _dev_kw(kw), _dev(norm)
    want = ppo_loss_spec(**kw, norm=None if norm is None else norm[1:3], **HYPER)
    wl, wv = ppo_loss_backward_spec(**kw, norm=None if norm is None else norm[1:3], **HYPER, stats=want)
    fresh = batch.ppo_loss(**d, norm=dn, **HYPER)
    static = batch.alloc_ppo_loss((M,))
    for t in (static.stats, static.grad_logits, static.grad_values):
        t.fill_(float("nan"))
    assert batch.ppo_loss(**d, norm=dn, **HYPER, out=static) is static
    logits, values = d["logits"].clone().requires_grad_(), d["values"].clone().requires_grad_()
    auto = batch.ppo_loss(**{**d, "logits": logits, "values": values}, norm=dn, **HYPER)
    auto.loss.backward()
    gl0, gv0 = batch.ppo_loss_backward(**d, norm=dn, **HYPER, stats=static.stats, out=static)
    gl0, gv0 = gl0.clone(), gv0.clone()
    gl1, gv1 = batch.ppo_loss_backward(**d, norm=dn, **HYPER, stats=static.stats, grad_loss=torch.ones(1, device="cuda"), out=static)
    batch.synchronize()
    assert fresh.workspace is None and auto.workspace is None and gl1 is static.grad_logits and gv1 is static.grad_values
    for form, r in (("fresh", fresh), ("out=", static), ("autograd", auto)):
        np.testing.assert_array_equal(bits32(r.stats.cpu().numpy()), bits32(want), err_msg="stats " + form)
    for form, gl, gv in (("autograd", logits.grad, values.grad), ("grad_loss None", gl0, gv0), ("grad_loss 1.0f", gl1, gv1)):
        np.testing.assert_array_equal(bits32(gl.cpu().numpy()), bits32(wl), err_msg="grad_logits " + form)
        np.testing.assert_array_equal(bits32(gv.cpu().numpy()), bits32(wv), err_msg="grad_values " + form)


def test_zero_rows_in_the_three_call_forms(batch, case, monkeypatch):
    import torch

    d = {k: v[:0] for k, v in _dev_kw(case_args(case, True, True, 4)).items()}
    static = batch.alloc_ppo_loss((0,))
    static.stats.fill_(float("nan"))

    def called(*args, **kwargs):
        raise AssertionError("zero rows must not reach the library")

    monkeypatch.setattr(batch, "_enqueue", called)
    fresh = batch.ppo_loss(**d)
    assert batch.ppo_loss(**d, out=static) is static
    logits, values = d["logits"].clone().requires_grad_(), d["values"].clone().requires_grad_()
    auto = batch.ppo_loss(**{**d, "logits": logits, "values": values})
    assert auto.loss.requires_grad and not auto.stats.requires_grad
    auto.loss.backward()
    for r in (fresh, static, auto):
        assert r.stats.shape == (8,) and not r.stats.view(torch.int32).any()
    assert logits.grad.shape == (0, 5) and values.grad.shape == (0,)
    gl, gv = batch.ppo_loss_backward(**d, stats=static.stats, out=static)
    assert gl is static.grad_logits and gv is static.grad_values


# ------------------------------------------------------------------------------------------------- 4. streams and capture
def test_another_current_stream(batch, case):
    """torch's current stream is not the handle's stream, and a blocker (tests/_stream_order.py) keeps one of the two
    busy: first the current one, so the launches must wait for inputs produced behind it; then the handle's, so the torch
    ops that consume the results at once must wait for the launches."""
    import torch
    from _stream_order import Blocker

    M = 257
    kw = case_args(case, True, True, M)
    d = _dev_kw(kw)
    live = _dev(_live(kw))
    nn = masked_moments_spec(kw["advantages"], _live(kw))
    want = ppo_loss_spec(**kw, norm=nn[1:3], **HYPER)
    assert np.isfinite(want).all()
    wl, wv = ppo_loss_backward_spec(**kw, norm=nn[1:3], **HYPER, stats=want)
    blocker = Blocker()
    handle = batch._stream                                               # (where the batch launches)
    other = torch.cuda.Stream()
    blocker.warm(other, handle)
    for busy in (None, other, handle):                                   # (None: once without a blocker, the one-off host work)
        torch.cuda.synchronize()
        with torch.cuda.stream(other):                                   # torch's current stream is not the handle's stream
            ev = None if busy is None else blocker.run(busy)
            logits = (d["logits"] * 1.0).requires_grad_(True)            # produced on `other`
            values = (d["values"] * 1.0).requires_grad_(True)
            norm = batch.masked_moments(d["advantages"] * 1.0, live)
            r = batch.ppo_loss(**{**d, "logits": logits, "values": values}, norm=norm, **HYPER)
            r.loss.backward()
            early = [t.detach().clone() for t in (norm, r.stats, logits.grad, values.grad)]   # consumers, at once, on `other`
            still_running = ev is None or not ev.query()
            got = [t.cpu().numpy() for t in early]
        assert still_running, "blocker too short: it had ended before the consumers were enqueued"
        for g, w in zip(got, (nn, want, wl, wv)):
            np.testing.assert_array_equal(bits32(g), bits32(w))


def test_captured_forward_and_backward_and_static_buffers(batch, case):
    import torch

    M = 1023
    kw = case_args(case, True, True, M)
    kw2 = case_args(make_ppo_case(M, seed=77, density=0.5), True, True, M)
    specs = []
    for k in (kw, kw2):
        nn = masked_moments_spec(k["advantages"], _live(k))
        st = ppo_loss_spec(**k, norm=nn[1:3], **HYPER)
        assert np.isfinite(st).all()
        specs.append((nn, st) + ppo_loss_backward_spec(**k, norm=nn[1:3], **HYPER, stats=st))
    side = torch.cuda.Stream()
    batch.use_stream(side)
    torch.cuda.synchronize()
    try:
        with torch.cuda.stream(side):
            new = [dict(_dev_kw(k), live=_dev(_live(k))) for k in (kw, kw2)]
            static = {k: v.clone() for k, v in new[0].items()}
            live = static.pop("live")
            auto = {**static, "logits": static["logits"].clone().requires_grad_(True),
                    "values": static["values"].clone().requires_grad_(True)}
            out = batch.alloc_ppo_loss((M,))
            norm_out = torch.empty(4, dtype=torch.float32, device="cuda")

            def autograd_body():
                norm = batch.masked_moments(auto["advantages"], live)
                r = batch.ppo_loss(**auto, norm=norm, **HYPER)
                gl, gv = torch.autograd.grad(r.loss, (auto["logits"], auto["values"]))
                return norm, r.stats, gl, gv

            def static_body():
                batch.masked_moments(static["advantages"], live, out=norm_out, workspace=out.workspace)
                batch.ppo_loss(**static, norm=norm_out, **HYPER, out=out)
                batch.ppo_loss_backward(**static, norm=norm_out, **HYPER, stats=out.stats, out=out)
                return norm_out, out.stats, out.grad_logits, out.grad_values

            for body, inp in ((autograd_body, auto), (static_body, static)):
                body()                                                   # warm-up outside the capture
                side.synchronize()
                graph = torch.cuda.CUDAGraph()
                with torch.cuda.graph(graph, stream=side):
                    held = body()
                side.synchronize()
                for x, spec in zip((new[1], new[0]), (specs[1], specs[0])):
                    with torch.no_grad():
                        for k, v in x.items():
                            (live if k == "live" else inp[k]).copy_(v)
                    graph.replay()
                    side.synchronize()
                    for got, w, name in zip(held, spec, ("moments", "stats", "grad_logits", "grad_values")):
                        np.testing.assert_array_equal(bits32(got.cpu().numpy()), bits32(w), err_msg=f"{body.__name__}: {name}")
                del graph
    finally:
        batch.use_stream(None)
    assert not np.array_equal(bits32(specs[0][1]), bits32(specs[1][1]))


# ------------------------------------------------------------------------------------------------- 5. refusals
def test_refusals_leave_the_batch_usable(batch, case):
    import torch

    from collectivecrossing_amd import _abi

    M = 65
    kw = case_args(case, True, True, M)
    d = _dev_kw(kw)
    shifted = torch.empty(M * 5 + 1, dtype=torch.float32, device="cuda")[1:].view(M, 5)
    assert shifted.is_contiguous() and shifted.data_ptr() % 16
    good = batch.alloc_ppo_loss((M,))
    bad = [
        dict(logits=d["logits"].double()), dict(logits=d["logits"].half()), dict(logits=d["logits"][:, :4].contiguous()),
        dict(logits=d["logits"].cpu()), dict(logits=d["logits"].t().contiguous().t()), dict(logits=shifted), dict(logits=kw["logits"]),
        dict(values=d["values"].double()), dict(values=d["values"][:-1]), dict(values=d["values"].cpu()),
        dict(values=torch.empty(2 * M, device="cuda")[::2]), dict(actions=d["actions"].long()), dict(actions=d["actions"][:-1]),
        dict(logp_old=d["logp_old"].double()), dict(logp_old=d["logp_old"].view(M, 1)), dict(advantages=d["advantages"][:-1]),
        dict(returns=d["returns"].cpu()), dict(masks=d["masks"].to(torch.int32)), dict(valid=d["valid"].bool()),
        dict(valid=d["valid"][:-1]), dict(norm=torch.zeros(3, device="cuda")), dict(norm=torch.zeros(4, dtype=torch.float64, device="cuda")),
        dict(norm=torch.zeros(4)), dict(norm=[0.0, 1.0]),
        dict(clip=0.0), dict(clip=1.0), dict(clip=-0.1), dict(clip=float("nan")), dict(clip=float("inf")), dict(vf_coef=-1.0),
        dict(vf_coef=float("inf")), dict(ent_coef=float("nan")), dict(ent_coef=-0.5), dict(adv_eps=-1e-8), dict(adv_eps=float("inf")),
        dict(out=(1, 2)), dict(out=type(good)(good.loss, good.stats[:4])), dict(out=type(good)(good.loss, good.stats, good.workspace[:8])),
        dict(logits=d["logits"].clone().requires_grad_(True), out=good),  # the autograd path allocates its outputs
        dict(values=d["values"].clone().requires_grad_(True), out=good),
    ]
    for extra in bad:
        with pytest.raises(ValueError):
            batch.ppo_loss(**{**d, **HYPER, **extra})
    stats = batch.ppo_loss(**d, **HYPER).stats
    bad_bwd = [
        dict(stats=stats[:4]), dict(stats=stats.double()), dict(stats=stats.cpu()), dict(grad_loss=torch.ones(1)),
        dict(grad_loss=torch.ones(1, dtype=torch.float64, device="cuda")), dict(grad_loss=torch.ones((1, 1), device="cuda")),
        dict(want_logits_grad=False, want_values_grad=False), dict(out=type(good)(good.loss, good.stats)),
        dict(out=type(good)(good.loss, good.stats, None, shifted, None)),
        dict(out=type(good)(good.loss, good.stats, None, None, torch.empty(M + 1, device="cuda"))),
        dict(logits=shifted), dict(clip=2.0), dict(actions=d["actions"].long()),
    ]
    for extra in bad_bwd:
        with pytest.raises(ValueError):
            batch.ppo_loss_backward(**{**d, **HYPER, "stats": stats, **extra})
    for extra in (dict(x=d["advantages"].double()), dict(x=d["advantages"].cpu()), dict(valid=d["valid"][:-1]),
                  dict(valid=d["valid"].bool()), dict(out=torch.empty(3, device="cuda")), dict(workspace=torch.empty(4, dtype=torch.uint8, device="cuda")),
                  dict(x=torch.empty(2 * M, device="cuda")[::2])):
        with pytest.raises(ValueError):
            batch.masked_moments(**{**dict(x=d["advantages"], valid=d["valid"]), **extra})
    # zero rows: zeros, the library is not called
    empty = {k: v[:0] for k, v in d.items()}
    z = batch.ppo_loss(**empty)
    assert not bits32(z.stats.cpu().numpy()).any()
    gl, gv = batch.ppo_loss_backward(**empty, stats=z.stats)
    assert gl.shape == (0, 5) and gv.shape == (0,)
    np.testing.assert_array_equal(batch.masked_moments(d["advantages"][:0]).cpu().numpy(), np.array([0, 0, 1, 0], np.float32))
    # the library's own refusals (the wrapper refuses first, so they are reached through the bindings)
    lib, h = batch._lib, batch._h
    assert lib.ccx_ppo_workspace_bytes(0) == 0 and lib.ccx_ppo_workspace_bytes(1) == 48 and lib.ccx_ppo_workspace_bytes(257) == 96
    p = {k: v.data_ptr() for k, v in d.items()}
    ws, st, gl_p, gv_p = good.workspace.data_ptr(), good.stats.data_ptr(), good.grad_logits.data_ptr(), good.grad_values.data_ptr()

    def fwd(**kw_):
        a = dict(h=h, rows=M, logits=p["logits"], actions=p["actions"], masks=p["masks"], logp_old=p["logp_old"],
                 advantages=p["advantages"], returns=p["returns"], values=p["values"], valid=p["valid"], norm=None, clip=0.2,
                 vf_coef=0.5, ent_coef=0.01, adv_eps=1e-8, workspace=ws, stats=st)
        a.update(kw_)
        return lib.ccx_ppo_loss(*a.values())

    def bwd(**kw_):
        a = dict(h=h, rows=M, logits=p["logits"], actions=p["actions"], masks=p["masks"], logp_old=p["logp_old"],
                 advantages=p["advantages"], returns=p["returns"], values=p["values"], valid=p["valid"], norm=None, clip=0.2,
                 vf_coef=0.5, ent_coef=0.01, adv_eps=1e-8, stats=st, grad_loss=None, grad_logits=gl_p, grad_values=gv_p)
        a.update(kw_)
        return lib.ccx_ppo_loss_backward(*a.values())

    for call, kw_, word in ((fwd, dict(h=None), "NULL handle"), (fwd, dict(logits=None), "NULL"), (fwd, dict(values=None), "NULL"),
                            (fwd, dict(workspace=None), "NULL"), (fwd, dict(stats=None), "NULL"), (fwd, dict(rows=0), "rows"),
                            (fwd, dict(logits=shifted.data_ptr()), "aligned"), (fwd, dict(workspace=ws + 4), "aligned"),
                            (fwd, dict(clip=0.0), "clip"), (fwd, dict(clip=1.0), "clip"), (fwd, dict(clip=float("nan")), "clip"),
                            (fwd, dict(vf_coef=-1.0), "vf_coef"), (fwd, dict(ent_coef=float("inf")), "ent_coef"),
                            (fwd, dict(adv_eps=float("nan")), "adv_eps"),
                            (bwd, dict(h=None), "NULL handle"), (bwd, dict(stats=None), "NULL"), (bwd, dict(rows=-2), "rows"),
                            (bwd, dict(grad_logits=None, grad_values=None), "both gradient"),
                            (bwd, dict(grad_logits=shifted.data_ptr()), "aligned"), (bwd, dict(clip=1.5), "clip"),
                            (bwd, dict(rows=(1 << 37) + 1), "workgroups")):
        assert call(**kw_) == _abi.EINVAL, (call.__name__, kw_)
        assert word in lib.ccx_last_error().decode(), (kw_, lib.ccx_last_error().decode())
    xs = p["advantages"]
    for args, word in (((None, M, xs, None, ws, st), "NULL handle"), ((h, M, None, None, ws, st), "NULL"),
                       ((h, M, xs, None, None, st), "NULL"), ((h, 0, xs, None, ws, st), "rows"), ((h, M, xs, None, ws + 4, st), "aligned")):
        assert lib.ccx_masked_moments(*args) == _abi.EINVAL
        assert word in lib.ccx_last_error().decode()
    r = batch.ppo_loss(**d, **HYPER)
    np.testing.assert_array_equal(bits32(r.stats.cpu().numpy()), bits32(ppo_loss_spec(**kw, **HYPER)), err_msg="after the refusals")
