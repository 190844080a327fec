"""The wide perceptron on the device (include/ccx.h: CCX_MLP_WIDE) against CCX_MLP's rule: y and hidden, the four parameter
gradients and grad_a bit for bit on every shape class of tests/_mlp_wide_shape_classes.py and on row counts that cross every
boundary of the kernels' layout; the wide entry points against the narrow ones for O <= 8, kernel against kernel; row
independence; the Python layer (autograd in both modes, graph capture, conversions, checkpoints, zero rows, refusals); the
example.  The reference is the rule of csrc/ccx_mlp_wide.h compiled for the host, which tests/test_mlp_wide_host_rule.py
shows equal to the NumPy specs; at the customary head the NumPy specs themselves.  f32 values are compared as bit patterns
throughout (tests/_mlp_spec.bits32c: a NaN's sign and payload are the one thing the rule leaves open)."""

import io
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
from _mlp_backward_spec import NAMES, make_mlp_backward_case, mlp_backward_spec
from _mlp_spec import RELU, TANH, bits32, bits32c, make_mlp_case, mlp_spec
from _mlp_wide_host_rule import compiler, host_backward, host_forward, load
from _mlp_wide_shape_classes import CATALOGUE, FORWARD_ROWS, NARROW, backward_rows
from _reset_obs_spec import make_config

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
ACT = {TANH: "tanh", RELU: "relu"}
# beside the catalogue: the smallest and the largest O, the narrow head's limit and the first O beyond it, an O that is no
# multiple of 4 at every H of the issue's list, L = 255 / 256 / 512 beside a wide O
EXTRA = ((38, 64, 1, TANH), (38, 64, 8, RELU), (38, 64, 9, TANH), (7, 16, 319, RELU), (7, 64, 320, TANH), (7, 256, 319, TANH),
         (255, 64, 255, RELU), (256, 64, 255, TANH), (512, 64, 319, RELU), (7, 16, 320, TANH))
FORWARD = tuple(s.dims for s in CATALOGUE) + EXTRA


@pytest.fixture(scope="module")
def batch():
    import torch

    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    from collectivecrossing_amd.batched import BatchedCollectiveCrossing

    b = BatchedCollectiveCrossing(make_config(8, max_steps=12), 16)
    yield b
    b.close()


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    cxx = compiler()
    assert cxx is not None, "the reference needs a host C++ compiler"
    return load(cxx, tmp_path_factory.mktemp("gpu_mlp_wide"))


def _head(batch, c, L, H, O, act, **kw):
    import torch

    from collectivecrossing_amd import WideMlpHead

    head = WideMlpHead(batch, H, O, ACT[act], L=L, **kw)
    with torch.no_grad():
        for name in ("w1t", "b1", "w2", "b2"):
            getattr(head, name).copy_(torch.from_numpy(c[name]))
    return head


def _dev(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _poisoned(shape):
    import torch

    t = torch.empty(shape, dtype=torch.float32, device="cuda")
    t.view(torch.uint8).fill_(0xEE)
    return t


# ------------------------------------------------------------------------------------------------- 1. the forward
@pytest.mark.parametrize("L,H,O,act", FORWARD)
def test_y_and_hidden_equal_the_rule(batch, host, L, H, O, act):
    import torch

    c = make_mlp_case(max(FORWARD_ROWS), L, H, O, seed=L * 7 + H + O)
    want_y, want_h = host_forward(host, c["x"], c["w1t"], c["b1"], c["w2"], c["b2"], act)
    if (L, H, O) == (38, 64, 255):                                        # the customary head: the NumPy spec itself
        spec_y, spec_h = mlp_spec(c["x"], c["w1t"], c["b1"], c["w2"], c["b2"], act)
        np.testing.assert_array_equal(bits32c(want_y), bits32c(spec_y))
        np.testing.assert_array_equal(bits32c(want_h), bits32c(spec_h))
    head = _head(batch, c, L, H, O, act)
    x_all = _dev(c["x"])
    for rows in FORWARD_ROWS:
        x = x_all[:rows].clone()
        y, hid = _poisoned((rows, O)), _poisoned((rows, H))
        torch.cuda.synchronize()
        with torch.no_grad():
            got = head(x, out=y, hidden_out=hid)
            plain = head(x)
        batch.synchronize()
        assert got.data_ptr() == y.data_ptr()
        np.testing.assert_array_equal(bits32c(y.cpu().numpy()), bits32c(want_y[:rows]), err_msg=f"y, {rows} rows")
        np.testing.assert_array_equal(bits32c(hid.cpu().numpy()), bits32c(want_h[:rows]), err_msg=f"hidden, {rows} rows")
        np.testing.assert_array_equal(bits32(plain.cpu().numpy()), bits32(y.cpu().numpy()), err_msg=f"head(x), {rows} rows")
    assert np.isnan(want_y).any() and np.isfinite(want_y).any()


# ------------------------------------------------------------------------------------------------- 2. the backward
def _check_backward(batch, host, c, L, H, O, act, rows_list, spec=False):
    import torch

    head = _head(batch, c, L, H, O, act)
    xa, ha, ga_ = _dev(c["x"]), _dev(c["hidden"]), _dev(c["grad_y"])
    for rows in rows_list:
        want = host_backward(host, c["x"][:rows], c["hidden"][:rows], c["grad_y"][:rows], c["w2"], act)
        if spec:
            numpy_spec = mlp_backward_spec(c["x"][:rows], c["hidden"][:rows], c["grad_y"][:rows], c["w2"], act)
            for name in NAMES + ("ga",):
                np.testing.assert_array_equal(bits32c(want[name]), bits32c(numpy_spec[name]), err_msg=name)
        x, hid, gy = xa[:rows].clone(), ha[:rows].clone(), ga_[:rows].clone()
        out = head.alloc_param_grads((rows,), want_grad_a=True)
        for t in (out.w1t, out.b1, out.w2, out.b2, out.grad_a):
            t.view(torch.uint8).fill_(0xEE)
        torch.cuda.synchronize()
        got = head.param_grads(x, hid, gy, out=out)
        fresh = head.param_grads(x, hid, gy)                              # its own outputs and workspace, no grad_a
        batch.synchronize()
        assert got is out and fresh.grad_a is None
        for name in NAMES:
            np.testing.assert_array_equal(bits32c(getattr(out, name).cpu().numpy()), bits32c(want[name]), err_msg=f"{name}, {rows} rows")
            np.testing.assert_array_equal(bits32c(getattr(fresh, name).cpu().numpy()), bits32c(want[name]), err_msg=f"{name}, {rows} rows")
        np.testing.assert_array_equal(bits32c(out.grad_a.cpu().numpy()), bits32c(want["ga"]), err_msg=f"grad_a, {rows} rows")


@pytest.mark.parametrize("s", CATALOGUE, ids=lambda s: f"{s.L}-{s.H}-{s.O}")
def test_gradients_equal_the_rule(batch, host, s):
    rows_list = sorted(set(backward_rows(s.rows1)) | set(backward_rows(s.rows2)))
    c = make_mlp_backward_case(max(rows_list), s.L, s.H, s.O, s.act, seed=s.L + s.H + s.O)
    _check_backward(batch, host, c, s.L, s.H, s.O, s.act, rows_list, spec=False)


def test_gradients_equal_the_numpy_spec_at_the_customary_head(batch, host):
    c = make_mlp_backward_case(257, 38, 64, 255, TANH, seed=51)
    _check_backward(batch, host, c, 38, 64, 255, TANH, (257,), spec=True)


def test_gradients_over_more_than_64_blocks(batch, host):
    """16 385 rows are 65 blocks: the final step's places take a second partial."""
    L, H, O, rows = 7, 16, 9, 16385
    c = make_mlp_backward_case(rows, L, H, O, RELU, seed=3)
    _check_backward(batch, host, c, L, H, O, RELU, (rows,))


# ------------------------------------------------------------------------------------------------- 3. kernel against kernel
@pytest.mark.parametrize("L,H,O,act", NARROW)
def test_wide_entry_points_give_the_narrow_ones_bits(batch, L, H, O, act):
    import torch

    rows = 300 if L < 100 else 70
    c = make_mlp_backward_case(rows, L, H, O, act, seed=L + O)
    adv = make_mlp_case(rows, L, H, O, seed=L + O)                        # rows with NaN and infinities for the forward
    lib = batch._lib
    f = torch.float32
    p = [_dev(c[k]) for k in ("w1t", "b1", "w2", "b2")]
    x = _dev(adv["x"])
    outs = {}
    for name, fn in (("narrow", lib.ccx_mlp_forward), ("wide", lib.ccx_mlp_wide_forward)):
        y, hid = _poisoned((rows, O)), _poisoned((rows, H))
        batch._enqueue(fn, rows, L, H, O, act, x, *p, y, hid)
        outs[name] = (y, hid)
    batch.synchronize()
    for a, b in zip(outs["narrow"], outs["wide"]):
        np.testing.assert_array_equal(bits32c(a.cpu().numpy()), bits32c(b.cpu().numpy()))
    assert np.isnan(outs["wide"][0].cpu().numpy()).any()
    xb, hb, gy = _dev(c["x"]), _dev(c["hidden"]), _dev(c["grad_y"])
    assert lib.ccx_mlp_wide_backward_workspace_bytes(rows, L, H, O) == lib.ccx_mlp_backward_workspace_bytes(rows, L, H, O) > 0
    ws = torch.empty(lib.ccx_mlp_backward_workspace_bytes(rows, L, H, O), dtype=torch.uint8, device="cuda")
    grads = {}
    for name, fn in (("narrow", lib.ccx_mlp_backward), ("wide", lib.ccx_mlp_wide_backward)):
        g = [_poisoned(s) for s in ((L, H), (H,), (O, H), (O,), (rows, H))]
        ws.fill_(0xEE)
        batch._enqueue(fn, rows, L, H, O, act, xb, hb, gy, p[2], ws, *g)
        grads[name] = g
    batch.synchronize()
    for a, b in zip(grads["narrow"], grads["wide"]):
        np.testing.assert_array_equal(bits32(a.cpu().numpy()), bits32(b.cpu().numpy()))
        assert np.isfinite(a.cpu().numpy()).all() and f is a.dtype


# ------------------------------------------------------------------------------------------------- 4. row independence
def test_rows_do_not_depend_on_their_number_or_place(batch):
    import torch

    L, H, O = 38, 64, 255
    c = make_mlp_case(4 * 16 * 8, L, H, O, seed=17, adversarial=False)
    head = _head(batch, c, L, H, O, TANH, out_shape=(5, 51))
    x = _dev(c["x"]).view(4, 16, 8, L)
    perm = torch.randperm(512, generator=torch.Generator().manual_seed(5)).cuda()
    with torch.no_grad():
        whole = head(x)
        assert tuple(whole.shape) == (4, 16, 8, 5, 51)
        flat = whole.reshape(512, O)
        for cuts in ((1, 511), (63, 65, 384), (256, 256), (129, 383)):
            parts, at = [], 0
            for n in cuts:
                parts.append(head(x.view(512, L)[at:at + n].clone()).reshape(n, O))
                at += n
            assert torch.equal(torch.cat(parts).view(torch.int32), flat.view(torch.int32)), cuts
        shuffled = head(x.view(512, L)[perm].contiguous()).reshape(512, O)
        back = torch.empty_like(shuffled)
        back[perm] = shuffled
        assert torch.equal(back.view(torch.int32), flat.view(torch.int32))
    batch.synchronize()


# ------------------------------------------------------------------------------------------------- 5. the Python layer
@pytest.mark.parametrize("act", ("tanh", "relu"))
def test_autograd_in_both_modes(batch, act):
    """``backward="torch"`` is held to the f32 Sequential's own error against f64 autograd (the same f32 arithmetic in another
    summation order: at most 4 x as much, per parameter, maximum norm); ``"device"`` gives ``param_grads``' bits."""
    import torch

    from collectivecrossing_amd import WideMlpHead

    torch.manual_seed(11)
    head = WideMlpHead(batch, 64, 255, act, out_shape=(5, 51))
    L = head.L
    x = torch.randn((300, L), device="cuda")
    coef = torch.randn((300, 5, 51), device="cuda")
    with torch.no_grad():
        hid = torch.empty((300, 64), device="cuda")
        plain = head(x, hidden_out=hid)
    y = head(x)
    assert y.requires_grad and tuple(y.shape) == (300, 5, 51)
    assert torch.equal(y.detach().view(torch.int32), plain.view(torch.int32))      # the same bits under grad
    (y * coef).sum().backward()
    ours = [p.grad.double() for p in head.parameters()]
    grads = {}
    for dtype in (torch.float64, torch.float32):
        seq = head.to_sequential(dtype)
        (seq(x.to(dtype)).view(300, 5, 51) * coef.to(dtype)).sum().backward()
        grads[dtype] = [seq[0].weight.grad.t().double(), seq[0].bias.grad.double(), seq[2].weight.grad.double(), seq[2].bias.grad.double()]
    for name, g, g32, g64 in zip(NAMES, ours, grads[torch.float32], grads[torch.float64]):
        err, yard = float((g - g64).abs().max()), float((g32 - g64).abs().max())
        print(f"{act} grad {name}: max |ours - f64| = {err:.3e}, max |f32 Sequential - f64| = {yard:.3e}, max |f64| = {float(g64.abs().max()):.3e}")
        assert g.shape == g64.shape and err <= 4.0 * yard, name
    with pytest.raises(ValueError):
        head(x, out=torch.empty((300, 255), device="cuda"))
    with pytest.raises(ValueError):
        head(x, hidden_out=hid)
    # the device backward: the bits of param_grads on the very gradient autograd hands over
    dev_head = WideMlpHead(batch, 64, 255, act, backward="device", out_shape=(5, 51))
    dev_head.load_state_dict(head.state_dict())
    xg = x.clone().requires_grad_(True)
    (dev_head(xg) * coef).sum().backward()
    want = dev_head.param_grads(x, hid, coef, want_grad_a=True)           # [300, 5, 51], taken as it is
    batch.synchronize()
    for name, p in zip(NAMES, dev_head.parameters()):
        assert torch.equal(p.grad.view(torch.int32), getattr(want, name).view(torch.int32)), name
    gx = want.grad_a @ dev_head.w1t.detach().t()
    assert torch.equal(xg.grad, gx)
    seq = head.to_sequential(torch.float64)
    x64 = x.double().requires_grad_(True)
    (seq(x64).view(300, 5, 51) * coef.double()).sum().backward()
    assert float((xg.grad.double() - x64.grad).abs().max()) <= 1e-5 * float(x64.grad.abs().max())


def test_static_buffers_capture_and_replay(batch):
    import torch

    from collectivecrossing_amd import WideMlpHead

    torch.manual_seed(3)
    side = torch.cuda.Stream()
    batch.use_stream(side)
    torch.cuda.synchronize()
    try:
        with torch.cuda.stream(side):
            head = WideMlpHead(batch, 64, 255, "tanh", out_shape=(5, 51))
            rows = (16, 8)
            x = torch.randn(rows + (head.L,), device="cuda")
            gy = torch.randn(rows + (5, 51), device="cuda")
            y, hid = torch.empty(rows + (5, 51), device="cuda"), torch.empty(rows + (64,), device="cuda")
            out = head.alloc_param_grads(rows, want_grad_a=True)

            def body():
                with torch.no_grad():
                    head(x, out=y, hidden_out=hid)
                head.param_grads(x, hid, gy, out=out)

            def snapshot():
                side.synchronize()
                return [t.clone() for t in (y, hid, out.w1t, out.b1, out.w2, out.b2, out.grad_a)]

            body()
            eager = snapshot()
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph, stream=side):
                body()
            side.synchronize()
            for _ in range(2):
                for t in (y, hid, out.w1t, out.b1, out.w2, out.b2, out.grad_a):
                    t.view(torch.uint8).fill_(0xEE)
                graph.replay()
                for a, b in zip(snapshot(), eager):
                    assert torch.equal(a.view(torch.int32), b.view(torch.int32))
            x.mul_(0.5)                                                   # new inputs through the same graph
            graph.replay()
            replayed = snapshot()
            body()
            for a, b in zip(snapshot(), replayed):
                assert torch.equal(a.view(torch.int32), b.view(torch.int32))
            assert not torch.equal(replayed[0], eager[0])
    finally:
        batch.use_stream(None)


def test_conversions_and_checkpoints_are_exact(batch):
    import torch

    from collectivecrossing_amd import CategoricalQ, WideMlpHead

    torch.manual_seed(2)
    seq = torch.nn.Sequential(torch.nn.Linear(38, 32), torch.nn.ReLU(), torch.nn.Linear(32, 255)).cuda()
    head = WideMlpHead.from_linear(batch, seq[0], seq[2], "relu")
    assert (head.L, head.H, head.O, head.activation, head.out_shape) == (38, 32, 255, "relu", (255,))
    for a, b in zip(seq.parameters(), head.to_sequential().parameters()):
        assert torch.equal(a, b)
    torch.manual_seed(7)
    cq = CategoricalQ(batch, atoms=51)
    fresh = cq.head(64)
    assert isinstance(fresh, WideMlpHead) and (fresh.O, fresh.out_shape, fresh.backward) == (255, (5, 51), "torch")
    torch.manual_seed(7)
    ref = torch.nn.Sequential(torch.nn.Linear(38, 64), torch.nn.Tanh(), torch.nn.Linear(64, 255))
    assert torch.equal(fresh.w1t.cpu(), ref[0].weight.t()) and torch.equal(fresh.b2.cpu(), ref[2].bias)   # initialised as Linear
    x = torch.randn((300, 38), device="cuda")
    with torch.no_grad():
        y = fresh(x)
        assert float((y.reshape(300, 255) - ref.cuda()(x)).abs().max()) < 1e-5
        q = cq.q_values(y)                                                # feeds CategoricalQ as it is
    assert tuple(q.shape) == (300, 5)
    # a checkpoint: through a file on the CPU into a new head
    buf = io.BytesIO()
    torch.save(fresh.state_dict(), buf)
    buf.seek(0)
    sd = torch.load(buf, map_location="cpu")
    assert sorted(sd) == ["b1", "b2", "w1t", "w2"] and all(not t.is_cuda for t in sd.values())
    other = cq.head(64, backward="device")
    other.load_state_dict(sd)
    with torch.no_grad():
        assert torch.equal(other(x).view(torch.int32), y.view(torch.int32))
    assert [tuple(p.shape) for p in batch.adam(other.parameters()).params] == [(38, 64), (64,), (255, 64), (255,)]
    batch.synchronize()


def test_zero_rows_and_refusals_leave_the_batch_usable(batch):
    import torch

    from collectivecrossing_amd import CategoricalQ, WideMlpHead, _abi

    L, H, O = batch.obs_len, 64, 255
    head = WideMlpHead(batch, H, O, out_shape=(5, 51))
    x = torch.randn((16, 8, L), device="cuda")
    # zero rows: empty tensors, zero gradients, no library call
    with torch.no_grad():
        empty = head(torch.empty((0, L), device="cuda"))
        empty2 = head(torch.empty((3, 0, L), device="cuda"))
    assert tuple(empty.shape) == (0, 5, 51) and tuple(empty2.shape) == (3, 0, 5, 51)
    assert tuple(head(torch.empty((0, L), device="cuda")).shape) == (0, 5, 51)                   # under grad too
    z = head.param_grads(torch.empty((0, L), device="cuda"), torch.empty((0, H), device="cuda"), torch.empty((0, O), device="cuda"))
    assert all(not getattr(z, n).any() for n in NAMES)
    # the wrapper's refusals
    shifted = torch.empty(16 * 8 * L + 1, dtype=torch.float32, device="cuda")[1:].view(16, 8, L)
    assert shifted.is_contiguous() and shifted.data_ptr() % 16
    for bad in (x.double(), x.half(), x[..., :-1], x[..., :-1].contiguous(), x.transpose(0, 1), x.cpu(), shifted, x.cpu().numpy()):
        with pytest.raises(ValueError):
            with torch.no_grad():
                head(bad)
    with torch.no_grad():
        for kw in (dict(out=torch.empty((16, 8, 254), device="cuda")), dict(out=torch.empty((16, 8, 51, 5), device="cuda")),
                   dict(out=torch.empty((16, 8, 255), dtype=torch.float64, device="cuda")), dict(hidden_out=torch.empty((16, 8, 63), device="cuda")),
                   dict(hidden_out=torch.empty(16 * 8 * H + 1, device="cuda")[1:].view(16, 8, H))):
            with pytest.raises(ValueError):
                head(x, **kw)
    for kw in (dict(H=24, O=9), dict(H=8, O=9), dict(H=272, O=9), dict(H=64, O=321), dict(H=64, O=0), dict(H=64, O=9, L=513),
               dict(H=64, O=9, activation="gelu"), dict(H=64, O=9, backward="jax"), dict(H=64, O=255, out_shape=(5, 50)),
               dict(H=64, O=255, out_shape=()), dict(H=64, O=255, out_shape="5x51"), dict(H=64, O=True)):
        with pytest.raises(ValueError):
            WideMlpHead(batch, **kw)
    with pytest.raises(ValueError):
        WideMlpHead("batch", 64, 9)
    with pytest.raises(ValueError):
        CategoricalQ(batch, atoms=51).head(24)
    hid, gy = torch.randn((16, 8, H), device="cuda"), torch.randn((16, 8, 5, 51), device="cuda")
    good = head.param_grads(x, hid, gy)
    for kw in (dict(x=shifted), dict(hidden=hid[..., :-1].contiguous()), dict(hidden=hid.double()), dict(grad_y=gy[..., :-1].contiguous()),
               dict(grad_y=gy.transpose(-1, -2)), dict(grad_y=gy.cpu()), dict(out=(1, 2)), dict(workspace=torch.empty(8, dtype=torch.uint8, device="cuda")),
               dict(workspace=torch.empty(10**6, dtype=torch.float32, device="cuda"))):
        with pytest.raises(ValueError):
            head.param_grads(**{**dict(x=x, hidden=hid, grad_y=gy), **kw})
    small = head.alloc_param_grads((16, 8))
    small.workspace = small.workspace[:-8]
    with pytest.raises(ValueError):
        head.param_grads(x, hid, gy, out=small)                           # its workspace is eight bytes short
    # the library's own refusals (the wrapper refuses first, so they are reached through the bindings)
    lib, h = batch._lib, batch._h
    y = torch.empty((128, O), device="cuda")
    p = [t.data_ptr() for t in (x, head.w1t, head.b1, head.w2, head.b2, y)]
    for args, word in (((None, 128, L, H, O, 0, *p, None), "NULL handle"), ((h, 128, L, H, O, 0, None, *p[1:], None), "NULL"),
                       ((h, 128, L, H, O, 0, *p[:5], None, None), "NULL"), ((h, 0, L, H, O, 0, *p, None), "rows"),
                       ((h, 128, L, 24, O, 0, *p, None), "multiple of 16"), ((h, 128, L, H, 321, 0, *p, None), "O = 321"),
                       ((h, 128, L, H, 0, 0, *p, None), "O = 0"), ((h, 128, 0, H, O, 0, *p, None), "L = 0"),
                       ((h, 128, L, H, O, 2, *p, None), "activation"), ((h, 128, L, H, O, 0, shifted.data_ptr(), *p[1:], None), "aligned"),
                       ((h, 128, L, H, O, 0, *p[:5], y.data_ptr() + 2, None), "aligned"),
                       ((h, 128, L, H, O, 0, *p, hid.data_ptr() + 4), "aligned")):
        assert lib.ccx_mlp_wide_forward(*args) == _abi.EINVAL, args
        assert word in lib.ccx_last_error().decode(), (word, lib.ccx_last_error())
    ws = torch.empty(lib.ccx_mlp_wide_backward_workspace_bytes(128, L, H, O) + 8, dtype=torch.uint8, device="cuda")
    g = [t.data_ptr() for t in (x, hid, gy, head.w2, ws, good.w1t, good.b1, good.w2, good.b2)]
    for args, word in (((None, 128, L, H, O, 0, *g, None), "NULL handle"), ((h, 128, L, H, O, 0, *g[:4], None, *g[5:], None), "NULL"),
                       ((h, 0, L, H, O, 0, *g, None), "rows"), ((h, 128, L, H, 321, 0, *g, None), "O = 321"),
                       ((h, 128, L, 8, O, 0, *g, None), "H = 8"), ((h, 128, L, H, O, 3, *g, None), "activation"),
                       ((h, 128, L, H, O, 0, g[0], g[1] + 4, *g[2:], None), "16-byte"), ((h, 128, L, H, O, 0, *g[:4], g[4] + 4, *g[5:], None), "8-byte"),
                       ((h, 128, L, H, O, 0, *g[:2], g[2] + 2, *g[3:], None), "4-byte"), ((h, 128, L, H, O, 0, *g, hid.data_ptr() + 8), "16-byte")):
        assert lib.ccx_mlp_wide_backward(*args) == _abi.EINVAL, args
        assert word in lib.ccx_last_error().decode(), (word, lib.ccx_last_error())
    assert lib.ccx_mlp_wide_backward_workspace_bytes(257, L, H, O) == 2 * (L * H + H + O * H + O) * 8
    assert lib.ccx_mlp_wide_backward_workspace_bytes(0, L, H, O) == 0 == lib.ccx_mlp_wide_backward_workspace_bytes(8, L, H, 321)
    # the narrow entry points keep their limit
    assert lib.ccx_mlp_forward(h, 128, L, H, 9, 0, *p, None) == _abi.EINVAL and "O = 9" in lib.ccx_last_error().decode()
    again = head.param_grads(x, hid, gy)
    batch.synchronize()
    for n in NAMES:
        assert torch.equal(getattr(again, n).view(torch.int32), getattr(good, n).view(torch.int32))


# ------------------------------------------------------------------------------------------------- 6. the example
def test_the_example_runs_with_a_tiny_configuration():
    code = ("import sys; sys.path.insert(0, 'examples'); import c51_wide_dqn as ex; "
            "stats, equal = ex.train(num_envs=32, updates=6, ring_steps=8, batch=64, warmup_steps=4, target_every=3, "
            "anneal_updates=4, atoms=51, hidden=16, log_every=2); "
            "assert equal and len(stats) == 6 and all(s[6] > 0 and s[0] == s[0] for s in stats); print('ok', equal)")
    run = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True, timeout=300)
    print(run.stdout[-1500:])
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-4000:]
    assert "ok True" in run.stdout and run.stdout.count("update ") == 3
