"""The backward pass of the two-layer perceptron on the device (include/ccx.h: CCX_MLP, backward) against the NumPy spec
(tests/_mlp_backward_spec.py): the four parameter gradients and grad_a bit for bit on row counts that cross every boundary
of the kernel's layout and of the reduction tree, poisoned buffers, a NaN row, autograd with ``backward="device"``, the
gradient through ``ppo_loss``, graph capture and the refusals.  f32 values are compared as bit patterns throughout
(``bits32``; ``bits32c`` only where a NaN is expected: its sign and payload are the one thing the rule leaves open)."""

import numpy as np
import pytest
from _mlp_backward_spec import NAMES, make_mlp_backward_case, mlp_backward_spec
from _mlp_spec import RELU, SHAPES, TANH, bits32, bits32c, mlp_spec
from _reset_obs_spec import make_config

pytestmark = pytest.mark.gpu

# one row; 63 / 64 / 65 rows around one sub-tile; 255 / 256 / 257 around one block; 1000: four blocks, a tail of 232
ROWS = (1, 63, 64, 65, 255, 256, 257, 1000)
ALL_SHAPES = SHAPES + ((1, 16, 1, TANH),)                                   # L = 1: rows * L < 4 floats for one row
ACT = {TANH: "tanh", RELU: "relu"}
OUTS = NAMES + ("ga",)


@pytest.fixture(scope="module")
def batch():
    import torch

    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    from collectivecrossing_amd.batched import BatchedCollectiveCrossing

    b = BatchedCollectiveCrossing(make_config(8, max_steps=12), 96)
    yield b
    b.close()


@pytest.fixture(scope="module")
def spec_cases():
    """Generator rows per shape and the spec's gradients for the first M of them, for every M asked for, made once (the
    chains are walked once: tests/test_mlp_backward_spec.py)."""
    cache = {}

    def get(L, H, O, act, rows=ROWS):
        key = (L, H, O, act, tuple(rows))
        if key not in cache:
            c = make_mlp_backward_case(max(rows), L, H, O, act, seed=L * 7 + H)
            cache[key] = (c, mlp_backward_spec(c["x"], c["hidden"], c["grad_y"], c["w2"], act, rows=rows))
        return cache[key]

    return get


def _head(batch, c, L, H, O, act, backward="torch"):
    import torch

    head = batch.mlp_head(H, O, ACT[act], L=L, backward=backward)
    with torch.no_grad():
        for name in ("w1t", "b1", "w2", "b2"):
            getattr(head, name).copy_(torch.from_numpy(c[name]))
    return head


def _np(res):
    return dict(w1t=res.w1t.cpu().numpy(), b1=res.b1.cpu().numpy(), w2=res.w2.cpu().numpy(), b2=res.b2.cpu().numpy(),
                ga=None if res.grad_a is None else res.grad_a.cpu().numpy())


def _assert_bits(got, want, tag, names=OUTS, bits=bits32):
    for name in names:
        assert got[name].shape == want[name].shape, (name, tag)
        np.testing.assert_array_equal(bits(got[name]), bits(want[name]), err_msg=f"{name}, {tag}")


def _cuda(c, m=None):
    import torch

    return tuple(torch.from_numpy(np.ascontiguousarray(c[k][:m])).cuda() for k in ("x", "hidden", "grad_y"))


# ------------------------------------------------------------------------------------------------- 1. bits against the spec
@pytest.mark.parametrize("L,H,O,act", ALL_SHAPES)
def test_gradients_equal_the_spec(batch, spec_cases, L, H, O, act):
    c, want = spec_cases(L, H, O, act)
    head = _head(batch, c, L, H, O, act)
    for rows in ROWS:
        x, hidden, gy = _cuda(c, rows)
        got = _np(batch.mlp_backward(head, x, hidden, gy, want_grad_a=True))
        bare = _np(batch.mlp_backward(head, x, hidden, gy))
        batch.synchronize()
        _assert_bits(got, want[rows], f"{rows} rows")
        _assert_bits(bare, want[rows], f"{rows} rows, without grad_a", NAMES)
        assert bare["ga"] is None
    assert all(np.isfinite(want[1000][k]).all() and want[1000][k].any() for k in OUTS)


# ------------------------------------------------------------------------------------------------- 2. more than 64 partials
def test_more_than_64_block_partials(batch, spec_cases):
    L, H, O, act = 7, 48, 3, TANH
    rows = (64 * 256 + 1, 128 * 256 + 77)                                  # place 0 gets a second partial; three rounds, the last ragged
    c, want = spec_cases(L, H, O, act, rows)
    head = _head(batch, c, L, H, O, act)
    for m in rows:
        got = _np(batch.mlp_backward(head, *_cuda(c, m), want_grad_a=True))
        batch.synchronize()
        _assert_bits(got, want[m], f"{m} rows")


# ------------------------------------------------------------------------------------------------- 3. poisoned buffers
def test_every_element_is_written_and_the_workspace_means_nothing(batch, spec_cases):
    import torch

    L, H, O, act = SHAPES[0]
    c, want = spec_cases(L, H, O, act)
    head = _head(batch, c, L, H, O, act)
    x, hidden, gy = _cuda(c, 1000)
    out = batch.alloc_mlp_backward(head, (1000,), want_grad_a=True)
    assert out.workspace.numel() == 4 * (L * H + H + O * H + O) * 8
    for fill in (0xEE, 0x55):
        for t in (out.w1t, out.b1, out.w2, out.b2, out.grad_a, out.workspace):
            t.view(torch.uint8).fill_(fill)
        torch.cuda.synchronize()
        assert batch.mlp_backward(head, x, hidden, gy, out=out) is out
        batch.synchronize()
        _assert_bits(_np(out), want[1000], f"buffers filled with {fill:#x}")
    shaped = batch.mlp_backward(head, x.view(10, 100, L), hidden.view(10, 100, H), gy.view(10, 100, O), want_grad_a=True)
    batch.synchronize()
    assert tuple(shaped.grad_a.shape) == (10, 100, H)
    got = _np(shaped)
    got["ga"] = got["ga"].reshape(1000, H)
    _assert_bits(got, want[1000], "a [10, 100] leading shape")


# ------------------------------------------------------------------------------------------------- 4. a NaN row
@pytest.mark.parametrize("L,H,O,act", (SHAPES[1], SHAPES[2]))
def test_a_nan_row_poisons_what_the_spec_says(batch, L, H, O, act):
    M = 300
    c = make_mlp_backward_case(M, L, H, O, act, seed=3)
    c["x"][17, 3] = np.nan
    _, c["hidden"] = mlp_spec(c["x"], c["w1t"], c["b1"], c["w2"], c["b2"], act)   # the forward's hidden: row 17 is NaN
    want = mlp_backward_spec(c["x"], c["hidden"], c["grad_y"], c["w2"], act)
    assert np.isnan(c["hidden"][17]).all() and np.isnan(want["w1t"][3]).all() and np.isnan(want["w2"]).all()
    assert np.isfinite(want["b2"]).all() and np.isfinite(want["ga"][np.arange(M) != 17]).all()
    if act == RELU:                                                        # a NaN h selects +0.0: only the row of x's NaN is lost
        assert np.isfinite(want["b1"]).all() and np.isfinite(np.delete(want["w1t"], 3, 0)).all() and not bits32(want["ga"][17]).any()
    else:
        assert np.isnan(want["b1"]).all() and np.isnan(want["ga"][17]).all()
    head = _head(batch, c, L, H, O, act)
    got = _np(batch.mlp_backward(head, *_cuda(c), want_grad_a=True))
    batch.synchronize()
    _assert_bits(got, want, "a NaN row", bits=bits32c)


# ------------------------------------------------------------------------------------------------- 5. autograd
@pytest.mark.parametrize("act", ("tanh", "relu"))
def test_autograd_on_the_device(batch, act):
    import torch

    def fresh():
        torch.manual_seed(11)
        return batch.mlp_head(64, 5, act, backward="device")

    head = fresh()
    L, H = head.L, head.H
    torch.manual_seed(12)
    x = torch.randn((1000, L), device="cuda")
    coef = torch.randn((1000, 5), device="cuda")
    hidden = torch.empty((1000, H), device="cuda")
    with torch.no_grad():
        plain = head(x, hidden_out=hidden)
    y = head(x)
    assert y.requires_grad
    np.testing.assert_array_equal(bits32(y.detach().cpu().numpy()), bits32(plain.cpu().numpy()))   # the same bits under grad
    (y * coef).sum().backward()
    params = ("w1t", "b1", "w2", "b2")
    ours = {k: getattr(head, k).grad.cpu().numpy() for k in params}
    direct = _np(batch.mlp_backward(head, x, hidden, coef))
    want = mlp_backward_spec(x.cpu().numpy(), hidden.cpu().numpy(), coef.cpu().numpy(), head.w2.detach().cpu().numpy(),
                             TANH if act == "tanh" else RELU)
    _assert_bits(ours, direct, ".grad against mlp_backward", params)
    _assert_bits(ours, want, ".grad against the spec", params)
    # against f64 autograd: the yardstick of tests/test_gpu_mlp.py, the f32 torch module's own error, times 4
    grads = {}
    for dtype in (torch.float64, torch.float32):
        seq = head.to_sequential(dtype)
        (seq(x.to(dtype)) * coef.to(dtype)).sum().backward()
        grads[dtype] = [seq[0].weight.grad.t().double(), seq[0].bias.grad.double(), seq[2].weight.grad.double(), seq[2].bias.grad.double()]
    for name, g32, g64 in zip(params, grads[torch.float32], grads[torch.float64]):
        g = getattr(head, name).grad.double()
        err, yard = float((g - g64).abs().max()), float((g32 - g64).abs().max())
        print(f"{act} grad {name}: max |device - f64| = {err:.3e}, max |f32 Sequential - f64| = {yard:.3e}, max |f64| = {float(g64.abs().max()):.3e}")
        assert g.shape == g64.shape and err <= 4.0 * yard, name
    # x requires a gradient: the parameters' bits stay, x.grad is a torch product on grad_a
    again = fresh()
    xg = x.clone().requires_grad_(True)
    (again(xg) * coef).sum().backward()
    _assert_bits({k: getattr(again, k).grad.cpu().numpy() for k in params}, ours, "with x.requires_grad", params)
    seq = head.to_sequential(torch.float64)
    x64 = x.double().requires_grad_(True)
    (seq(x64) * coef.double()).sum().backward()
    assert float((xg.grad.double() - x64.grad).abs().max()) <= 1e-5 * float(x64.grad.abs().max())
    # a frozen w1t gets no gradient; the others are unchanged
    frozen = fresh()
    frozen.w1t.requires_grad_(False)
    (frozen(x) * coef).sum().backward()
    assert frozen.w1t.grad is None
    _assert_bits({k: getattr(frozen, k).grad.cpu().numpy() for k in params[1:]}, ours, "with w1t frozen", params[1:])
    with pytest.raises(ValueError):
        head(x, out=torch.empty((1000, 5), device="cuda"))


# ------------------------------------------------------------------------------------------------- 6. through the loss
def test_the_update_gradient_is_reproducible_and_equals_the_spec(batch):
    import torch
    from _ppo_loss_spec import ppo_loss_backward_spec, ppo_loss_spec

    M, L = 777, batch.obs_len
    rng = np.random.default_rng(21)
    x = rng.integers(0, 21, size=(M, L)).astype(np.float32)
    actions = rng.integers(0, 5, size=M).astype(np.uint8)
    actions[rng.random(M) < 0.1] = 255
    valid = (rng.random(M) < 0.8).astype(np.uint8)
    logp_old = (-1.6 + 0.2 * rng.standard_normal(M)).astype(np.float32)
    adv, ret = rng.standard_normal(M).astype(np.float32), rng.standard_normal(M).astype(np.float32)
    dev = {k: torch.from_numpy(v).cuda() for k, v in dict(x=x, actions=actions, valid=valid, logp_old=logp_old, adv=adv, ret=ret).items()}

    def update():
        torch.manual_seed(31)
        actor, critic = batch.mlp_head(64, 5, backward="device"), batch.mlp_head(64, 1, "relu", backward="device")
        values = critic(dev["x"]).squeeze(-1)
        r = batch.ppo_loss(actor(dev["x"]), values, dev["actions"], dev["logp_old"], dev["adv"], dev["ret"], valid=dev["valid"])
        r.loss.backward()
        batch.synchronize()
        return actor, critic, [p.grad.cpu().numpy() for h in (actor, critic) for p in (h.w1t, h.b1, h.w2, h.b2)]

    actor, critic, first = update()
    _, _, second = update()
    for a, b in zip(first, second):
        np.testing.assert_array_equal(bits32(a), bits32(b))
    par = [{k: getattr(h, k).detach().cpu().numpy() for k in NAMES} for h in (actor, critic)]
    logits, hid_a = mlp_spec(x, *(par[0][k] for k in NAMES), TANH)
    vals, hid_c = mlp_spec(x, *(par[1][k] for k in NAMES), RELU)
    args = (logits, vals[:, 0], actions, logp_old, adv, ret, None, valid)
    gl, gv = ppo_loss_backward_spec(*args, stats=ppo_loss_spec(*args))
    assert np.isfinite(gl).all() and gl.any() and gv.any() and not gl[actions == 255].any() and not gv[valid == 0].any()
    want = [mlp_backward_spec(x, hid_a, gl, par[0]["w2"], TANH), mlp_backward_spec(x, hid_c, gv[:, None], par[1]["w2"], RELU)]
    for i, name in enumerate(NAMES):
        np.testing.assert_array_equal(bits32(first[i]), bits32(want[0][name]), err_msg=f"actor {name}")
        np.testing.assert_array_equal(bits32(first[4 + i]), bits32(want[1][name]), err_msg=f"critic {name}")


# ------------------------------------------------------------------------------------------------- 7. graph capture
def test_captured_forward_backward_pair_repeats_the_eager_run(spec_cases):
    import torch

    from collectivecrossing_amd.batched import BatchedCollectiveCrossing

    L, H, O, act = SHAPES[0]
    M = 1000
    c, want = spec_cases(L, H, O, act)
    env = BatchedCollectiveCrossing(make_config(8, max_steps=12), 64)
    head = _head(env, c, L, H, O, act)
    side = torch.cuda.Stream()
    env.use_stream(side)
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        x, _, gy = _cuda(c, M)
        y = torch.empty((M, O), device="cuda")
        hidden = torch.empty((M, H), device="cuda")
        out = env.alloc_mlp_backward(head, (M,), want_grad_a=True)

        def body():
            with torch.no_grad():
                head(x, out=y, hidden_out=hidden)
            env.mlp_backward(head, x, hidden, gy, out=out)

        def poison(fill):
            for t in (y, hidden, out.w1t, out.b1, out.w2, out.b2, out.grad_a, out.workspace):
                t.view(torch.uint8).fill_(fill)

        poison(0xEE)
        body()
        side.synchronize()
        eager = _np(out)
        np.testing.assert_array_equal(bits32(hidden.cpu().numpy()), bits32(c["hidden"][:M]))
        _assert_bits(eager, want[M], "eager, static buffers")
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            body()
        side.synchronize()
        for fill in (0x55, 0xAA):                                          # the workspace is overwritten between the replays
            poison(fill)
            graph.replay()
            side.synchronize()
            _assert_bits(_np(out), eager, f"graph replay over {fill:#x}")
    env.use_stream(None)
    env.close()


# ------------------------------------------------------------------------------------------------- 8. refusals
def test_refusals_leave_the_batch_usable(batch, spec_cases):
    import torch

    from collectivecrossing_amd import MlpGradResult, _abi

    L, H, O, act = SHAPES[0]
    M = 256
    c, want = spec_cases(L, H, O, act)
    head = _head(batch, c, L, H, O, act)
    x, hidden, gy = _cuda(c, M)

    def shifted(t):
        s = torch.empty(t.numel() + 1, dtype=torch.float32, device="cuda")[1:].view(t.shape)
        assert s.is_contiguous() and s.data_ptr() % 16
        return s

    good = dict(head=head, x=x, hidden=hidden, grad_y=gy)
    small = batch.alloc_mlp_backward(head, (M,))
    small.workspace = small.workspace[:-8]
    odd_a = batch.alloc_mlp_backward(head, (M,), want_grad_a=True)
    odd_a.grad_a = shifted(odd_a.grad_a)
    wrong = batch.alloc_mlp_backward(head, (M,))
    wrong.b1 = wrong.b1[:-1]
    for kw in (dict(x=x.double()), dict(x=x.half()), dict(x=x[:, :-1].contiguous()), dict(x=x.cpu()), dict(x=x.cpu().numpy()),
               dict(x=x.t().contiguous().t()), dict(x=shifted(x)), dict(hidden=shifted(hidden)), dict(hidden=hidden[:-1]),
               dict(hidden=hidden.double()), dict(grad_y=gy[:, :-1]), dict(grad_y=gy[:, :-1].contiguous()), dict(grad_y=gy.cpu()),
               dict(grad_y=gy.double()), dict(head="head"), dict(head=batch.mlp_head(64, 5, L=L + 1)), dict(out=(1, 2)),
               dict(out=small), dict(out=odd_a), dict(out=wrong)):
        with pytest.raises(ValueError):
            batch.mlp_backward(**{**good, **kw})
    with pytest.raises(ValueError):
        batch.mlp_head(64, backward="other")
    with pytest.raises(ValueError):
        batch.mlp_head(64, backward=None)
    with pytest.raises(ValueError):                                        # hidden_out together with a gradient path
        head(x, hidden_out=torch.empty((M, H), device="cuda"))
    with torch.no_grad():
        for bad in (torch.empty((M, H + 1), device="cuda"), torch.empty((M, H), dtype=torch.float64, device="cuda"),
                    shifted(hidden), torch.empty((M, H))):
            with pytest.raises(ValueError):
                head(x, hidden_out=bad)
    # zero rows: zeros, without the library
    empty = batch.mlp_backward(head, x[:0], hidden[:0], gy[:0], want_grad_a=True)
    batch.synchronize()
    assert tuple(empty.grad_a.shape) == (0, H) and all(not bits32(v).any() for k, v in _np(empty).items() if k != "ga")
    # the library's own refusals (the wrapper refuses first, so they are reached through the bindings)
    lib, h = batch._lib, batch._h
    assert lib.ccx_mlp_backward_workspace_bytes(M, L, H, O) == (L * H + H + O * H + O) * 8
    assert lib.ccx_mlp_backward_workspace_bytes(0, L, H, O) == 0 and lib.ccx_mlp_backward_workspace_bytes(M, L, 24, O) == 0
    out = batch.alloc_mlp_backward(head, (M,), want_grad_a=True)
    p = [t.data_ptr() for t in (x, hidden, gy, head.w2, out.workspace, out.w1t, out.b1, out.w2, out.b2, out.grad_a)]
    dims = (M, L, H, O, 0)

    def but(i, v):
        return tuple(p[:i]) + (v,) + tuple(p[i + 1:])

    for args, word in (((None, *dims, *p), "NULL handle"), ((h, *dims, *but(0, None)), "NULL"), ((h, *dims, *but(4, None)), "NULL"),
                       ((h, *dims, *but(8, None)), "NULL"), ((h, 0, L, H, O, 0, *p), "rows"), ((h, -5, L, H, O, 0, *p), "rows"),
                       ((h, 2**40 * 256, L, H, O, 0, *p), "rows"), ((h, M, L, 24, O, 0, *p), "multiple of 16"),
                       ((h, M, L, H, 9, 0, *p), "O = 9"), ((h, M, 0, H, O, 0, *p), "L = 0"), ((h, M, L, H, O, 2, *p), "activation"),
                       ((h, *dims, *but(0, shifted(x).data_ptr())), "16-byte"), ((h, *dims, *but(1, p[1] + 4)), "16-byte"),
                       ((h, *dims, *but(9, p[9] + 8)), "16-byte"), ((h, *dims, *but(4, p[4] + 4)), "8-byte"),
                       ((h, *dims, *but(2, p[2] + 2)), "4-byte"), ((h, *dims, *but(6, p[6] + 1)), "4-byte")):
        assert lib.ccx_mlp_backward(*args) == _abi.EINVAL, args
        assert word in lib.ccx_last_error().decode(), (word, lib.ccx_last_error())
    assert lib.ccx_mlp_backward(h, *dims, *but(9, None)) == _abi.OK           # grad_a may be NULL
    assert isinstance(out, MlpGradResult)
    got = _np(batch.mlp_backward(head, x, hidden, gy, want_grad_a=True))
    batch.synchronize()
    _assert_bits(got, want[M], "after the refusals")
