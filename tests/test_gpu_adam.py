"""The optimiser step on the device (include/ccx.h: CCX_ADAM) against the NumPy spec (tests/_adam_spec.py): parameters, m, v,
the 64 state bytes and stats bit for bit over three steps, on tensor sets at the boundaries of the reduction tree; clipping
below and above the norm, weight decay, the rate by value and from the device scalar, a NaN and an inf gradient (a skipped
step), graph replay against eager calls, state_dict, the update through autograd, and the refusals.  Every comparison is on
bit patterns; only a NaN norm in ``stats[0]`` is compared as "NaN" (IEEE leaves its sign and payload open)."""

import ctypes as C

import numpy as np
import pytest
from _adam_spec import TWO_HEADS, bits32, make_adam_case, run_spec, sum_of_squares
from _reset_obs_spec import make_config

pytestmark = pytest.mark.gpu

# single tensors around a group (63, 64, 65), a block (255, 256, 257) and several blocks with a tail (1023); 16 389: B = 65, a
# place of the final wave adds twice; the two heads of the examples with their ragged tails, B = 27; 32 blocks of one element;
# one head of L = 512, H = 256, O = 8: B = 522
SETS = {"1": (1,), "63": (63,), "64": (64,), "65": (65,), "255": (255,), "256": (256,), "257": (257,), "1023": (1023,),
        "16389": (16389,), "two heads": TWO_HEADS, "32 x 1": (1,) * 32, "133384": (133384,)}
HYPER = dict(beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.0, max_grad_norm=0.0)
LRS = (3e-4, 1e-2, 1e-3)


@pytest.fixture(scope="module")
def batch():
    import torch

    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    from collectivecrossing_amd.batched import BatchedCollectiveCrossing

    b = BatchedCollectiveCrossing(make_config(8, max_steps=12), 96)
    yield b
    b.close()


def _dev(arrays):
    import torch

    return [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in arrays]


def _adam(batch, params_np, lr, hyper):
    return batch.adam(_dev(params_np), lr=lr, betas=(hyper["beta1"], hyper["beta2"]), eps=hyper["eps"],
                      weight_decay=hyper["weight_decay"], max_grad_norm=hyper["max_grad_norm"])


def _snapshot(batch, opt):
    batch.synchronize()
    return ([p.detach().cpu().numpy() for p in opt.params], [m.cpu().numpy() for m in opt.m], [v.cpu().numpy() for v in opt.v],
            opt.state.cpu().numpy(), opt.stats.cpu().numpy())


def _assert_same(got, want, tag):
    gp, gm, gv, gstate, gstats = got
    wp, wm, wv, wstate, wstats = want
    nan = np.isnan(wstats)
    np.testing.assert_array_equal(np.isnan(gstats), nan, err_msg="stats (NaN places), " + tag)
    np.testing.assert_array_equal(bits32(gstats)[~nan], bits32(wstats)[~nan], err_msg="stats, " + tag)
    np.testing.assert_array_equal(gstate, wstate, err_msg="state bytes, " + tag)
    for name, g, w in (("param", gp, wp), ("m", gm, wm), ("v", gv, wv)):
        assert len(g) == len(w)
        for k, (a, b) in enumerate(zip(g, w)):
            np.testing.assert_array_equal(bits32(a), bits32(b), err_msg=f"{name} {k}, {tag}")


def _three_steps(batch, params, grad_steps, lrs, hyper, tag, by_value=False):
    """Steps on the device, compared with the spec after every one.  Returns the spec's per-step results."""
    want = run_spec(params, grad_steps, lrs, **hyper)
    opt = _adam(batch, params, lrs[0], hyper)
    for s, (grads, lr) in enumerate(zip(grad_steps, lrs)):
        g = _dev(grads)
        if by_value:                                                     # NULL lr_dev: the by-value argument is the rate
            batch._adam_step(opt.params, g, opt.m, opt.v, float(np.float32(lr)), None, opt._hyper, opt.state, opt.workspace, opt.stats)
        else:
            opt.lr = lr                                                  # the device scalar, written on the handle's stream
            opt.step(grads=g)
        _assert_same(_snapshot(batch, opt), want[s], f"{tag}, step {s}")
        for a, b in zip(g, grads):                                       # gradients are read only
            np.testing.assert_array_equal(bits32(a.cpu().numpy()), bits32(b))
    return want, opt


# ------------------------------------------------------------------------------------------------- 1. the tree's boundaries
@pytest.mark.parametrize("name", list(SETS))
def test_three_steps_equal_the_spec_at_the_boundaries_of_the_tree(batch, name):
    numels = SETS[name]
    params, grad_steps = make_adam_case(numels, seed=100 + len(numels) + numels[0])
    gn = float(np.sqrt(sum_of_squares(grad_steps[0])))
    hyper = {**HYPER, "max_grad_norm": gn / 3}                            # (every step's norm is of this size: the scale is in use)
    want, opt = _three_steps(batch, params, grad_steps, LRS, hyper, name)
    assert want[0][4][1] < 1.0 and want[0][4][2] == 0.0
    assert opt.counts() == (3, 0)
    B = sum(-(-n // 256) for n in numels)
    assert opt.workspace.numel() == 64 + 8 * B


# ------------------------------------------------------------------------------------------------- 2. hyper-parameters
@pytest.mark.parametrize("case", ("clip below", "clip above", "no clip", "decay", "decay and clip", "beta1 = 0"))
def test_clipping_decay_and_betas(batch, case):
    params, grad_steps = make_adam_case(TWO_HEADS, seed=7)
    norms = [float(np.sqrt(sum_of_squares(g))) for g in grad_steps]
    extra = {"clip below": dict(max_grad_norm=max(norms) * 2), "clip above": dict(max_grad_norm=min(norms) / 2), "no clip": {},
             "decay": dict(weight_decay=0.01), "decay and clip": dict(weight_decay=0.1, max_grad_norm=min(norms) / 2),
             "beta1 = 0": dict(beta1=0.0)}[case]
    want, _ = _three_steps(batch, params, grad_steps, LRS, {**HYPER, **extra}, case)
    scales = [w[4][1] for w in want]
    if case in ("clip below", "no clip", "decay", "beta1 = 0"):
        assert all(s == 1.0 for s in scales)                             # gn < max_grad_norm: the gradient goes through unscaled
    else:
        assert all(s < 1.0 for s in scales)


def test_the_rate_by_value_and_from_the_device_scalar(batch):
    params, grad_steps = make_adam_case((257, 5), seed=9)
    hyper = {**HYPER, "weight_decay": 0.01, "max_grad_norm": 0.5}
    a, _ = _three_steps(batch, params, grad_steps, LRS, hyper, "lr_dev")
    b, _ = _three_steps(batch, params, grad_steps, LRS, hyper, "lr by value", by_value=True)
    assert [w[4][3] for w in a] == [np.float32(x) for x in LRS]          # stats[3]: the rate used


# ------------------------------------------------------------------------------------------------- 3. a skipped step
@pytest.mark.parametrize("bad", (np.nan, np.inf, -np.inf))
def test_a_bad_gradient_skips_the_step_and_the_next_continues(batch, bad):
    params, grad_steps = make_adam_case(TWO_HEADS, seed=5, steps=3)
    grad_steps[1][-1][-1] = bad                                          # the last place of the last tensor's tail
    hyper = {**HYPER, "weight_decay": 0.01, "max_grad_norm": 0.5}
    want, opt = _three_steps(batch, params, grad_steps, (3e-4,) * 3, hyper, f"bad = {bad}")
    assert [w[4][2] for w in want] == [0.0, 1.0, 0.0]
    for k in range(3):                                                   # params, m, v: the skipped step kept every bit
        for a, b in zip(want[0][k], want[1][k]):
            np.testing.assert_array_equal(bits32(a), bits32(b))
    assert opt.counts() == (2, 1)                                        # the following step continued from the unskipped count
    assert float(opt.skipped) == 0.0 and np.isfinite(float(opt.grad_norm)) and 0.0 < float(opt.scale) <= 1.0


# ------------------------------------------------------------------------------------------------- 4. graph replay
def test_a_replayed_graph_equals_eager_calls_and_follows_the_rate():
    import torch

    from collectivecrossing_amd.batched import BatchedCollectiveCrossing

    params, grad_steps = make_adam_case(TWO_HEADS, seed=13, steps=5)
    lrs = (3e-4, 3e-4, 3e-4, 1e-3, 1e-3)
    hyper = {**HYPER, "weight_decay": 0.01, "max_grad_norm": 0.5}
    want = run_spec(params, grad_steps, lrs, **hyper)
    env = BatchedCollectiveCrossing(make_config(8, max_steps=12), 64)
    side = torch.cuda.Stream()
    env.use_stream(side)
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        eager = _adam(env, params, lrs[0], hyper)
        for s in range(5):
            eager.lr = lrs[s]
            eager.step(grads=_dev(grad_steps[s]))
            _assert_same(_snapshot(env, eager), want[s], f"eager, step {s}")
        opt = _adam(env, params, lrs[0], hyper)
        static = _dev(grad_steps[0])
        side.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            opt.step(grads=static)
        side.synchronize()
        assert opt.counts() == (0, 0)                                    # capturing ran nothing
        for s in range(5):
            for t, g in zip(static, grad_steps[s]):
                t.copy_(torch.from_numpy(g))
            if float(np.float32(lrs[s])) != opt.lr:
                opt.lr = lrs[s]                                          # between two replays: the device scalar
            graph.replay()
            _assert_same(_snapshot(env, opt), want[s], f"replay {s}")
        assert opt.counts() == (5, 0)                                    # the graph advanced the device's step count
    env.use_stream(None)
    env.close()


# ------------------------------------------------------------------------------------------------- 5. state_dict
def test_state_dict_continues_with_the_same_bits(batch):
    import torch

    params, grad_steps = make_adam_case((1023, 64, 5), seed=17)
    hyper = {**HYPER, "weight_decay": 0.01, "max_grad_norm": 0.5}
    want = run_spec(params, grad_steps, LRS, **hyper)
    first = _adam(batch, params, LRS[0], hyper)
    for s in range(2):
        first.lr = LRS[s]
        first.step(grads=_dev(grad_steps[s]))
    sd = first.state_dict()
    batch.synchronize()
    fresh = batch.adam([p.clone() for p in first.params], lr=0.5, betas=(0.5, 0.5), eps=1.0)        # other hyper-parameters: replaced
    fresh.load_state_dict(sd)
    assert fresh.lr == first.lr and fresh._hyper == first._hyper and fresh.counts() == (2, 0)
    for opt in (first, fresh):
        opt.lr = LRS[2]
        opt.step(grads=_dev(grad_steps[2]))
        _assert_same(_snapshot(batch, opt), want[2], "the third step")
    assert sd["state"].data_ptr() != first.state.data_ptr() and torch.equal(sd["m"][0].cpu(), torch.from_numpy(want[1][1][0]))
    with pytest.raises(ValueError):
        fresh.load_state_dict({"m": sd["m"][:-1], "v": sd["v"], "state": sd["state"], "hyper": sd["hyper"]})
    with pytest.raises(ValueError):
        fresh.load_state_dict({"m": sd["m"]})


# ------------------------------------------------------------------------------------------------- 6. through autograd
def test_the_update_through_autograd_is_pinned_by_its_seeds(batch):
    import torch

    M, L = 777, batch.obs_len
    rng = np.random.default_rng(21)
    x = rng.integers(0, 21, size=(M, L)).astype(np.float32)
    actions = rng.integers(0, 5, size=M).astype(np.uint8)
    actions[rng.random(M) < 0.1] = 255
    valid = (rng.random(M) < 0.8).astype(np.uint8)
    logp_old = (-1.6 + 0.2 * rng.standard_normal(M)).astype(np.float32)
    adv, ret = rng.standard_normal(M).astype(np.float32), rng.standard_normal(M).astype(np.float32)
    dev = {k: torch.from_numpy(v).cuda() for k, v in dict(x=x, actions=actions, valid=valid, logp_old=logp_old, adv=adv, ret=ret).items()}

    def run():
        torch.manual_seed(31)
        actor, critic = batch.mlp_head(64, 5, backward="device"), batch.mlp_head(64, 1, "relu", backward="device")
        opt = batch.adam([*actor.parameters(), *critic.parameters()], lr=3e-3, weight_decay=0.01, max_grad_norm=0.5)
        norms = []
        for _ in range(3):
            r = batch.ppo_loss(actor(dev["x"]), critic(dev["x"]).squeeze(-1), dev["actions"], dev["logp_old"], dev["adv"], dev["ret"],
                               valid=dev["valid"])
            opt.zero_grad()
            r.loss.backward()
            opt.step()
            norms.append(opt.stats.clone())
        return _snapshot(batch, opt), torch.stack(norms).cpu().numpy(), opt

    (first, n1, opt), (second, n2, _) = run(), run()
    _assert_same(first, second, "two runs from the same seeds")
    np.testing.assert_array_equal(bits32(n1), bits32(n2))
    assert opt.counts() == (3, 0) and np.isfinite(n1).all() and (n1[:, 0] > 0).all() and (n1[:, 1] < 1.0).any()
    torch.manual_seed(31)
    fresh = [p.detach().cpu().numpy() for h in (batch.mlp_head(64, 5), batch.mlp_head(64, 1, "relu")) for p in h.parameters()]
    assert any((bits32(a) != bits32(b)).any() for a, b in zip(first[0], fresh))       # the parameters moved
    opt.zero_grad(set_to_none=True)
    assert all(p.grad is None for p in opt.params)
    with pytest.raises(ValueError):                                      # a missing .grad
        opt.step()
    assert opt.counts() == (3, 0)


# ------------------------------------------------------------------------------------------------- 7. refusals
def test_refusals_come_before_the_library_is_called(batch):
    import torch

    from collectivecrossing_amd import DeviceAdam, _abi

    params, grad_steps = make_adam_case((300, 7), seed=3)
    good = _dev(params)

    def shifted(t):
        s = torch.empty(t.numel() + 1, dtype=torch.float32, device="cuda")[1:].view(t.shape)
        assert s.is_contiguous() and s.data_ptr() % 16
        return s

    for bad in ([good[0].double(), good[1]], [good[0].cpu(), good[1]], [good[0].half()], [torch.empty((4, 6), device="cuda").t()],
                [shifted(good[0])], [good[0][:0]], [], [torch.zeros(1, device="cuda")] * 33, [good[0].cpu().numpy()], 5):
        with pytest.raises(ValueError):
            batch.adam(bad)
    nan, inf = float("nan"), float("inf")
    for kw in (dict(lr=-1e-3), dict(lr=nan), dict(lr=inf), dict(betas=(1.0, 0.999)), dict(betas=(0.9, 1.0)), dict(betas=(-0.1, 0.9)),
               dict(betas=(0.9, 0.99999999)), dict(betas=(0.9,)), dict(betas=0.9), dict(eps=0.0), dict(eps=-1e-8), dict(eps=1e-50),
               dict(eps=inf), dict(weight_decay=-0.1), dict(weight_decay=nan), dict(max_grad_norm=-1.0), dict(max_grad_norm=inf),
               dict(lr="fast")):
        with pytest.raises(ValueError):
            batch.adam(good, **kw)
    opt = batch.adam(good, lr=1e-3, max_grad_norm=0.5)
    assert isinstance(opt, DeviceAdam)
    g = _dev(grad_steps[0])
    for bad in ([g[0]], [g[0], g[1], g[1]], [g[0].double(), g[1]], [g[0].cpu(), g[1]], [g[0][:-1], g[1]], [g[0], None],
                [shifted(g[0]), g[1]], [g[0].view(2, 150), g[1]], [g[0], torch.empty((7, 2), device="cuda")[:, 0]], 7):
        with pytest.raises(ValueError):
            opt.step(grads=bad)
    with pytest.raises(ValueError):                                      # plain tensors carry no .grad
        opt.step()
    for bad in (-1.0, nan, inf, "x"):
        with pytest.raises(ValueError):
            opt.lr = bad
    assert opt.lr == float(np.float32(1e-3)) and opt.counts() == (0, 0)   # nothing ran
    before = _snapshot(batch, opt)
    assert not bits32(before[4]).any()
    # the library's own refusals (the wrapper refuses first, so they are reached through the bindings)
    lib, h = batch._lib, batch._h
    numel = (C.c_int64 * 2)(300, 7)
    assert lib.ccx_adam_workspace_bytes(2, numel) == 64 + 8 * 3
    assert lib.ccx_adam_workspace_bytes(0, numel) == 0 and lib.ccx_adam_workspace_bytes(33, numel) == 0
    assert lib.ccx_adam_workspace_bytes(2, (C.c_int64 * 2)(300, 0)) == 0 and lib.ccx_adam_workspace_bytes(2, None) == 0

    def table(rows):
        tab = (_abi.CcxAdamTensor * max(len(rows), 1))()
        for r, (p, gr, m, v, n) in zip(tab, rows):
            r.param, r.grad, r.m, r.v, r.numel = p, gr, m, v, n
        return tab

    rows = [(p.data_ptr(), x.data_ptr(), m.data_ptr(), v.data_ptr(), p.numel()) for p, x, m, v in zip(opt.params, g, opt.m, opt.v)]
    tail = (opt.state.data_ptr(), opt.workspace.data_ptr(), opt.stats.data_ptr())
    hy = (0.9, 0.999, 1e-8, 0.0, 0.5)

    def but(i, v):
        return tuple(tail[:i]) + (v,) + tuple(tail[i + 1:])

    def row_but(i, v):
        r = list(rows[0])
        r[i] = v
        return [tuple(r), rows[1]]

    for args, word in (((None, 2, table(rows), 1e-3, None, *hy, *tail), "NULL handle"),
                       ((h, 2, None, 1e-3, None, *hy, *tail), "NULL"), ((h, 2, table(rows), 1e-3, None, *hy, *but(0, None)), "NULL"),
                       ((h, 2, table(rows), 1e-3, None, *hy, *but(1, None)), "NULL"), ((h, 2, table(rows), 1e-3, None, *hy, *but(2, None)), "NULL"),
                       ((h, 0, table(rows), 1e-3, None, *hy, *tail), "num_tensors"), ((h, 33, table(rows), 1e-3, None, *hy, *tail), "num_tensors"),
                       ((h, 2, table(row_but(1, None)), 1e-3, None, *hy, *tail), "NULL pointer"),
                       ((h, 2, table(row_but(4, 0)), 1e-3, None, *hy, *tail), "numel"),
                       ((h, 2, table(row_but(4, 2**41)), 1e-3, None, *hy, *tail), "numel"),
                       ((h, 2, table(row_but(0, rows[0][0] + 4)), 1e-3, None, *hy, *tail), "16-byte"),
                       ((h, 2, table(row_but(3, rows[0][3] + 8)), 1e-3, None, *hy, *tail), "16-byte"),
                       ((h, 2, table(rows), 1e-3, None, *hy, *but(0, tail[0] + 4)), "8-byte"),
                       ((h, 2, table(rows), 1e-3, None, *hy, *but(1, tail[1] + 4)), "8-byte"),
                       ((h, 2, table(rows), 1e-3, None, *hy, *but(2, tail[2] + 2)), "4-byte"),
                       ((h, 2, table(rows), 1e-3, opt._lr_dev.data_ptr() + 1, *hy, *tail), "4-byte"),
                       ((h, 2, table(rows), -1.0, None, *hy, *tail), "lr"), ((h, 2, table(rows), nan, None, *hy, *tail), "lr"),
                       ((h, 2, table(rows), 1e-3, None, 1.0, 0.999, 1e-8, 0.0, 0.5, *tail), "beta1"),
                       ((h, 2, table(rows), 1e-3, None, 0.9, -0.5, 1e-8, 0.0, 0.5, *tail), "beta2"),
                       ((h, 2, table(rows), 1e-3, None, 0.9, 0.999, 0.0, 0.0, 0.5, *tail), "eps"),
                       ((h, 2, table(rows), 1e-3, None, 0.9, 0.999, 1e-8, -1.0, 0.5, *tail), "weight_decay"),
                       ((h, 2, table(rows), 1e-3, None, 0.9, 0.999, 1e-8, 0.0, inf, *tail), "max_grad_norm")):
        assert lib.ccx_adam_step(*args) == _abi.EINVAL, word
        assert word in lib.ccx_last_error().decode(), (word, lib.ccx_last_error())
    _assert_same(_snapshot(batch, opt), before, "after the refusals")    # no refusal launched anything
    want = run_spec(params, grad_steps[:1], (1e-3,), **{**HYPER, "max_grad_norm": 0.5})
    opt.step(grads=g)
    _assert_same(_snapshot(batch, opt), want[0], "the batch stays usable")
