"""The deep perceptron on the device (include/ccx.h: CCX_MLP_DEEP) against its rule: y, both hiddens, the six parameter
gradients and both grad_a bit for bit on the catalogue of tests/_mlp_deep_spec.py and on row counts around every boundary of
the kernels' layout; the deep entry points against CCX_MLP's and CCX_MLP_WIDE's through the identities of the rule, kernel
against kernel; the fused actor launches against the two launches they stand for; row independence; the Python layer
(autograd in both modes, graph capture, conversions, checkpoints, zero rows, refusals); the example.  The reference is the
rule of csrc/ccx_mlp_deep.h compiled for the host, which tests/test_mlp_deep_host_rule.py shows equal to the NumPy spec; at
the workload's head the NumPy spec itself.  f32 values are compared as bit patterns throughout (tests/_mlp_spec.bits32c: a
NaN's sign and payload are the one thing the rule leaves open)."""

import io
import itertools
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
from _mlp_deep_host_rule import compiler, host_backward, host_forward, launch_shape, load
from _mlp_deep_spec import (CATALOGUE, NAMES, RELU, TANH, bits32c, deep_backward_spec, deep_spec, make_deep_backward_case,
                            make_deep_case)
from _mlp_spec import bits32
from _reset_obs_spec import make_config

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
ACT = {TANH: "tanh", RELU: "relu"}
SEED = 0x0123_4567_89AB_CDEF
FORWARD_ROWS = (1, 63, 64, 65, 129)
# the catalogue with an activation each: both appear at small and at large shapes
SHAPES = tuple(s + (RELU if i % 2 else TANH,) for i, s in enumerate(CATALOGUE))
AGENTS_OF_L = {18: 3, 38: 8, 262: 64}                                     # obs_len = 6 + 4 N
ALL = NAMES + ("ga1", "ga2")


@pytest.fixture(scope="module")
def batches():
    import torch

    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    from collectivecrossing_amd.batched import BatchedCollectiveCrossing

    made = {}

    def get(N=8, E=16):
        if (N, E) not in made:
            b = BatchedCollectiveCrossing(make_config(N, max_steps=12), E)
            b.make_reset_pool(seed0=5, size=256)
            made[N, E] = b
        return made[N, E]

    yield get
    for b in made.values():
        b.close()


@pytest.fixture(scope="module")
def batch(batches):
    return batches()


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    cxx = compiler()
    assert cxx is not None, "the reference needs a host C++ compiler"
    return load(cxx, tmp_path_factory.mktemp("gpu_mlp_deep"))


def _head(batch, c, L, H1, H2, O, act, **kw):
    import torch

    from collectivecrossing_amd import DeepMlpHead

    head = DeepMlpHead(batch, H1, H2, O, ACT[act], L=L, **kw)
    with torch.no_grad():
        for name in NAMES:
            getattr(head, name).copy_(torch.from_numpy(c[name]))
    return head


def _dev(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _poisoned(shape, dtype=None):
    import torch

    t = torch.empty(shape, dtype=dtype or torch.float32, device="cuda")
    t.view(torch.uint8).fill_(0xEE)
    return t


def _np(t):
    return t.cpu().numpy()


# ------------------------------------------------------------------------------------------------- 1. the forward
@pytest.mark.parametrize("L,H1,H2,O,act", SHAPES)
def test_y_and_hiddens_equal_the_rule(batch, host, L, H1, H2, O, act):
    import torch

    c = make_deep_case(max(FORWARD_ROWS), L, H1, H2, O, seed=L * 7 + H1 + H2)
    p = tuple(c[n] for n in NAMES)
    want = host_forward(host, c["x"], *p, act)
    if (L, H1, H2, O) == (38, 64, 64, 5):                                 # the workload's head: the NumPy spec itself
        for w, s in zip(want, deep_spec(c["x"], *p, act)):
            np.testing.assert_array_equal(bits32c(w), bits32c(s))
    head = _head(batch, c, L, H1, H2, O, act)
    x_all = _dev(c["x"])
    for rows in FORWARD_ROWS:
        x = x_all[:rows].clone()
        y, h1, h2 = _poisoned((rows, O)), _poisoned((rows, H1)), _poisoned((rows, H2))
        torch.cuda.synchronize()
        with torch.no_grad():
            got = head(x, out=y, hidden1_out=h1, hidden2_out=h2)
            plain = head(x)
        batch.synchronize()
        assert got.data_ptr() == y.data_ptr()
        for name, g, w in zip(("y", "hidden1", "hidden2"), (y, h1, h2), want):
            np.testing.assert_array_equal(bits32c(_np(g)), bits32c(w[:rows]), err_msg=f"{name}, {rows} rows")
        np.testing.assert_array_equal(bits32(_np(plain)), bits32(_np(y)), err_msg=f"head(x), {rows} rows")
    assert np.isnan(want[0]).any() and np.isfinite(want[0]).any()


# ------------------------------------------------------------------------------------------------- 2. the backward
def _check_backward(batch, host, c, L, H1, H2, O, act, rows_list, spec=False):
    import torch

    head = _head(batch, c, L, H1, H2, O, act)
    xa, h1a, h2a, gya = (_dev(c[k]) for k in ("x", "hidden1", "hidden2", "grad_y"))
    for rows in rows_list:
        args = (c["x"][:rows], c["hidden1"][:rows], c["hidden2"][:rows], c["grad_y"][:rows], c["w2t"], c["w3"], act)
        want = host_backward(host, *args)
        if spec:
            numpy_spec = deep_backward_spec(*args)
            for name in ALL:
                np.testing.assert_array_equal(bits32c(want[name]), bits32c(numpy_spec[name]), err_msg=name)
        x, h1, h2, gy = (t[:rows].clone() for t in (xa, h1a, h2a, gya))
        out = head.alloc_param_grads((rows,), want_grad_a=True)
        for t in out.grads() + (out.grad_a1, out.grad_a2):
            t.view(torch.uint8).fill_(0xEE)
        torch.cuda.synchronize()
        got = head.param_grads(x, h1, h2, gy, out=out)
        fresh = head.param_grads(x, h1, h2, gy)                           # its own outputs and workspace, no grad_a
        batch.synchronize()
        assert got is out and fresh.grad_a1 is None and fresh.grad_a2 is None
        for name in NAMES:
            np.testing.assert_array_equal(bits32c(_np(getattr(out, name))), bits32c(want[name]), err_msg=f"{name}, {rows} rows")
            np.testing.assert_array_equal(bits32c(_np(getattr(fresh, name))), bits32c(want[name]), err_msg=f"{name}, {rows} rows")
        np.testing.assert_array_equal(bits32c(_np(out.grad_a1)), bits32c(want["ga1"]), err_msg=f"grad_a1, {rows} rows")
        np.testing.assert_array_equal(bits32c(_np(out.grad_a2)), bits32c(want["ga2"]), err_msg=f"grad_a2, {rows} rows")


@pytest.mark.parametrize("L,H1,H2,O,act", SHAPES)
def test_gradients_equal_the_rule(batch, host, L, H1, H2, O, act):
    R = launch_shape(host, L, H1, H2, O).sub_rows                        # the rows of a sub-tile of the blocks kernel
    rows_list = sorted({R - 1, R, R + 1, 2 * R + 3, 255, 256, 257})
    c = make_deep_backward_case(max(rows_list), L, H1, H2, O, act, seed=L + H1 + O)
    _check_backward(batch, host, c, L, H1, H2, O, act, rows_list, spec=(L, H1, H2, O) == (18, 16, 32, 5))


def test_gradients_over_more_than_64_blocks(batch, host):
    """16 385 rows are 65 blocks: the final step's places take a second partial."""
    L, H1, H2, O, rows = 18, 16, 32, 5, 16385
    c = make_deep_backward_case(rows, L, H1, H2, O, RELU, seed=3)
    _check_backward(batch, host, c, L, H1, H2, O, RELU, (rows,))


# ------------------------------------------------------------------------------------------------- 3. kernel against kernel
@pytest.mark.parametrize("L,H1,H2,O,act", SHAPES)
def test_deep_entry_points_give_the_bits_of_the_identities(batch, L, H1, H2, O, act):
    import torch

    rows = 300 if L < 100 else 70
    c = make_deep_backward_case(rows, L, H1, H2, O, act, seed=L + O)
    adv = make_deep_case(rows, L, H1, H2, O, seed=L + O)                  # rows with NaN and infinities for the forward
    lib = batch._lib
    p = {k: _dev(c[k]) for k in NAMES}
    x = _dev(adv["x"])
    y, h1, h2 = _poisoned((rows, O)), _poisoned((rows, H1)), _poisoned((rows, H2))
    batch._enqueue(lib.ccx_mlp_deep_forward, rows, L, H1, H2, O, act, x, *(p[k] for k in NAMES), y, h1, h2)
    # the forward: CCX_MLP on x gives hidden1 (whatever its second layer), CCX_MLP on hidden1 gives hidden2 and y
    dummy_w, dummy_b = torch.ones((1, H1), device="cuda"), torch.ones((1,), device="cuda")
    n1, ny1 = _poisoned((rows, H1)), _poisoned((rows, 1))
    batch._enqueue(lib.ccx_mlp_forward, rows, L, H1, 1, act, x, p["w1t"], p["b1"], dummy_w, dummy_b, ny1, n1)
    ny, n2 = _poisoned((rows, O)), _poisoned((rows, H2))
    batch._enqueue(lib.ccx_mlp_forward, rows, H1, H2, O, act, h1, p["w2t"], p["b2"], p["w3"], p["b3"], ny, n2)
    batch.synchronize()
    for a, b in ((y, ny), (h1, n1), (h2, n2)):
        np.testing.assert_array_equal(bits32c(_np(a)), bits32c(_np(b)))
    assert np.isnan(_np(y)).any()
    # the backward: CCX_MLP's on the last two layers, CCX_MLP_WIDE's (O := H2) on the first
    xb, hb1, hb2, gy = (_dev(c[k]) for k in ("x", "hidden1", "hidden2", "grad_y"))
    need = lib.ccx_mlp_deep_backward_workspace_bytes(rows, L, H1, H2, O)
    assert need == -(-rows // 256) * (L * H1 + H1 + H1 * H2 + H2 + O * H2 + O) * 8
    ws = _poisoned((need,), torch.uint8)
    g = [_poisoned(s) for s in ((L, H1), (H1,), (H1, H2), (H2,), (O, H2), (O,), (rows, H1), (rows, H2))]
    batch._enqueue(lib.ccx_mlp_deep_backward, rows, L, H1, H2, O, act, xb, hb1, hb2, gy, p["w2t"], p["w3"], ws, *g)
    ws2 = _poisoned((lib.ccx_mlp_backward_workspace_bytes(rows, H1, H2, O),), torch.uint8)
    last = [_poisoned(s) for s in ((H1, H2), (H2,), (O, H2), (O,), (rows, H2))]
    batch._enqueue(lib.ccx_mlp_backward, rows, H1, H2, O, act, hb1, hb2, gy, p["w3"], ws2, *last)
    ws1 = _poisoned((lib.ccx_mlp_wide_backward_workspace_bytes(rows, L, H1, H2),), torch.uint8)
    first = [_poisoned(s) for s in ((L, H1), (H1,), (H2, H1), (H2,), (rows, H1))]
    w2 = p["w2t"].t().contiguous()
    batch._enqueue(lib.ccx_mlp_wide_backward, rows, L, H1, H2, act, xb, hb1, g[7], w2, ws1, *first)
    batch.synchronize()
    for a, b in ((g[2], last[0]), (g[3], last[1]), (g[4], last[2]), (g[5], last[3]), (g[7], last[4]), (g[0], first[0]), (g[1], first[1]),
                 (g[6], first[4])):
        np.testing.assert_array_equal(bits32(_np(a)), bits32(_np(b)))
        assert np.isfinite(_np(a)).all()


# ------------------------------------------------------------------------------------------------- 4. the fused actor launches
def _stepped(batch, steps=9):
    batch.reset_from_pool()
    batch.set_rng_seed(SEED)
    batch.rollout_greedy(steps, want_obs=False)
    state = batch.get_state()
    return batch.observe(), batch.action_masks(), (state["terminated"] | state["truncated"]) != 0


def _actor(batch, H1, H2, O, act, seed=3, scale=4.0):
    """A head whose outputs spread enough for every action to be taken."""
    import torch

    from collectivecrossing_amd import DeepMlpHead

    torch.manual_seed(seed)
    head = DeepMlpHead(batch, H1, H2, O, ACT[act])
    with torch.no_grad():
        head.w3.mul_(scale)
        head.w1t.mul_(0.25)
    return head


@pytest.mark.parametrize("N,E,H1,H2,act", ((8, 96, 64, 64, TANH), (3, 5, 16, 32, RELU), (3, 22, 16, 32, TANH), (8, 8, 48, 16, TANH)))
def test_fused_sampling_equals_the_two_launches(batches, N, E, H1, H2, act):
    import torch

    batch = batches(N, E)
    assert batch.obs_len in AGENTS_OF_L and AGENTS_OF_L[batch.obs_len] == N
    obs, masks, dead = _stepped(batch)
    head = _actor(batch, H1, H2, 5, act)
    seen = set()
    for masked, det in itertools.product((True, False), (False, True)):
        m = masks if masked else None
        lo = _poisoned((E, N, 5))
        fused = head.sample_actions(obs, m, deterministic=det, want_logp=True, want_entropy=True, logits_out=lo)
        with torch.no_grad():
            logits = head(obs)
        two = batch.sample_actions(logits, m, deterministic=det, want_logp=True, want_entropy=True)
        bare = head.sample_actions(obs, m, deterministic=det, want_logp=False)      # the instantiations without statistics
        only_logp = head.sample_actions(obs, m, deterministic=det)
        batch.synchronize()
        tag = f"masked {masked} det {det}"
        np.testing.assert_array_equal(bits32(_np(lo)), bits32(_np(logits)), err_msg=f"logits_out {tag}")
        for name in ("actions", "logp", "entropy"):
            np.testing.assert_array_equal(bits32(_np(getattr(fused, name))), bits32(_np(getattr(two, name))), err_msg=f"{name} {tag}")
        assert bare.logp is None and bare.entropy is None and only_logp.entropy is None
        np.testing.assert_array_equal(_np(bare.actions), _np(two.actions), err_msg=f"no statistics {tag}")
        np.testing.assert_array_equal(bits32(_np(only_logp.logp)), bits32(_np(two.logp)))
        acts = _np(two.actions)
        assert (acts[dead] == 255).all() and (acts[~dead] < 5).all()
        seen |= set(np.unique(acts).tolist())
    assert E * N < 512 or seen >= {0, 1, 2, 3, 4}


@pytest.mark.parametrize("N,E,H1,H2,O,act", ((8, 9, 64, 64, 5, TANH), (3, 22, 16, 32, 5, RELU), (8, 9, 48, 16, 6, TANH), (3, 21, 16, 32, 6, TANH)))
def test_fused_q_actions_equal_the_kernels_composed(batches, N, E, H1, H2, O, act):
    import torch

    from collectivecrossing_amd import QLearning

    batch = batches(N, E)
    obs, masks, dead = _stepped(batch)
    ql = QLearning(batch)
    head = _actor(batch, H1, H2, O, act, seed=10 * N + O)
    explored_any = False
    for masked, eps in itertools.product((True, False), (None, 0.0, 0.25, 1.0)):
        m = masks if masked else None
        tag = f"masked {masked} eps {eps}"
        if eps is not None:
            ql.epsilon = eps
        out = ql.alloc_q_actions(want_explored=True)
        out.actions.fill_(0xEE)
        out.explored.fill_(0xEE)
        q_out = _poisoned((E, N, 5))
        fused = head.q_actions(ql, obs, m, greedy=eps is None, q_out=q_out, out=out)
        assert fused is out
        bare = head.q_actions(ql, obs, m, greedy=eps is None)             # no explored, no q_out
        with torch.no_grad():
            y = head(obs)
            q = ql.dueling(y) if O == 6 else y
        two = ql.q_actions(q, m, greedy=eps is None, want_explored=True)
        batch.synchronize()
        assert bare.explored is None
        np.testing.assert_array_equal(_np(fused.actions), _np(two.actions), err_msg="actions " + tag)
        np.testing.assert_array_equal(_np(fused.explored), _np(two.explored), err_msg="explored " + tag)
        np.testing.assert_array_equal(bits32(_np(q_out)), bits32(_np(q)), err_msg="q_out " + tag)
        np.testing.assert_array_equal(_np(bare.actions), _np(fused.actions), err_msg="bare " + tag)
        acts = _np(fused.actions)
        assert (acts[dead] == 255).all() and (acts[~dead] < 5).all() and not _np(fused.explored)[dead].any()
        explored_any |= bool(_np(fused.explored).any())
    assert explored_any


# ------------------------------------------------------------------------------------------------- 5. row independence
def test_a_rows_logits_do_not_depend_on_the_call_that_holds_it(batch):
    import torch

    L, H1, H2, O = 38, 64, 64, 5
    c = make_deep_case(8 * 64 * 8, L, H1, H2, O, seed=17, adversarial=False)
    head = _head(batch, c, L, H1, H2, O, TANH)
    x = _dev(c["x"]).view(8, 64, 8, L)
    n = 8 * 64 * 8
    perm = torch.randperm(n, generator=torch.Generator().manual_seed(5)).cuda()
    with torch.no_grad():
        whole = head(x)
        assert tuple(whole.shape) == (8, 64, 8, O)
        flat = whole.reshape(n, O)
        for cuts in ((1, n - 1), (63, 65, n - 128), (n // 2, n // 2), (129, n - 129)):
            parts, at = [], 0
            for k in cuts:
                parts.append(head(x.view(n, L)[at:at + k].clone()))
                at += k
            assert torch.equal(torch.cat(parts).view(torch.int32), flat.view(torch.int32)), cuts
        shuffled = head(x.view(n, L)[perm].contiguous())
        back = torch.empty_like(shuffled)
        back[perm] = shuffled
        assert torch.equal(back.view(torch.int32), flat.view(torch.int32))
    batch.synchronize()


# ------------------------------------------------------------------------------------------------- 6. the Python layer
def _seq_grads(seq):
    return [seq[0].weight.grad.t().double(), seq[0].bias.grad.double(), seq[2].weight.grad.t().double(), seq[2].bias.grad.double(),
            seq[4].weight.grad.double(), seq[4].bias.grad.double()]


@pytest.mark.parametrize("act", ("tanh", "relu"))
def test_autograd_in_both_modes(batch, act):
    """``backward="torch"`` is held to the f32 Sequential's own error against f64 autograd (the same f32 arithmetic in another
    summation order: at most 4 x as much, per parameter, maximum norm); ``"device"`` gives ``param_grads``' bits."""
    import torch

    from collectivecrossing_amd import DeepMlpHead

    torch.manual_seed(11)
    head = DeepMlpHead(batch, 64, 48, 5, act)
    L = head.L
    x = torch.randn((300, L), device="cuda")
    coef = torch.randn((300, 5), device="cuda")
    with torch.no_grad():
        h1, h2 = torch.empty((300, 64), device="cuda"), torch.empty((300, 48), device="cuda")
        plain = head(x, hidden1_out=h1, hidden2_out=h2)
    y = head(x)
    assert y.requires_grad and tuple(y.shape) == (300, 5)
    assert torch.equal(y.detach().view(torch.int32), plain.view(torch.int32))      # the same bits under grad
    (y * coef).sum().backward()
    ours = [p.grad.double() for p in head.parameters()]
    grads = {}
    for dtype in (torch.float64, torch.float32):
        seq = head.to_sequential(dtype)
        (seq(x.to(dtype)) * coef.to(dtype)).sum().backward()
        grads[dtype] = _seq_grads(seq)
    for name, g, g32, g64 in zip(NAMES, ours, grads[torch.float32], grads[torch.float64]):
        err, yard = float((g - g64).abs().max()), float((g32 - g64).abs().max())
        print(f"{act} grad {name}: max |ours - f64| = {err:.3e}, max |f32 Sequential - f64| = {yard:.3e}, max |f64| = {float(g64.abs().max()):.3e}")
        assert g.shape == g64.shape and err <= 4.0 * yard, name
    for kw in (dict(out=torch.empty((300, 5), device="cuda")), dict(hidden1_out=h1), dict(hidden2_out=h2)):
        with pytest.raises(ValueError):
            head(x, **kw)
    # the device backward: the bits of param_grads on the very gradient autograd hands over
    dev_head = DeepMlpHead(batch, 64, 48, 5, act, backward="device")
    dev_head.load_state_dict(head.state_dict())
    xg = x.clone().requires_grad_(True)
    (dev_head(xg) * coef).sum().backward()
    want = dev_head.param_grads(x, h1, h2, coef, want_grad_a=True)
    batch.synchronize()
    for name, p in zip(NAMES, dev_head.parameters()):
        assert torch.equal(p.grad.view(torch.int32), getattr(want, name).view(torch.int32)), name
    assert torch.equal(xg.grad, want.grad_a1 @ dev_head.w1t.detach().t())
    seq = head.to_sequential(torch.float64)
    x64 = x.double().requires_grad_(True)
    (seq(x64) * coef.double()).sum().backward()
    assert float((xg.grad.double() - x64.grad).abs().max()) <= 1e-5 * float(x64.grad.abs().max())


def test_static_buffers_capture_and_replay(batch):
    import torch

    from collectivecrossing_amd import DeepMlpHead

    torch.manual_seed(3)
    side = torch.cuda.Stream()
    batch.use_stream(side)
    torch.cuda.synchronize()
    try:
        with torch.cuda.stream(side):
            head = DeepMlpHead(batch, 64, 32, 5, "tanh")
            rows = (16, 8)
            x = torch.randn(rows + (head.L,), device="cuda")
            gy = torch.randn(rows + (5,), device="cuda")
            y, h1, h2 = (torch.empty(rows + (k,), device="cuda") for k in (5, 64, 32))
            out = head.alloc_param_grads(rows, want_grad_a=True)
            held = (y, h1, h2) + out.grads() + (out.grad_a1, out.grad_a2)

            def body():
                with torch.no_grad():
                    head(x, out=y, hidden1_out=h1, hidden2_out=h2)
                head.param_grads(x, h1, h2, gy, out=out)

            def snapshot():
                side.synchronize()
                return [t.clone() for t in held]

            body()
            eager = snapshot()
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph, stream=side):
                body()
            side.synchronize()
            for _ in range(2):
                for t in held:
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

    from collectivecrossing_amd import DeepMlpHead, DeviceAdam

    torch.manual_seed(2)
    seq = torch.nn.Sequential(torch.nn.Linear(38, 32), torch.nn.ReLU(), torch.nn.Linear(32, 48), torch.nn.ReLU(), torch.nn.Linear(48, 6)).cuda()
    head = DeepMlpHead.from_linear(batch, seq[0], seq[2], seq[4], "relu")
    assert (head.L, head.H1, head.H2, head.O, head.activation) == (38, 32, 48, 6, "relu")
    for a, b in zip(seq.parameters(), head.to_sequential().parameters()):
        assert torch.equal(a, b)
    torch.manual_seed(7)
    fresh = DeepMlpHead(batch, 64, 64)
    torch.manual_seed(7)
    ref = torch.nn.Sequential(torch.nn.Linear(38, 64), torch.nn.Tanh(), torch.nn.Linear(64, 64), torch.nn.Tanh(), torch.nn.Linear(64, 5))
    for mine, theirs in ((fresh.w1t, ref[0].weight.t()), (fresh.b1, ref[0].bias), (fresh.w2t, ref[2].weight.t()), (fresh.b2, ref[2].bias),
                         (fresh.w3, ref[4].weight), (fresh.b3, ref[4].bias)):
        assert torch.equal(mine.cpu(), theirs)                            # initialised as three Linear layers drawn in order
    x = torch.randn((300, 38), device="cuda")
    with torch.no_grad():
        y = fresh(x)
        assert float((y - ref.cuda()(x)).abs().max()) < 1e-5
    with pytest.raises(ValueError):
        DeepMlpHead.from_linear(batch, seq[0], seq[4], seq[2])
    # a checkpoint: through a file on the CPU into a new head
    buf = io.BytesIO()
    torch.save(fresh.state_dict(), buf)
    buf.seek(0)
    sd = torch.load(buf, map_location="cpu")
    assert sorted(sd) == sorted(NAMES) and all(not t.is_cuda for t in sd.values())
    other = DeepMlpHead(batch, 64, 64, backward="device")
    other.load_state_dict(sd)
    with torch.no_grad():
        assert torch.equal(other(x).view(torch.int32), y.view(torch.int32))
    shapes = [(38, 64), (64,), (64, 64), (64,), (5, 64), (5,)]
    assert [tuple(p.shape) for p in DeviceAdam(batch, other.parameters()).params] == shapes
    batch.synchronize()


def test_zero_rows_and_refusals_leave_the_batch_usable(batch):
    import torch

    from collectivecrossing_amd import DeepMlpHead, QLearning, _abi

    L, H1, H2, O = batch.obs_len, 64, 32, 5
    E, N = batch.num_envs, batch.num_agents
    head = DeepMlpHead(batch, H1, H2, O)
    x = torch.randn((E, N, L), device="cuda")
    # zero rows: empty tensors, zero gradients, no library call
    with torch.no_grad():
        empty = head(torch.empty((0, L), device="cuda"))
        empty2 = head(torch.empty((3, 0, L), device="cuda"))
    assert tuple(empty.shape) == (0, O) and tuple(empty2.shape) == (3, 0, O)
    assert tuple(head(torch.empty((0, L), device="cuda")).shape) == (0, O)                        # under grad too
    z = head.param_grads(*(torch.empty((0, k), device="cuda") for k in (L, H1, H2, O)))
    assert all(not getattr(z, n).any() for n in NAMES)
    # the wrapper's refusals
    shifted = torch.empty(E * N * L + 1, dtype=torch.float32, device="cuda")[1:].view(E, N, L)
    assert shifted.is_contiguous() and shifted.data_ptr() % 16
    for bad in (x.double(), x.half(), x[..., :-1], x[..., :-1].contiguous(), x.transpose(0, 1), x.cpu(), shifted, x.cpu().numpy()):
        with pytest.raises(ValueError):
            with torch.no_grad():
                head(bad)
        with pytest.raises(ValueError):
            head.sample_actions(bad)
    with torch.no_grad():
        for kw in (dict(out=torch.empty((E, N, 4), device="cuda")), dict(out=torch.empty((E, N, O), dtype=torch.float64, device="cuda")),
                   dict(hidden1_out=torch.empty((E, N, H2), device="cuda")), dict(hidden2_out=torch.empty((E, N, H1), device="cuda")),
                   dict(hidden1_out=torch.empty(E * N * H1 + 1, device="cuda")[1:].view(E, N, H1)),
                   dict(hidden2_out=torch.empty(E * N * H2 + 1, device="cuda")[1:].view(E, N, H2))):
            with pytest.raises(ValueError):
                head(x, **kw)
    for kw in (dict(H1=24, H2=16), dict(H1=16, H2=24), dict(H1=8, H2=16), dict(H1=16, H2=272), dict(H1=64, H2=64, O=9), dict(H1=64, H2=64, O=0),
               dict(H1=64, H2=64, L=513), dict(H1=64, H2=64, L=0), dict(H1=64, H2=64, activation="gelu"), dict(H1=64, H2=64, backward="jax"),
               dict(H1=64, H2=64, O=True), dict(H1=64.0, H2=64)):
        with pytest.raises(ValueError):
            DeepMlpHead(batch, **kw)
    with pytest.raises(ValueError):
        DeepMlpHead("batch", 64, 64)
    ql = QLearning(batch)
    critic, long_head = DeepMlpHead(batch, 16, 16, 1), DeepMlpHead(batch, 16, 16, 5, L=L + 1)
    for bad_head in (critic, long_head):
        with pytest.raises(ValueError):
            bad_head.sample_actions(x)
        with pytest.raises(ValueError):
            bad_head.q_actions(ql, x)
    for kw in (dict(masks=torch.zeros((E, N), device="cuda")), dict(logits_out=torch.empty((E, N, 4), device="cuda")), dict(out=(1, 2))):
        with pytest.raises(ValueError):
            head.sample_actions(x, **kw)
    for kw in (dict(masks=torch.zeros((E, N), device="cuda")), dict(q_out=torch.empty((E, N, 6), device="cuda")), dict(out=(1, 2))):
        with pytest.raises(ValueError):
            head.q_actions(ql, x, **kw)
    with pytest.raises(ValueError):
        head.q_actions("ql", x)
    h1, h2, gy = (torch.randn((E, N, k), device="cuda") for k in (H1, H2, O))
    good = head.param_grads(x, h1, h2, gy)
    for kw in (dict(x=shifted), dict(hidden1=h1[..., :-1].contiguous()), dict(hidden2=h2.double()), dict(hidden2=h1), dict(grad_y=gy[..., :-1].contiguous()),
               dict(grad_y=gy.cpu()), dict(out=(1, 2)), dict(workspace=torch.empty(8, dtype=torch.uint8, device="cuda")),
               dict(workspace=torch.empty(10**6, dtype=torch.float32, device="cuda"))):
        with pytest.raises(ValueError):
            head.param_grads(**{**dict(x=x, hidden1=h1, hidden2=h2, grad_y=gy), **kw})
    small = head.alloc_param_grads((E, N))
    small.workspace = small.workspace[:-8]
    with pytest.raises(ValueError):
        head.param_grads(x, h1, h2, gy, out=small)                        # its workspace is eight bytes short
    # the library's own refusals (the wrapper refuses first, so they are reached through the bindings)
    lib, h = batch._lib, batch._h
    rows = E * N
    y = torch.empty((rows, O), device="cuda")
    p = [t.data_ptr() for t in (x, head.w1t, head.b1, head.w2t, head.b2, head.w3, head.b3, y)]
    d = (L, H1, H2, O, 0)
    for args, word in (((None, rows, *d, *p, None, None), "NULL handle"), ((h, rows, *d, None, *p[1:], None, None), "NULL"),
                       ((h, rows, *d, *p[:7], None, None, None), "NULL"), ((h, 0, *d, *p, None, None), "rows"),
                       ((h, rows, L, 24, H2, O, 0, *p, None, None), "H1 = 24"), ((h, rows, L, H1, 8, O, 0, *p, None, None), "H2 = 8"),
                       ((h, rows, L, H1, H2, 9, 0, *p, None, None), "O = 9"), ((h, rows, 0, H1, H2, O, 0, *p, None, None), "L = 0"),
                       ((h, rows, L, H1, H2, O, 2, *p, None, None), "activation"), ((h, rows, *d, shifted.data_ptr(), *p[1:], None, None), "aligned"),
                       ((h, rows, *d, *p[:7], y.data_ptr() + 2, None, None), "aligned"), ((h, rows, *d, *p, h1.data_ptr() + 4, None), "aligned"),
                       ((h, rows, *d, *p, None, h2.data_ptr() + 8), "aligned")):
        assert lib.ccx_mlp_deep_forward(*args) == _abi.EINVAL, args
        assert word in lib.ccx_last_error().decode(), (word, lib.ccx_last_error())
    acts = torch.empty((E, N), dtype=torch.uint8, device="cuda")
    s = [t.data_ptr() for t in (x, head.w1t, head.b1, head.w2t, head.b2, head.w3, head.b3)]
    for args, word in (((None, H1, H2, 0, *s, None, 0, acts.data_ptr(), None, None, None), "NULL handle"),
                       ((h, H1, H2, 0, *s, None, 0, None, None, None, None), "NULL"), ((h, 24, H2, 0, *s, None, 0, acts.data_ptr(), None, None, None), "H1 = 24"),
                       ((h, H1, H2, 5, *s, None, 0, acts.data_ptr(), None, None, None), "activation"),
                       ((h, H1, H2, 0, shifted.data_ptr(), *s[1:], None, 0, acts.data_ptr(), None, None, None), "aligned"),
                       ((h, H1, H2, 0, *s, None, 0, acts.data_ptr(), y.data_ptr() + 2, None, None), "aligned")):
        assert lib.ccx_mlp_deep_sample_actions(*args) == _abi.EINVAL, args
        assert word in lib.ccx_last_error().decode(), (word, lib.ccx_last_error())
    for args, word in (((None, H1, H2, 0, 5, *s, None, None, acts.data_ptr(), None, None), "NULL handle"),
                       ((h, H1, H2, 0, 5, *s[:6], None, None, None, acts.data_ptr(), None, None), "NULL"),
                       ((h, H1, H2, 0, 7, *s, None, None, acts.data_ptr(), None, None), "O = 7"), ((h, H1, 272, 0, 5, *s, None, None, acts.data_ptr(), None, None), "H2 = 272"),
                       ((h, H1, H2, 0, 5, shifted.data_ptr(), *s[1:], None, None, acts.data_ptr(), None, None), "aligned"),
                       ((h, H1, H2, 0, 5, *s, None, y.data_ptr() + 2, acts.data_ptr(), None, None), "aligned")):
        assert lib.ccx_mlp_deep_q_actions(*args) == _abi.EINVAL, args
        assert word in lib.ccx_last_error().decode(), (word, lib.ccx_last_error())
    ws = torch.empty(lib.ccx_mlp_deep_backward_workspace_bytes(rows, L, H1, H2, O) + 8, dtype=torch.uint8, device="cuda")
    g = [t.data_ptr() for t in (x, h1, h2, gy, head.w2t, head.w3, ws) + good.grads()]
    for args, word in (((None, rows, *d, *g, None, None), "NULL handle"), ((h, rows, *d, *g[:6], None, *g[7:], None, None), "NULL"),
                       ((h, rows, *d, *g[:12], None, None, None), "NULL"), ((h, 0, *d, *g, None, None), "rows"),
                       ((h, rows, L, H1, H2, 9, 0, *g, None, None), "O = 9"), ((h, rows, L, 8, H2, O, 0, *g, None, None), "H1 = 8"),
                       ((h, rows, L, H1, H2, O, 3, *g, None, None), "activation"), ((h, rows, *d, g[0], g[1] + 4, *g[2:], None, None), "16-byte"),
                       ((h, rows, *d, *g[:2], g[2] + 8, *g[3:], None, None), "16-byte"), ((h, rows, *d, *g[:6], g[6] + 4, *g[7:], None, None), "8-byte"),
                       ((h, rows, *d, *g[:3], g[3] + 2, *g[4:], None, None), "4-byte"), ((h, rows, *d, *g, h1.data_ptr() + 8, None), "16-byte"),
                       ((h, rows, *d, *g, None, h2.data_ptr() + 4), "16-byte")):
        assert lib.ccx_mlp_deep_backward(*args) == _abi.EINVAL, args
        assert word in lib.ccx_last_error().decode(), (word, lib.ccx_last_error())
    assert lib.ccx_mlp_deep_backward_workspace_bytes(257, L, H1, H2, O) == 2 * (L * H1 + H1 + H1 * H2 + H2 + O * H2 + O) * 8
    assert lib.ccx_mlp_deep_backward_workspace_bytes(0, L, H1, H2, O) == 0 == lib.ccx_mlp_deep_backward_workspace_bytes(8, L, H1, H2, 9)
    again = head.param_grads(x, h1, h2, gy)
    batch.synchronize()
    for n in NAMES:
        assert torch.equal(getattr(again, n).view(torch.int32), getattr(good, n).view(torch.int32))


# ------------------------------------------------------------------------------------------------- 7. the example
def test_the_example_prints_zero_and_equal_bits():
    code = ("import sys; sys.path.insert(0, 'examples'); import ppo_deep as ex; "
            "gap, equal = ex.main(num_envs=16, iterations=2, steps=4); assert gap == 0.0 and equal; print('ok', gap, equal)")
    run = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True, timeout=300)
    print(run.stdout[-1500:])
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-4000:]
    assert "ok 0.0 True" in run.stdout
