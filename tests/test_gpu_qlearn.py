"""Q-learning on the device (include/ccx.h: CCX_QLEARN) against the NumPy spec (tests/_qlearn_spec.py): epsilon-greedy
actions on slot counts that straddle a wave, in a stepped and auto-reset state, eager and captured, with the rate changed
between replays; the TD loss, its ``td_error`` and its gradient on row counts that cross the group, block and final-wave
boundaries of the tree, for every NULL combination of the optional inputs; the autograd path down to an ``MlpHead``'s
parameters; the static-buffer pair in a replayed graph; the refusals; and the example's loop, twice.  f32 values are compared
as bit patterns throughout."""

import ctypes as C
import importlib.util
from pathlib import Path

import numpy as np
import pytest
from _qlearn_spec import TD_VARIANTS, make_q_case, make_td_case, q_actions_spec, td_args, td_loss_backward_spec, td_loss_spec
from _reset_obs_spec import make_config
from _sample_spec import bits32

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
SEED = 0x0123_4567_89AB_CDEF
SENTINEL = 0xEE
ROWS = (1, 63, 64, 65, 255, 256, 257, 1023, 16385, 16389)
GAMMA, DELTA = 0.97, 1.0
KEYS = ("q", "actions", "reward", "done", "q_next_target", "q_next_online", "masks_next", "valid", "weights")


@pytest.fixture(scope="module")
def batches():
    import torch

    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    from collectivecrossing_amd.batched import BatchedCollectiveCrossing

    made = []

    def new(N, E, **kw):
        b = BatchedCollectiveCrossing(make_config(N, max_steps=12), E, **kw)
        assert b.num_agents == N
        made.append(b)
        return b

    yield new
    for b in made:
        b.close()


@pytest.fixture(scope="module")
def ql8(batches):
    """One 8-agent batch and its QLearning for the row-wise tests (they never read the env state)."""
    from collectivecrossing_amd import QLearning

    b = batches(8, 4)
    return b, QLearning(b)


@pytest.fixture(scope="module")
def td_case():
    return make_td_case(max(ROWS), seed=41, huber_delta=DELTA)


def _cuda(kw):
    import torch

    return {k: None if v is None else torch.from_numpy(v).cuda() for k, v in kw.items()}


# ------------------------------------------------------------------------------------------------- 1. q_actions: bits
@pytest.mark.parametrize("N,E", [(3, 21), (3, 22), (8, 8), (8, 9)])      # 63 / 66 and 64 / 72 slots: around one wave
def test_q_actions_bits_in_a_stepped_state(batches, N, E):
    import torch

    from collectivecrossing_amd import QLearning

    batch = batches(N, E)
    batch.make_reset_pool(seed0=7, size=64)
    batch.reset_from_pool()
    batch.set_rng_seed(SEED)
    rng = np.random.default_rng(N * 100 + E)
    # 17 steps with auto-reset at max_steps = 12: a second episode, five steps in, with agents that have arrived
    batch.rollout(torch.from_numpy(rng.integers(0, 5, size=(17, E, N), dtype=np.uint8)).cuda(), auto_reset=True, want_traj=False)
    case = make_q_case(E, N, seed=E * 100 + N)
    st = batch.get_state()
    assert (st["episode"] >= 1).all() and (st["step_count"] > 0).all()
    half = np.arange(E) % 2 == 1                                         # every other env: the generator's far counters
    batch.set_state(terminated=st["terminated"] | case["terminated"], truncated=st["truncated"] | case["truncated"],
                    step_count=np.where(half, case["step_count"], st["step_count"]).astype(np.int32),
                    episode=np.where(half, case["episode"], st["episode"]).astype(np.int32))
    st = batch.get_state()
    state = (st["terminated"], st["truncated"], st["step_count"], st["episode"])
    dead = (st["terminated"] | st["truncated"]) != 0
    assert dead.any() and not dead.all() and len(np.unique(st["step_count"])) > 2 and len(np.unique(st["episode"])) > 2
    ql = QLearning(batch)
    d = {k: torch.from_numpy(np.ascontiguousarray(case[k])).cuda() for k in ("q", "q_masked", "masks")}
    for masked in (True, False):
        q, masks = (d["q_masked"], d["masks"]) if masked else (d["q"], None)
        q_np, masks_np = (case["q_masked"], case["masks"]) if masked else (case["q"], None)
        for eps in (None, 0.0, 0.25, 1.0):
            for want_explored in (True, False):
                out = ql.alloc_q_actions(want_explored)
                out.actions.fill_(SENTINEL)
                if want_explored:
                    out.explored.fill_(SENTINEL)
                if eps is not None:
                    ql.epsilon = eps
                got = ql.q_actions(q, masks, greedy=eps is None, out=out)
                assert got is out
                batch.synchronize()
                want = q_actions_spec(q_np, masks_np, *state, seed=SEED, epsilon=eps)
                tag = f"N {N} E {E} masked {masked} eps {eps}"
                np.testing.assert_array_equal(out.actions.cpu().numpy(), want[0], err_msg="actions " + tag)
                assert (want[0][dead] == 255).all() and (want[0][~dead] <= 4).all()
                if want_explored:
                    np.testing.assert_array_equal(out.explored.cpu().numpy(), want[1], err_msg="explored " + tag)
                    assert not want[1][dead].any() and (eps != 1.0 or want[1][~dead].all()) and (eps or not want[1].any())
    res = ql.q_actions(d["q_masked"], d["masks"], want_explored=True)    # fresh tensors, the rate of the last setting (1.0)
    batch.synchronize()
    np.testing.assert_array_equal(res.actions.cpu().numpy(), q_actions_spec(case["q_masked"], case["masks"], *state, seed=SEED, epsilon=1.0)[0])


# ------------------------------------------------------------------------------------------------- 2. q_actions: a loop
C1 = np.array([0.37, -0.21, 0.11, 0.29, -0.13], np.float32)
C2 = np.array([0.19, 0.23, -0.31, 0.07, 0.17], np.float32)
LOOP_E, LOOP_N, LOOP_K = 64, 8, 24
RATES = [1.0] * 6 + [0.0] * 6 + [0.3] * 12                               # the rate of every step: it changes between replays


def test_actor_loop_eager_and_captured_with_a_changing_rate():
    import torch

    from collectivecrossing_amd import QLearning
    from collectivecrossing_amd.batched import BatchedCollectiveCrossing
    from collectivecrossing_amd.qlearn import QActions

    E, N, K = LOOP_E, LOOP_N, LOOP_K
    env = BatchedCollectiveCrossing(make_config(N, max_steps=12), E)
    env.make_reset_pool(seed0=5, size=256)
    env.reset_from_pool()
    env.set_rng_seed(SEED)
    start = env.get_state()
    c1, c2 = torch.from_numpy(C1).cuda(), torch.from_numpy(C2).cuda()
    side = torch.cuda.Stream()
    env.use_stream(side)
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        ql = QLearning(env)
        obs, masks = env.observe(), env.action_masks()
        actions = torch.empty((1, E, N), dtype=torch.uint8, device="cuda")
        chosen = QActions(actions[0], torch.empty((E, N), dtype=torch.uint8, device="cuda"))
        out = env.alloc_rollout(1)

        def body():
            q = obs[..., 0:5] * c1 - obs[..., 5:10] * c2
            ql.q_actions(q, masks, out=chosen)
            env.rollout(actions, auto_reset=True, out=out, masks_out=masks, reset_obs="next")
            obs.copy_(out.obs[0])

        def run(step, check):
            hist = dict(actions=[], explored=[])
            for s in range(K):
                ql.epsilon = RATES[s]
                if check:                                                # the spec on the state, rows and masks of this step
                    side.synchronize()
                    st, o = env.get_state(), obs.cpu().numpy()
                    want = q_actions_spec(o[..., 0:5] * C1 - o[..., 5:10] * C2, masks.cpu().numpy(), st["terminated"], st["truncated"],
                                          st["step_count"], st["episode"], seed=SEED, epsilon=RATES[s])
                step()
                side.synchronize()
                hist["actions"].append(actions[0].cpu().numpy())
                hist["explored"].append(chosen.explored.cpu().numpy())
                if check:
                    np.testing.assert_array_equal(hist["actions"][-1], want[0], err_msg=f"step {s}")
                    np.testing.assert_array_equal(hist["explored"][-1], want[1], err_msg=f"step {s}")
            return {k: np.stack(v) for k, v in hist.items()}

        eager = run(body, check=True)
        live = eager["actions"] != 255
        assert (eager["explored"][:6] == 1)[live[:6]].all() and not eager["explored"][6:12].any()
        assert 0.15 < eager["explored"][12:][live[12:]].mean() < 0.45 and (~live).any()
        assert env.get_state()["episode"].max() >= 1                     # an auto-reset happened on the way
        # the same loop from the same start, captured once and replayed: the rate is read from the device when a replay runs
        env.set_state(**start)
        env.observe(out=obs)
        env.action_masks(out=masks)
        side.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            body()
        side.synchronize()
        replayed = run(graph.replay, check=False)
        for k in eager:
            np.testing.assert_array_equal(replayed[k], eager[k], err_msg=f"graph replay: {k}")
    env.use_stream(None)
    env.close()


# ------------------------------------------------------------------------------------------------- 3. td_loss: bits
def _forward(ql, d, M, want_td=True, **hyper):
    import torch

    out = ql.alloc_td_loss((M,), want_td_error=want_td)
    for t in (out.stats, out.td_error, out.grad_q):
        if t is not None:
            t.view(torch.uint8).fill_(SENTINEL)
    got = ql.td_loss(*(d[k] for k in KEYS), **hyper, out=out)
    assert got is out
    return out


@pytest.mark.parametrize("M", ROWS)
def test_td_loss_bits_every_optional_input(ql8, td_case, M):
    import torch

    batch, ql = ql8
    gloss = torch.tensor([-1.75], device="cuda")
    hyper = dict(gamma=GAMMA, huber_delta=DELTA)
    for variant in TD_VARIANTS:
        tag = f"M {M} masked {variant[0]} double {variant[1]} valid {variant[2]} weights {variant[3]}"
        kw = td_args(td_case, *variant, M=M)
        d = _cuda(kw)
        want_stats, want_td, t = td_loss_spec(**kw, **hyper, details=True)
        out = _forward(ql, d, M, **hyper)
        grads = [ql.td_loss_backward(*(d[k] for k in KEYS), **hyper, stats=out.stats, grad_loss=gl, out=o)
                 for gl, o in ((None, out), (gloss, None))]
        batch.synchronize()
        np.testing.assert_array_equal(bits32(out.stats.cpu().numpy()), bits32(want_stats), err_msg="stats " + tag)
        np.testing.assert_array_equal(bits32(out.td_error.cpu().numpy()), bits32(want_td), err_msg="td_error " + tag)
        assert grads[0] is out.grad_q
        for g, gl in zip(grads, (None, -1.75)):
            want = td_loss_backward_spec(**kw, **hyper, stats=want_stats, grad_loss=gl)
            np.testing.assert_array_equal(bits32(g.cpu().numpy()), bits32(want), err_msg=f"grad_q {gl} " + tag)
            assert not bits32(want)[~t["counts"]].any() and np.isfinite(want).all()
        if M >= 255:                                                     # rows that do not count are NaN-filled
            assert np.isnan(kw["q"][~t["counts"]]).any() and np.isnan(kw["reward"][~t["counts"]]).any()
    # without td_error, other hyper-parameters, and no row that counts
    kw = td_args(td_case, True, True, True, True, M=M)
    d = _cuda(kw)
    for hy in (dict(gamma=0.0, huber_delta=0.5), dict(gamma=1.0, huber_delta=float("inf"))):
        out = _forward(ql, d, M, want_td=False, **hy)
        g = ql.td_loss_backward(*(d[k] for k in KEYS), **hy, stats=out.stats)
        batch.synchronize()
        want_stats, _ = td_loss_spec(**kw, **hy)
        np.testing.assert_array_equal(bits32(out.stats.cpu().numpy()), bits32(want_stats), err_msg=str(hy))
        np.testing.assert_array_equal(bits32(g.cpu().numpy()), bits32(td_loss_backward_spec(**kw, **hy, stats=want_stats)))
    d["valid"] = torch.zeros_like(d["valid"])
    out = _forward(ql, d, M, **hyper)
    g = ql.td_loss_backward(*(d[k] for k in KEYS), **hyper, stats=out.stats, out=out)
    batch.synchronize()
    assert not out.stats.view(torch.int32).any() and not out.td_error.view(torch.int32).any() and not g.view(torch.int32).any()


def test_leading_shapes_and_zero_rows(ql8, td_case):
    import torch

    batch, ql = ql8
    kw = td_args(td_case, True, True, True, True, M=6 * 8 * 8)
    d = {k: v.reshape((6, 8, 8) + tuple(v.shape[1:])) for k, v in _cuda(kw).items()}
    r = ql.td_loss(*(d[k] for k in KEYS), gamma=GAMMA, want_td_error=True)
    g = ql.td_loss_backward(*(d[k] for k in KEYS), gamma=GAMMA, stats=r.stats)
    batch.synchronize()
    want_stats, want_td = td_loss_spec(**kw, gamma=GAMMA)
    np.testing.assert_array_equal(bits32(r.stats.cpu().numpy()), bits32(want_stats))
    assert r.loss.dim() == 0 and r.td_error.shape == (6, 8, 8) and g.shape == (6, 8, 8, 5) and r.workspace is None
    np.testing.assert_array_equal(bits32(r.td_error.cpu().numpy().reshape(-1)), bits32(want_td))
    np.testing.assert_array_equal(bits32(g.cpu().numpy().reshape(-1, 5)), bits32(td_loss_backward_spec(**kw, gamma=GAMMA, stats=want_stats)))
    e = {k: v[:0] for k, v in d.items()}
    r = ql.td_loss(*(e[k] for k in KEYS), want_td_error=True)
    assert not r.stats.any() and r.td_error.shape == (0, 8, 8)
    assert ql.td_loss_backward(*(e[k] for k in KEYS), stats=r.stats).shape == (0, 8, 8, 5)


# ------------------------------------------------------------------------------------------------- 4. autograd
def test_autograd_reaches_q_and_the_parameters_of_a_head(ql8, td_case):
    import torch

    batch, ql = ql8
    M = 1023
    kw = td_args(td_case, True, True, True, True, M=M)
    d = _cuda(kw)
    static = _forward(ql, d, M, gamma=GAMMA)
    want = ql.td_loss_backward(*(d[k] for k in KEYS), gamma=GAMMA, stats=static.stats)
    q = d["q"].clone().requires_grad_()
    r = ql.td_loss(q, *(d[k] for k in KEYS[1:]), gamma=GAMMA, want_td_error=True)
    assert r.loss.requires_grad and not r.stats.requires_grad
    r.loss.backward()
    batch.synchronize()
    assert torch.equal(r.stats.view(torch.int32), static.stats.view(torch.int32))
    assert torch.equal(r.td_error.view(torch.int32), static.td_error.view(torch.int32))
    assert torch.equal(q.grad.view(torch.int32), want.view(torch.int32)) and q.grad.abs().sum() > 0
    with pytest.raises(ValueError, match="out="):
        ql.td_loss(q, *(d[k] for k in KEYS[1:]), out=static)
    for name in ("q_next_target", "q_next_online"):
        bad = dict(d, q=q)
        bad[name] = torch.zeros_like(d[name]).requires_grad_()
        with pytest.raises(ValueError, match="must not require a gradient"):
            ql.td_loss(*(bad[k] for k in KEYS))
    # through a head with the device backward: the parameters' gradients are mlp_backward's on the same grad_q, bit for bit
    torch.manual_seed(3)
    head = batch.mlp_head(16, backward="device")
    x = torch.randn((M, head.L), device="cuda")
    clean = {k: (None if v is None else torch.nan_to_num(v, nan=0.25) if v.is_floating_point() else v) for k, v in d.items()}
    r = ql.td_loss(head(x), *(clean[k] for k in KEYS[1:]), gamma=GAMMA)
    r.loss.backward()
    with torch.no_grad():
        hidden = torch.empty((M, head.H), device="cuda")
        qs = head(x, hidden_out=hidden)
        gq = ql.td_loss_backward(qs, *(clean[k] for k in KEYS[1:]), gamma=GAMMA, stats=r.stats)
        ref = batch.mlp_backward(head, x, hidden, gq)
    batch.synchronize()
    for p, g in zip((head.w1t, head.b1, head.w2, head.b2), (ref.w1t, ref.b1, ref.w2, ref.b2)):
        assert torch.equal(p.grad.view(torch.int32), g.view(torch.int32)) and torch.isfinite(p.grad).all() and p.grad.abs().sum() > 0


# ------------------------------------------------------------------------------------------------- 4b. the frame of the loss
FRAME_ROWS = (1, 63, 257, 513)                                           # inside a wave, across one, a block + a row, two + a row


@pytest.mark.parametrize("present", (False, True), ids=("optional-absent", "optional-present"))
@pytest.mark.parametrize("M", FRAME_ROWS)
def test_the_three_call_forms_agree(ql8, td_case, M, present):
    """Fresh outputs, ``out=`` of ``alloc_td_loss`` and autograd write the spec's bits, so the same ones; the gradient that
    ``r.loss.backward()`` leaves is ``td_loss_backward(out=)``'s with ``grad_loss`` absent and with a 1.0f."""
    import torch

    batch, ql = ql8
    hyper = dict(gamma=GAMMA, huber_delta=DELTA)
    kw = td_args(td_case, present, present, present, present, M=M)
    d = _cuda(kw)
    want_stats, want_td = td_loss_spec(**kw, **hyper)
    want_grad = td_loss_backward_spec(**kw, **hyper, stats=want_stats)
    fresh = ql.td_loss(*(d[k] for k in KEYS), **hyper, want_td_error=True)
    static = _forward(ql, d, M, **hyper)
    q = d["q"].clone().requires_grad_()
    auto = ql.td_loss(q, *(d[k] for k in KEYS[1:]), **hyper, want_td_error=True)
    auto.loss.backward()
    one = torch.ones(1, device="cuda")
    grads = [ql.td_loss_backward(*(d[k] for k in KEYS), **hyper, stats=static.stats, grad_loss=gl, out=o)
             for gl, o in ((None, static), (one, None))]
    batch.synchronize()
    assert fresh.workspace is None and auto.workspace is None and grads[0] is static.grad_q
    for form, r in (("fresh", fresh), ("out=", static), ("autograd", auto)):
        np.testing.assert_array_equal(bits32(r.stats.cpu().numpy()), bits32(want_stats), err_msg="stats " + form)
        np.testing.assert_array_equal(bits32(r.td_error.cpu().numpy()), bits32(want_td), err_msg="td_error " + form)
    for form, g in (("autograd", q.grad), ("grad_loss None", grads[0]), ("grad_loss 1.0f", grads[1])):
        np.testing.assert_array_equal(bits32(g.cpu().numpy()), bits32(want_grad), err_msg="grad_q " + form)


@pytest.mark.parametrize("why", ("valid all zero", "every action 255"))
def test_no_row_counts(ql8, td_case, why):
    """n = 0: the eight stats, every gradient element and td_error are +0.0f (all 32 bits clear), as the spec has them."""
    batch, ql = ql8
    M = 257
    hyper = dict(gamma=GAMMA, huber_delta=DELTA)
    kw = td_args(td_case, True, True, True, True, M=M)
    if why == "valid all zero":
        kw["valid"] = np.zeros(M, np.uint8)
    else:
        kw["actions"] = np.full(M, 255, np.uint8)
    d = _cuda(kw)
    want_stats, want_td = td_loss_spec(**kw, **hyper)
    want_grad = td_loss_backward_spec(**kw, **hyper, stats=want_stats)
    assert not bits32(want_stats).any() and not bits32(want_td).any() and not bits32(want_grad).any()
    out = _forward(ql, d, M, **hyper)                                    # (every output prefilled with a sentinel)
    g = ql.td_loss_backward(*(d[k] for k in KEYS), **hyper, stats=out.stats, out=out)
    batch.synchronize()
    assert out.stats.shape == (8,) and g.shape == (M, 5) and out.td_error.shape == (M,)
    for name, t in (("stats", out.stats), ("grad_q", g), ("td_error", out.td_error)):
        assert not bits32(t.cpu().numpy()).any(), name


def test_zero_rows_in_the_three_call_forms(ql8, td_case, monkeypatch):
    import torch

    batch, ql = ql8
    d = {k: v[:0] for k, v in _cuda(td_args(td_case, True, True, True, True, M=4)).items()}
    static = ql.alloc_td_loss((0,))
    static.stats.fill_(float("nan"))

    def called(*args, **kwargs):
        raise AssertionError("zero rows must not reach the library")

    monkeypatch.setattr(batch, "_enqueue", called)
    fresh = ql.td_loss(*(d[k] for k in KEYS), want_td_error=True)
    assert ql.td_loss(*(d[k] for k in KEYS), out=static) is static
    q = d["q"].clone().requires_grad_()
    auto = ql.td_loss(q, *(d[k] for k in KEYS[1:]), want_td_error=True)
    assert auto.loss.requires_grad and not auto.stats.requires_grad
    auto.loss.backward()
    for r in (fresh, static, auto):
        assert r.stats.shape == (8,) and not r.stats.view(torch.int32).any() and r.td_error.shape == (0,)
    assert q.grad.shape == (0, 5)
    assert ql.td_loss_backward(*(d[k] for k in KEYS), stats=static.stats, out=static) is static.grad_q


# ------------------------------------------------------------------------------------------------- 5. a replayed graph
def test_static_buffers_captured_and_replayed(td_case):
    import torch

    from collectivecrossing_amd import QLearning
    from collectivecrossing_amd.batched import BatchedCollectiveCrossing

    M = 1023
    env = BatchedCollectiveCrossing(make_config(8, max_steps=12), 4)
    side = torch.cuda.Stream()
    env.use_stream(side)
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        ql = QLearning(env)
        slices = [td_args({k: (v[o:] if isinstance(v, np.ndarray) else v) for k, v in td_case.items()}, True, True, True, True, M=M)
                  for o in (0, 2000, 7001)]
        d = _cuda(slices[0])
        out = ql.alloc_td_loss((M,))
        gloss = torch.tensor([0.5], device="cuda")
        side.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            ql.td_loss(*(d[k] for k in KEYS), gamma=GAMMA, out=out)
            ql.td_loss_backward(*(d[k] for k in KEYS), gamma=GAMMA, stats=out.stats, grad_loss=gloss, out=out)
        for kw in slices[::-1]:
            for k in KEYS:
                d[k].copy_(torch.from_numpy(kw[k]))
            for t in (out.stats, out.td_error, out.grad_q):
                t.view(torch.uint8).fill_(SENTINEL)
            graph.replay()
            side.synchronize()
            want_stats, want_td = td_loss_spec(**kw, gamma=GAMMA)
            np.testing.assert_array_equal(bits32(out.stats.cpu().numpy()), bits32(want_stats))
            np.testing.assert_array_equal(bits32(out.td_error.cpu().numpy()), bits32(want_td))
            np.testing.assert_array_equal(bits32(out.grad_q.cpu().numpy()),
                                          bits32(td_loss_backward_spec(**kw, gamma=GAMMA, stats=want_stats, grad_loss=0.5)))
    env.use_stream(None)
    env.close()


# ------------------------------------------------------------------------------------------------- 6. refusals
def test_refusals_leave_the_batch_usable(batches, td_case):
    import torch

    from collectivecrossing_amd import QLearning, _abi
    from collectivecrossing_amd.qlearn import QActions

    E, N, M = 21, 3, 257
    batch = batches(N, E)
    ql = QLearning(batch, epsilon=0.5)
    q = torch.zeros((E, N, 5), device="cuda")
    mk = torch.full((E, N), 0x1F, dtype=torch.uint8, device="cuda")
    shifted = torch.empty(E * N * 5 + 1, device="cuda")[1:].view(E, N, 5)
    assert shifted.is_contiguous() and shifted.data_ptr() % 16
    for kw in (dict(q=q.double()), dict(q=q.half()), dict(q=q[:-1]), dict(q=q.cpu()), dict(q=shifted), dict(q=None),
               dict(q=q.transpose(0, 1).contiguous().transpose(0, 1)), dict(q=q, masks=mk.int()), dict(q=q, masks=mk[:-1]),
               dict(q=q, out=(1, 2)), dict(q=q, out=QActions(torch.empty((E, N + 1), dtype=torch.uint8, device="cuda"), None)),
               dict(q=q, out=QActions(mk.clone(), torch.empty((E, N), dtype=torch.float32, device="cuda")))):
        with pytest.raises(ValueError):
            ql.q_actions(**kw)
    for eps in (-0.1, 1.5, float("nan"), "x"):
        with pytest.raises(ValueError):
            ql.epsilon = eps
        with pytest.raises(ValueError):
            QLearning(batch, epsilon=eps)
    assert ql.epsilon == 0.5
    with pytest.raises(ValueError):
        QLearning(object())
    d = _cuda(td_args(td_case, True, True, True, True, M=M))
    good = [d[k] for k in KEYS]
    stats = ql.td_loss(*good).stats
    shifted5 = torch.empty(M * 5 + 1, device="cuda")[1:].view(M, 5)
    swaps = [("q", d["q"].double()), ("q", shifted5), ("actions", d["actions"].long()), ("actions", d["actions"][:-1]),
             ("reward", d["reward"].float()), ("done", d["done"].bool()), ("q_next_target", shifted5), ("q_next_target", None),
             ("q_next_online", shifted5), ("q_next_online", d["q_next_online"].cpu()), ("masks_next", d["masks_next"].int()),
             ("valid", d["valid"].bool()), ("weights", d["weights"].double()), ("weights", d["weights"][:-1])]
    for name, bad in swaps:
        args = [bad if k == name else d[k] for k in KEYS]
        with pytest.raises(ValueError, match=name):
            ql.td_loss(*args)
        with pytest.raises(ValueError, match=name):
            ql.td_loss_backward(*args, stats=stats)
    for hy in (dict(gamma=-0.1), dict(gamma=1.5), dict(gamma=float("nan")), dict(huber_delta=0.0), dict(huber_delta=-1.0),
               dict(huber_delta=float("nan")), dict(gamma="x")):
        with pytest.raises(ValueError):
            ql.td_loss(*good, **hy)
        with pytest.raises(ValueError):
            ql.td_loss_backward(*good, **hy, stats=stats)
    for kw in (dict(out=(1,)), dict(out=ql.alloc_td_loss((M + 1,))), dict(out=batch.alloc_ppo_loss((M,)))):
        with pytest.raises(ValueError):
            ql.td_loss(*good, **kw)
    small = ql.alloc_td_loss((M,))
    small.workspace = small.workspace[:8]
    with pytest.raises(ValueError, match="workspace"):
        ql.td_loss(*good, out=small)
    for kw in (dict(stats=stats[:4]), dict(stats=stats, grad_loss=torch.ones(2, 2, device="cuda")), dict(stats=stats, out=shifted5),
               dict(stats=stats, grad_loss=torch.ones(1))):
        with pytest.raises(ValueError):
            ql.td_loss_backward(*good, **kw)
    # the library's own refusals (the wrapper refuses first, so they are reached through the bindings)
    lib, h = batch._lib, batch._h
    out = ql.alloc_td_loss((M,))
    ptr = [d[k].data_ptr() for k in KEYS]
    f = C.c_float

    def fwd(rows=M, p=ptr, gamma=0.99, delta=1.0, ws=out.workspace.data_ptr(), st=out.stats.data_ptr(), handle=h):
        return lib.ccx_td_loss(handle, rows, *p, f(gamma), f(delta), ws, st, out.td_error.data_ptr())

    def bwd(rows=M, p=ptr, gamma=0.99, delta=1.0, st=stats.data_ptr(), gq=out.grad_q.data_ptr(), handle=h):
        return lib.ccx_td_loss_backward(handle, rows, *p, f(gamma), f(delta), st, None, gq)

    assert fwd() == _abi.OK and bwd() == _abi.OK
    for call in (fwd, bwd):
        for kw, word in ((dict(gamma=-0.1), "gamma"), (dict(gamma=1.5), "gamma"), (dict(gamma=float("nan")), "gamma"),
                         (dict(gamma=float("inf")), "gamma"), (dict(delta=0.0), "huber_delta"), (dict(delta=-2.0), "huber_delta"),
                         (dict(delta=float("nan")), "huber_delta"), (dict(rows=0), "rows"), (dict(handle=None), "NULL handle"),
                         (dict(p=[None] + ptr[1:]), "NULL"), (dict(p=ptr[:4] + [None] + ptr[5:]), "NULL"), (dict(st=None), "NULL"),
                         (dict(p=[shifted5.data_ptr()] + ptr[1:]), "aligned"), (dict(p=ptr[:5] + [shifted5.data_ptr()] + ptr[6:]), "aligned")):
            assert call(**kw) == _abi.EINVAL, kw
            assert word in lib.ccx_last_error().decode(), (kw, lib.ccx_last_error())
    assert fwd(ws=None) == _abi.EINVAL and fwd(ws=out.workspace.data_ptr() + 4) == _abi.EINVAL
    assert "8-byte" in lib.ccx_last_error().decode()
    assert bwd(gq=None) == _abi.EINVAL and bwd(gq=shifted5.data_ptr()) == _abi.EINVAL
    assert fwd(delta=float("inf")) == _abi.OK and lib.ccx_td_workspace_bytes(0) == 0 and lib.ccx_td_workspace_bytes(257) == 2 * 6 * 8
    acts = torch.empty((E, N), dtype=torch.uint8, device="cuda")
    for args, word in (((None, q.data_ptr(), None, None, acts.data_ptr(), None), "NULL handle"), ((h, None, None, None, acts.data_ptr(), None), "NULL"),
                       ((h, q.data_ptr(), None, None, None, None), "NULL"), ((h, shifted.data_ptr(), None, None, acts.data_ptr(), None), "aligned")):
        assert lib.ccx_q_actions(*args) == _abi.EINVAL
        assert word in lib.ccx_last_error().decode()
    batch.synchronize()
    again = ql.td_loss(*good).stats
    batch.synchronize()
    assert torch.equal(again.view(torch.int32), stats.view(torch.int32))
    a = ql.q_actions(q, mk, greedy=True).actions.cpu()
    assert ((a == 0) | (a == 255)).all()                                 # all Q-values equal: the lowest legal action


# ------------------------------------------------------------------------------------------------- 7. end to end
def test_the_examples_loop_twice():
    import torch

    spec = importlib.util.spec_from_file_location("dqn_two_policies", ROOT / "examples" / "dqn_two_policies.py")
    example = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(example)
    kw = dict(num_envs=64, updates=20, ring_steps=16, batch=256, warmup_steps=8, target_every=5, anneal_updates=10, hidden=16,
              log_every=0)
    first, counts, stats = example.train(**kw)
    second, counts2, _ = example.train(**kw)
    assert counts == counts2 == (20, 0)
    assert all(torch.isfinite(p).all() for p in first) and all(np.isfinite(s).all() and s[6] > 0 for s in map(np.array, stats))
    assert example.same_bits(first, second), "two runs from the same seeds must end with the same parameter bits"
