"""The two-layer perceptron on the device (include/ccx.h: CCX_MLP) against the NumPy spec (tests/_mlp_spec.py): y and hidden
bit for bit on row counts that cross every boundary of the kernel's layout, row independence, the fused obs -> actions
launch against the two-launch composition, the ratio of exactly 1 on a [K, E, N, L] batch, graph capture, autograd and the
refusals.  f32 values are compared as bit patterns throughout (tests/_mlp_spec.bits32c: a NaN's sign and payload are the
one thing the rule leaves open)."""

import itertools

import numpy as np
import pytest
from _mlp_spec import RELU, SHAPES, TANH, bits32, bits32c, make_mlp_case, mlp_spec
from _reset_obs_spec import make_config

pytestmark = pytest.mark.gpu

# one row; 63 / 64 / 65 rows around one tile; 129: two tiles and one row; 1000: sixteen tiles, a tail of 40
ROWS = (1, 63, 64, 65, 129, 1000)
ALL_SHAPES = SHAPES + ((1, 16, 1, TANH),)                                   # L = 1: rows * L < 4 floats for one row
ACT = {TANH: "tanh", RELU: "relu"}
SEED = 0x0123_4567_89AB_CDEF
MODES = tuple(itertools.product((True, False), (False, True)))              # (masked, deterministic)


@pytest.fixture(scope="module")
def batches():
    import torch

    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    from collectivecrossing_amd.batched import BatchedCollectiveCrossing

    made = {}

    def get(N, E):
        if (N, E) not in made:
            b = BatchedCollectiveCrossing(make_config(N, max_steps=12), E)
            b.make_reset_pool(seed0=5, size=256)
            made[N, E] = b
        return made[N, E]

    yield get
    for b in made.values():
        b.close()


@pytest.fixture(scope="module")
def spec_cases():
    """1000 generator rows per shape and the spec's y and hidden for them, made once (a row's outputs do not depend on its
    neighbours -- tests/test_mlp_spec.py -- so the first M rows are the case of M rows)."""
    cache = {}

    def get(L, H, O, act):
        if (L, H, O, act) not in cache:
            c = make_mlp_case(max(ROWS), L, H, O, seed=L * 7 + H)
            cache[L, H, O, act] = (c, mlp_spec(c["x"], c["w1t"], c["b1"], c["w2"], c["b2"], act))
        return cache[L, H, O, act]

    return get


def _head(batch, c, L, H, O, act):
    import torch

    head = batch.mlp_head(H, O, ACT[act], L=L)
    with torch.no_grad():
        for name in ("w1t", "b1", "w2", "b2"):
            getattr(head, name).copy_(torch.from_numpy(c[name]))
    return head


def _policy(batch, scale=4.0, H=64, seed=3):
    """An actor whose logits spread enough for every action to be drawn."""
    import torch

    torch.manual_seed(seed)
    head = batch.mlp_head(H)
    with torch.no_grad():
        head.w2.mul_(scale)
        head.w1t.mul_(0.25)
    return head


# ------------------------------------------------------------------------------------------------- 1. bits against the spec
@pytest.mark.parametrize("L,H,O,act", ALL_SHAPES)
def test_y_and_hidden_equal_the_spec(batches, spec_cases, L, H, O, act):
    import torch

    batch = batches(8, 96)
    c, (want_y, want_h) = spec_cases(L, H, O, act)
    head = _head(batch, c, L, H, O, act)
    x_all = torch.from_numpy(c["x"]).cuda()
    for rows in ROWS:
        x = x_all[:rows].clone()
        y = torch.empty((rows, O), dtype=torch.float32, device="cuda")
        hid = torch.empty((rows, H), dtype=torch.float32, device="cuda")
        y.view(torch.uint8).fill_(0xEE)
        hid.view(torch.uint8).fill_(0xEE)
        torch.cuda.synchronize()
        batch._mlp_forward(head, x, y, hid)
        with torch.no_grad():
            plain = head(x)
        batch.synchronize()
        np.testing.assert_array_equal(bits32c(y.cpu().numpy()), bits32c(want_y[:rows]), err_msg=f"y, {rows} rows")
        np.testing.assert_array_equal(bits32c(hid.cpu().numpy()), bits32c(want_h[:rows]), err_msg=f"hidden, {rows} rows")
        np.testing.assert_array_equal(bits32(plain.cpu().numpy()), bits32(y.cpu().numpy()), err_msg=f"head(x), {rows} rows")
    assert np.isnan(want_y).any() and np.isfinite(want_y).any()


# ------------------------------------------------------------------------------------------------- 2. row independence
@pytest.mark.parametrize("L,H,O,act", SHAPES[:3])
def test_rows_do_not_depend_on_their_place(batches, spec_cases, L, H, O, act):
    import torch

    batch = batches(8, 96)
    c, _ = spec_cases(L, H, O, act)
    head = _head(batch, c, L, H, O, act)
    x_all = torch.from_numpy(c["x"]).cuda()
    rows = x_all[300:400].clone()
    big = x_all.flip(0).contiguous()
    big[437:537] = rows
    with torch.no_grad():
        alone, shaped, inside = head(rows), head(rows.view(5, 20, L).contiguous()), head(big)
    batch.synchronize()
    assert tuple(shaped.shape) == (5, 20, O)
    np.testing.assert_array_equal(bits32(shaped.view(100, O).cpu().numpy()), bits32(alone.cpu().numpy()))
    np.testing.assert_array_equal(bits32(inside[437:537].cpu().numpy()), bits32(alone.cpu().numpy()))


# ------------------------------------------------------------------------------------------------- 3. the fused launch
@pytest.mark.parametrize("E,N,steps", ((96, 8, 10), (5, 3, 9)))
def test_fused_sampling_equals_the_two_launches(batches, E, N, steps):
    import torch

    batch = batches(N, E)
    batch.reset_from_pool()
    batch.set_rng_seed(SEED)
    batch.rollout_greedy(steps, want_obs=False)
    obs, masks = batch.observe(), batch.action_masks()
    state = batch.get_state()
    dead = (state["terminated"] | state["truncated"]) != 0
    assert E * N < 64 or (dead.any() and not dead.all())
    head = _policy(batch)
    seen = set()
    for masked, det in MODES:
        m = masks if masked else None
        lo = torch.empty((E, N, 5), dtype=torch.float32, device="cuda")
        lo.view(torch.uint8).fill_(0xEE)
        fused = batch.mlp_sample_actions(head, obs, m, deterministic=det, want_logp=True, want_entropy=True, logits_out=lo)
        with torch.no_grad():
            logits = head(obs)
        two = batch.sample_actions(logits, m, deterministic=det, want_logp=True, want_entropy=True)
        bare = batch.mlp_sample_actions(head, obs, m, deterministic=det, want_logp=False)          # the instantiations without statistics
        only_logp = batch.mlp_sample_actions(head, obs, m, deterministic=det)
        batch.synchronize()
        tag = f"masked {masked} det {det}"
        np.testing.assert_array_equal(bits32(lo.cpu().numpy()), bits32(logits.cpu().numpy()), err_msg=f"logits_out {tag}")
        for name in ("actions", "logp", "entropy"):
            np.testing.assert_array_equal(bits32(getattr(fused, name).cpu().numpy()), bits32(getattr(two, name).cpu().numpy()),
                                          err_msg=f"{name} {tag}")
        assert bare.logp is None and bare.entropy is None and only_logp.entropy is None
        np.testing.assert_array_equal(bare.actions.cpu().numpy(), two.actions.cpu().numpy(), err_msg=f"no statistics {tag}")
        np.testing.assert_array_equal(bits32(only_logp.logp.cpu().numpy()), bits32(two.logp.cpu().numpy()))
        acts = two.actions.cpu().numpy()
        assert (acts[dead] == 255).all() and (acts[~dead] < 5).all()
        seen |= set(np.unique(acts).tolist())
    assert E * N < 64 or seen == {0, 1, 2, 3, 4, 255}


# ------------------------------------------------------------------------------------------------- 4. the ratio is exactly 1
def test_the_ratio_is_exactly_one_on_the_whole_batch(batches):
    import torch

    E, N, K = 64, 8, 8
    batch = batches(N, E)
    batch.reset_from_pool()
    batch.set_rng_seed(SEED)
    batch.rollout_greedy(6, want_obs=False)                                # some agents have arrived: 255 rows from the first step on
    head = _policy(batch, seed=4)
    L = batch.obs_len
    obs, masks = batch.observe(), batch.action_masks()
    rows = torch.empty((K, E, N, L), dtype=torch.float32, device="cuda")
    mk = torch.empty((K, E, N), dtype=torch.uint8, device="cuda")
    acts = torch.empty((K, E, N), dtype=torch.uint8, device="cuda")
    logp = torch.empty((K, E, N), dtype=torch.float32, device="cuda")
    ent = torch.empty((K, E, N), dtype=torch.float32, device="cuda")
    out = batch.alloc_rollout(1)
    for s in range(K):
        rows[s].copy_(obs)
        mk[s].copy_(masks)
        res = batch.mlp_sample_actions(head, obs, masks, want_entropy=True)
        acts[s].copy_(res.actions)
        logp[s].copy_(res.logp)
        ent[s].copy_(res.entropy)
        batch.rollout(res.actions[None], auto_reset=True, out=out, masks_out=masks, reset_obs="next")
        obs.copy_(out.obs[0])
    with torch.no_grad():
        logits = head(rows)                                                # ONE call on [K, E, N, L]
    ev = batch.evaluate_actions(logits, acts, mk)
    batch.synchronize()
    a = acts.cpu().numpy()
    live = a != 255
    assert live.sum() > K * E * N // 2 and (~live).any() and len(np.unique(a)) == 6
    np.testing.assert_array_equal(bits32(ev.logp.cpu().numpy())[live], bits32(logp.cpu().numpy())[live])
    np.testing.assert_array_equal(bits32(ev.entropy.cpu().numpy())[live], bits32(ent.cpu().numpy())[live])
    assert not bits32(ev.logp.cpu().numpy())[~live].any() and not bits32(logp.cpu().numpy())[~live].any()


# ------------------------------------------------------------------------------------------------- 5. graph capture
def test_captured_actor_loop_repeats_the_eager_run():
    import torch

    from collectivecrossing_amd.batched import BatchedCollectiveCrossing, SampleResult

    E, N, K = 64, 8, 8
    env = BatchedCollectiveCrossing(make_config(N, max_steps=12), E)
    env.make_reset_pool(seed0=5, size=256)
    env.reset_from_pool()
    env.set_rng_seed(SEED)
    env.rollout_greedy(6, want_obs=False)                                  # some agents have arrived
    start = env.get_state()
    head = _policy(env, seed=5)
    side = torch.cuda.Stream()
    env.use_stream(side)
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        obs, masks = env.observe(), env.action_masks()
        actions = torch.empty((1, E, N), dtype=torch.uint8, device="cuda")
        logp = torch.empty((E, N), dtype=torch.float32, device="cuda")
        sampled = SampleResult(actions[0], logp, None)
        out = env.alloc_rollout(1)
        hist = {k: torch.empty((K,) + tuple(t.shape), dtype=t.dtype, device="cuda") for k, t in (("actions", actions[0]), ("logp", logp))}

        def body():
            env.mlp_sample_actions(head, obs, masks, out=sampled)
            env.rollout(actions, auto_reset=True, out=out, masks_out=masks, reset_obs="next")
            obs.copy_(out.obs[0])

        def run(step):
            for s in range(K):
                step()
                hist["actions"][s].copy_(actions[0])
                hist["logp"][s].copy_(logp)
            side.synchronize()
            return {k: t.cpu().numpy() for k, t in hist.items()}

        eager = run(body)
        assert len(np.unique(eager["actions"])) == 6
        env.set_state(**start)
        env.observe(out=obs)
        env.action_masks(out=masks)
        side.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            body()
        side.synchronize()
        replayed = run(graph.replay)
        for k in hist:
            np.testing.assert_array_equal(bits32(replayed[k]), bits32(eager[k]), err_msg=f"graph replay: {k}")
    env.use_stream(None)
    env.close()


# ------------------------------------------------------------------------------------------------- 6. autograd
@pytest.mark.parametrize("act", ("tanh", "relu"))
def test_gradients_against_f64_autograd(batches, act):
    """The yardstick is the f32 torch module's own error against f64 autograd: the backward here is the same f32 arithmetic
    in another summation order, so it may err at most 4 x as much (per parameter, maximum norm)."""
    import torch

    batch = batches(8, 96)
    torch.manual_seed(11)
    head = batch.mlp_head(64, 5, act)
    L = head.L
    x = torch.randn((1000, L), device="cuda")
    coef = torch.randn((1000, 5), device="cuda")
    with torch.no_grad():
        plain = head(x)
    y = head(x)
    assert y.requires_grad
    np.testing.assert_array_equal(bits32(y.detach().cpu().numpy()), bits32(plain.cpu().numpy()))   # the same bits under grad
    (y * coef).sum().backward()
    ours = [p.grad.double() for p in (head.w1t, head.b1, head.w2, head.b2)]
    grads = {}
    for dtype in (torch.float64, torch.float32):
        seq = head.to_sequential(dtype)
        (seq(x.to(dtype)) * coef.to(dtype)).sum().backward()
        grads[dtype] = [seq[0].weight.grad.t().double(), seq[0].bias.grad.double(), seq[2].weight.grad.double(), seq[2].bias.grad.double()]
    for name, g, g32, g64 in zip(("w1t", "b1", "w2", "b2"), ours, grads[torch.float32], grads[torch.float64]):
        err, yard = float((g - g64).abs().max()), float((g32 - g64).abs().max())
        print(f"{act} grad {name}: max |ours - f64| = {err:.3e}, max |f32 Sequential - f64| = {yard:.3e}, max |f64| = {float(g64.abs().max()):.3e}")
        assert g.shape == g64.shape and err <= 4.0 * yard, name
    with pytest.raises(ValueError):
        head(x, out=torch.empty((1000, 5), device="cuda"))
    xg = x.clone().requires_grad_(True)
    head(xg).sum().backward()
    seq = head.to_sequential(torch.float64)
    x64 = x.double().requires_grad_(True)
    seq(x64).sum().backward()
    assert float((xg.grad.double() - x64.grad).abs().max()) <= 1e-5 * float(x64.grad.abs().max())


def test_conversions_are_exact(batches):
    import torch

    from collectivecrossing_amd import MlpHead

    batch = batches(8, 96)
    torch.manual_seed(2)
    seq = torch.nn.Sequential(torch.nn.Linear(38, 32), torch.nn.ReLU(), torch.nn.Linear(32, 1)).cuda()
    head = MlpHead.from_linear(batch, seq[0], seq[2], "relu")
    assert (head.L, head.H, head.O, head.activation) == (38, 32, 1, "relu")
    back = head.to_sequential()
    for a, b in zip(seq.parameters(), back.parameters()):
        assert torch.equal(a, b)
    torch.manual_seed(7)
    fresh = batch.mlp_head(64)
    torch.manual_seed(7)
    ref = torch.nn.Sequential(torch.nn.Linear(38, 64), torch.nn.Tanh(), torch.nn.Linear(64, 5))
    assert torch.equal(fresh.w1t.cpu(), ref[0].weight.t()) and torch.equal(fresh.b2.cpu(), ref[2].bias)   # initialised as Linear
    x = torch.randn((300, 38), device="cuda")
    with torch.no_grad():
        assert float((fresh(x) - ref.cuda()(x)).abs().max()) < 1e-5


# ------------------------------------------------------------------------------------------------- 7. refusals
def test_refusals_leave_the_batch_usable(batches):
    import torch

    from collectivecrossing_amd import _abi

    batch = batches(8, 96)
    E, N, L = 96, 8, batch.obs_len
    head = batch.mlp_head(64)
    x = torch.randn((E, N, L), device="cuda")
    shifted = torch.empty(E * N * L + 1, dtype=torch.float32, device="cuda")[1:].view(E, N, L)
    assert shifted.is_contiguous() and shifted.data_ptr() % 16
    for bad in (x.double(), x.half(), x[..., :-1], x[..., :-1].contiguous(), x.transpose(0, 1), x.cpu(), shifted, x.cpu().numpy()):
        with pytest.raises(ValueError):
            with torch.no_grad():
                head(bad)
    with pytest.raises(ValueError):
        with torch.no_grad():
            head(x, out=torch.empty((E, N, 4), device="cuda"))
    for kw in (dict(H=24), dict(H=8), dict(H=272), dict(H=64, O=9), dict(H=64, O=0), dict(H=64, L=513), dict(H=64, activation="gelu")):
        with pytest.raises(ValueError):
            batch.mlp_head(**kw)
    critic = batch.mlp_head(64, 1)
    other_l = batch.mlp_head(64, 5, L=L + 1)
    for kw in (dict(head=critic, obs=x), dict(head=other_l, obs=x), dict(head=head, obs=x.double()), dict(head=head, obs=x[:-1]),
               dict(head=head, obs=shifted), dict(head=head, obs=x, masks=torch.zeros((E, N), dtype=torch.int32, device="cuda")),
               dict(head=head, obs=x, logits_out=torch.empty((E, N, 4), device="cuda")), dict(head=head, obs=x, out=(1, 2)),
               dict(head="head", obs=x)):
        with pytest.raises(ValueError):
            batch.mlp_sample_actions(**kw)
    with torch.no_grad():
        empty = head(torch.empty((0, L), device="cuda"))
        empty2 = head(torch.empty((3, 0, L), device="cuda"))
    assert tuple(empty.shape) == (0, 5) and tuple(empty2.shape) == (3, 0, 5)
    assert tuple(head(torch.empty((0, L), device="cuda")).shape) == (0, 5)                       # under grad too
    # the library's own refusals (the wrapper refuses first, so they are reached through the bindings)
    lib, h = batch._lib, batch._h
    y = torch.empty((E * N, 5), device="cuda")
    p = [t.data_ptr() for t in (x, head.w1t, head.b1, head.w2, head.b2, y)]
    for args, word in (((None, 768, L, 64, 5, 0, *p, None), "NULL handle"), ((h, 768, L, 64, 5, 0, None, *p[1:], None), "NULL"),
                       ((h, 768, L, 64, 5, 0, *p[:5], None, None), "NULL"), ((h, 0, L, 64, 5, 0, *p, None), "rows"),
                       ((h, 768, L, 24, 5, 0, *p, None), "multiple of 16"), ((h, 768, L, 64, 9, 0, *p, None), "O = 9"),
                       ((h, 768, 0, 64, 5, 0, *p, None), "L = 0"), ((h, 768, L, 64, 5, 2, *p, None), "activation"),
                       ((h, 768, L, 64, 5, 0, shifted.data_ptr(), *p[1:], None), "aligned"),
                       ((h, 768, L, 64, 5, 0, *p, y.data_ptr() + 4), "aligned")):
        assert lib.ccx_mlp_forward(*args) == _abi.EINVAL, args
        assert word in lib.ccx_last_error().decode(), (word, lib.ccx_last_error())
    a = torch.empty((E, N), dtype=torch.uint8, device="cuda")
    for args, word in (((h, 24, 0, *p[:5], None, 0, a.data_ptr(), None, None, None), "multiple of 16"),
                       ((h, 64, 0, None, *p[1:5], None, 0, a.data_ptr(), None, None, None), "NULL"),
                       ((h, 64, 0, *p[:5], None, 0, None, None, None, None), "NULL"),
                       ((h, 64, 0, shifted.data_ptr(), *p[1:5], None, 0, a.data_ptr(), None, None, None), "aligned")):
        assert lib.ccx_mlp_sample_actions(*args) == _abi.EINVAL, args
        assert word in lib.ccx_last_error().decode(), (word, lib.ccx_last_error())
    with torch.no_grad():
        again = head(x)
        want = head.to_sequential()(x)
    batch.synchronize()
    assert float((again - want).abs().max()) < 1e-5
