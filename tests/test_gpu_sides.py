"""Per-side policy heads on the device (include/ccx.h: CCX_SIDES), forward and fused sampling: every group's rows of y and
hidden bit for bit against BOTH the existing kernel on the gathered, contiguous rows (``MlpHead``) and the NumPy spec
(tests/_mlp_spec.py) on those rows; unowned rows untouched; the fused draw against ``sample_actions(sides(obs))`` and, for
one ``"all"`` group, against ``mlp_sample_actions``; graph capture; the refusals.  f32 values are compared as bit patterns
(tests/_mlp_spec.bits32c: a NaN's sign and payload are the one thing the rule leaves open)."""

import itertools

import numpy as np
import pytest
from _mlp_spec import RELU, TANH, bits32, bits32c, make_mlp_case, mlp_spec
from _reset_obs_spec import make_config
from _split_step_cases import make_config as make_grid_config

pytestmark = pytest.mark.gpu

ACT = {TANH: "tanh", RELU: "relu"}
SEED = 0x0123_4567_89AB_CDEF
FILL = 0xA5
# N = 3 (2 + 1): the 64- and 256-row boundaries of both 2 M and M selected rows
MS_N3 = (1, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257)
# N = 8 (5 + 3): where 5 M and 3 M cross 64 and 256, and sixteen tiles and more
MS_N8 = (1, 12, 13, 21, 22, 51, 52, 85, 86, 1000)


@pytest.fixture(scope="module")
def batches():
    import torch

    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    from collectivecrossing_amd.batched import BatchedCollectiveCrossing

    made = {}

    def get(N, E):
        if (N, E) not in made:
            # (64 agents exceed the config validator's cap for any grid: built without validation, as the recorded fixture is)
            cfg = make_config(N, max_steps=40) if N <= 8 else make_grid_config(32, 16, N, nb=N // 2, max_steps=40)
            b = BatchedCollectiveCrossing(cfg, E)
            b.make_reset_pool(seed0=5, size=256)
            made[N, E] = b
        return made[N, E]

    yield get
    for b in made.values():
        b.close()


def slots_of(mask):
    return [a for a in range(64) if mask >> a & 1]


def make_sides(batch, keys, L, H, O, act, seed=0):
    """SideHeads over `keys` whose heads hold make_mlp_case's adversarial parameters, a different draw per group; returns it
    with the parameters as NumPy arrays per group (in the order of sides.groups)."""
    import torch

    from collectivecrossing_amd import SideHeads

    heads, params = {}, {}
    for i, key in enumerate(keys):
        c = make_mlp_case(1, L, H, O, seed=seed + 31 * i)
        head = batch.mlp_head(H, O, ACT[act], L=L)
        with torch.no_grad():
            for name in ("w1t", "b1", "w2", "b2"):
                getattr(head, name).copy_(torch.from_numpy(c[name]))
        heads[key] = head
        params[id(head)] = c
    sides = SideHeads(batch, heads)
    return sides, [params[id(h)] for _, h in sides.groups]


def rows_case(M, N, L, seed):
    """x f32 [M, N, L]: make_mlp_case's rows (integers, normals, huge, tiny, NaN / inf rows)."""
    return make_mlp_case(M * N, L, 16, 1, seed=seed)["x"].reshape(M, N, L)


def prefilled(shape):
    import torch

    t = torch.empty(shape, dtype=torch.float32, device="cuda")
    t.view(torch.uint8).fill_(FILL)
    return t


def check_forward(batch, sides, params, x_all, Ms, act):
    """sides(x[:M]) for every M: y and hidden of every group's rows against the kernel on gathered rows and the spec (computed
    once on the largest M: a row's outputs do not depend on its neighbours); every other element keeps the prefill."""
    import torch

    Mmax, N, L = x_all.shape
    H, O = sides.H, sides.O
    want = []
    for (mask, _), c in zip(sides.groups, params):
        g = np.ascontiguousarray(x_all[:, slots_of(mask), :]).reshape(-1, L)
        want.append(mlp_spec(g, c["w1t"], c["b1"], c["w2"], c["b2"], act))
    xd_all = torch.from_numpy(x_all).cuda()
    fill = np.frombuffer(bytes([FILL] * 4), np.uint32)[0]
    for M in Ms:
        x = xd_all[:M].clone()
        y, hid = prefilled((M, N, O)), prefilled((M, N, H))
        torch.cuda.synchronize()
        with torch.no_grad():
            got = sides(x, out=y, hidden_out=hid)
        assert got is y
        batch.synchronize()
        yb, hb = bits32c(y.cpu().numpy()), bits32c(hid.cpu().numpy())
        owned = np.zeros(N, bool)
        for (mask, head), (wy, wh) in zip(sides.groups, want):
            sl = slots_of(mask)
            owned[sl] = True
            S = len(sl)
            np.testing.assert_array_equal(yb[:, sl].reshape(M * S, O), bits32c(wy[:M * S]), err_msg=f"y against the spec, M = {M}, slots {sl}")
            np.testing.assert_array_equal(hb[:, sl].reshape(M * S, H), bits32c(wh[:M * S]), err_msg=f"hidden against the spec, M = {M}, slots {sl}")
            gx = x[:, sl, :].contiguous()
            gh = torch.empty((M, S, H), dtype=torch.float32, device="cuda")
            with torch.no_grad():
                gy = head(gx, hidden_out=gh)
            batch.synchronize()
            np.testing.assert_array_equal(bits32(y[:, sl].cpu().numpy()), bits32(gy.cpu().numpy()), err_msg=f"y against MlpHead, M = {M}, slots {sl}")
            np.testing.assert_array_equal(bits32(hid[:, sl].cpu().numpy()), bits32(gh.cpu().numpy()), err_msg=f"hidden against MlpHead, M = {M}, slots {sl}")
        assert (yb[:, ~owned] == fill).all() and (hb[:, ~owned] == fill).all(), f"unowned rows were written, M = {M}"
    return want


# ------------------------------------------------------------------------------------------------- 1. forward and hidden
@pytest.mark.parametrize("N,H,Ms", ((3, 16, MS_N3), (8, 64, MS_N8)))
def test_two_sides_equal_mlp_head_and_the_spec(batches, N, H, Ms):
    batch = batches(N, 64)
    L = batch.obs_len
    assert L == {3: 18, 8: 38}[N]
    sides, params = make_sides(batch, ("boarding", "exiting"), L, H, 5, TANH, seed=N)
    assert [m for m, _ in sides.groups] == {3: [0b011, 0b100], 8: [0b00011111, 0b11100000]}[N]
    want = check_forward(batch, sides, params, rows_case(max(Ms), N, L, seed=10 + N), Ms, TANH)
    # (the case exercises NaN / inf rows -- which slots hold them depends on N -- and ordinary ones in every group)
    assert any(np.isnan(wy).any() for wy, _ in want) and all(np.isfinite(wy).any() for wy, _ in want)


def test_three_groups_leave_the_unowned_rows_alone(batches):
    batch = batches(8, 64)
    sides, params = make_sides(batch, ((0, 2, 5), (1,), (6, 7)), 38, 64, 5, TANH, seed=5)
    assert [m for m, _ in sides.groups] == [0b00100101, 0b00000010, 0b11000000] and not sides.all_owned
    check_forward(batch, sides, params, rows_case(130, 8, 38, seed=6), (1, 21, 22, 64, 130), TANH)


def test_an_odd_row_length_takes_the_dword_loads(batches):
    batch = batches(4, 8)
    sides, params = make_sides(batch, ("boarding", "exiting"), 7, 16, 1, RELU, seed=7)
    check_forward(batch, sides, params, rows_case(65, 4, 7, seed=8), (1, 65), RELU)


def test_the_limits(batches):
    """N = 64, L = 262, H = 256 (sixteen waves), O = 8, the odd slots as one group: the LDS opt-in above 64 KB."""
    batch = batches(64, 4)
    assert batch.obs_len == 262
    sides, params = make_sides(batch, (tuple(range(1, 64, 2)),), 262, 256, 8, TANH, seed=9)
    check_forward(batch, sides, params, rows_case(5, 64, 262, seed=10), (5,), TANH)


def test_eight_single_slot_groups_with_eight_heads(batches):
    batch = batches(8, 64)
    sides, params = make_sides(batch, tuple((a,) for a in (3, 0, 7, 1, 6, 2, 5, 4)), 38, 32, 5, RELU, seed=11)
    assert [m for m, _ in sides.groups] == [1 << a for a in range(8)]        # ascending order of the lowest slot
    assert len(list(sides.parameters())) == 32
    check_forward(batch, sides, params, rows_case(70, 8, 38, seed=12), (1, 63, 64, 65, 70), RELU)


def test_one_group_all_is_mlp_head(batches):
    import torch

    batch = batches(8, 64)
    sides, _ = make_sides(batch, ("all",), 38, 64, 5, TANH, seed=13)
    head = sides.groups[0][1]
    for M in (1, 8, 9, 100):
        x = torch.from_numpy(rows_case(M, 8, 38, seed=14)).cuda()
        with torch.no_grad():
            hs, hh = torch.empty((M, 8, 64), device="cuda"), torch.empty((M, 8, 64), device="cuda")
            ys, yh = sides(x, hidden_out=hs), head(x, hidden_out=hh)
        batch.synchronize()
        np.testing.assert_array_equal(bits32(ys.cpu().numpy()), bits32(yh.cpu().numpy()))
        np.testing.assert_array_equal(bits32(hs.cpu().numpy()), bits32(hh.cpu().numpy()))


def test_outputs_the_call_allocates_hold_zeros_at_unowned_rows(batches):
    import torch

    batch = batches(8, 64)
    sides, _ = make_sides(batch, ("boarding",), 38, 64, 5, TANH, seed=15)
    x = torch.from_numpy(rows_case(9, 8, 38, seed=16)).cuda()
    with torch.no_grad():
        y = sides(x)
    batch.synchronize()
    assert not bits32(y[:, 5:].cpu().numpy()).any()


# ------------------------------------------------------------------------------------------------- 2. the fused draw
def _policy_sides(batch, keys, seed=3, scale=4.0, H=64):
    """Actors whose logits spread enough for every action to be drawn; a different draw per group."""
    import torch

    from collectivecrossing_amd import SideHeads

    torch.manual_seed(seed)
    heads = {}
    for key in keys:
        head = batch.mlp_head(H)
        with torch.no_grad():
            head.w2.mul_(scale)
            head.w1t.mul_(0.25)
        heads[key] = head
    return SideHeads(batch, heads)


def _ten_steps_in(batch):
    batch.reset_from_pool()
    batch.set_rng_seed(SEED)
    batch.rollout_policy(10, "random", want_obs=False)                     # ten random steps, then towards the goals: some agents are done
    batch.rollout_greedy(8, want_obs=False)
    state = batch.get_state()
    dead = (state["terminated"] | state["truncated"]) != 0
    assert dead.any() and not dead.all()
    return batch.observe(), batch.action_masks(), dead


@pytest.mark.parametrize("E,N", ((64, 3), (100, 3), (64, 8), (100, 8)))
def test_fused_sampling_equals_sample_actions_of_the_forward(batches, E, N):
    import torch

    batch = batches(N, E)
    obs, masks, dead = _ten_steps_in(batch)
    full = _policy_sides(batch, ("boarding", "exiting"))
    part = _policy_sides(batch, ("exiting",), seed=4)
    fill = np.frombuffer(bytes([FILL] * 4), np.uint32)[0]
    seen = set()
    for sides in (full, part):
        owned = np.array([bool(sides.owned >> a & 1) for a in range(N)])
        for masked, det, want_entropy in itertools.product((True, False), (False, True), (True, False)):
            m = masks if masked else None
            tag = f"owned {sides.owned:#x} masked {masked} det {det} entropy {want_entropy}"
            lo = prefilled((E, N, 5))
            torch.cuda.synchronize()
            fused = sides.sample_actions(obs, m, deterministic=det, want_logp=True, want_entropy=want_entropy, logits_out=lo)
            with torch.no_grad():
                logits = sides(obs)
            two = batch.sample_actions(logits, m, deterministic=det, want_logp=True, want_entropy=want_entropy)
            bare = sides.sample_actions(obs, m, deterministic=det, want_logp=False)               # the instantiations without statistics
            batch.synchronize()
            assert (fused.entropy is None) == (not want_entropy) and bare.logp is None and bare.entropy is None
            lob = bits32(lo.cpu().numpy())
            np.testing.assert_array_equal(lob[:, owned], bits32(logits.cpu().numpy())[:, owned], err_msg=f"logits_out {tag}")
            assert (lob[:, ~owned] == fill).all(), f"logits_out of unowned slots {tag}"
            for name in ("actions", "logp") + (("entropy",) if want_entropy else ()):
                got, want = getattr(fused, name).cpu().numpy(), getattr(two, name).cpu().numpy()
                np.testing.assert_array_equal(bits32(got)[:, owned], bits32(want)[:, owned], err_msg=f"{name} {tag}")
                if name == "actions":
                    assert (got[:, ~owned] == 255).all(), tag
                else:
                    assert not bits32(got)[:, ~owned].any(), f"{name} of unowned slots is not +0.0, {tag}"
            np.testing.assert_array_equal(bare.actions.cpu().numpy(), fused.actions.cpu().numpy(), err_msg=f"no statistics {tag}")
            acts = fused.actions.cpu().numpy()
            assert (acts[dead] == 255).all() and (acts[~dead & owned[None, :]] < 5).all()
            seen |= set(np.unique(acts).tolist())
    assert seen == {0, 1, 2, 3, 4, 255}


@pytest.mark.parametrize("E,N", ((100, 3), (64, 8)))
def test_one_group_all_equals_mlp_sample_actions(batches, E, N):
    import torch

    batch = batches(N, E)
    obs, masks, _ = _ten_steps_in(batch)
    sides = _policy_sides(batch, ("all",), seed=6)
    head = sides.groups[0][1]
    for masked, det in itertools.product((True, False), (False, True)):
        m = masks if masked else None
        la, lb = torch.empty((E, N, 5), device="cuda"), torch.empty((E, N, 5), device="cuda")
        a = sides.sample_actions(obs, m, deterministic=det, want_entropy=True, logits_out=la)
        b = batch.mlp_sample_actions(head, obs, m, deterministic=det, want_entropy=True, logits_out=lb)
        batch.synchronize()
        for name in ("actions", "logp", "entropy"):
            np.testing.assert_array_equal(bits32(getattr(a, name).cpu().numpy()), bits32(getattr(b, name).cpu().numpy()), err_msg=name)
        np.testing.assert_array_equal(bits32(la.cpu().numpy()), bits32(lb.cpu().numpy()))


def test_captured_actor_loop_repeats_the_eager_run():
    import torch

    from collectivecrossing_amd.batched import BatchedCollectiveCrossing, SampleResult

    E, N, K = 64, 8, 3
    env = BatchedCollectiveCrossing(make_config(N, max_steps=12), E)
    env.make_reset_pool(seed0=5, size=256)
    env.reset_from_pool()
    env.set_rng_seed(SEED)
    env.rollout_greedy(6, want_obs=False)                                  # some agents have arrived
    start = env.get_state()
    sides = _policy_sides(env, ("boarding", "exiting"), seed=5)
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
            sides.sample_actions(obs, masks, out=sampled)
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
        env.set_state(**start)
        env.observe(out=obs)
        env.action_masks(out=masks)
        side.synchronize()
        replayed = run(graph.replay)
        for k in hist:
            np.testing.assert_array_equal(bits32(replayed[k]), bits32(eager[k]), err_msg=f"graph replay: {k}")
    env.use_stream(None)
    env.close()


# ------------------------------------------------------------------------------------------------- 3. refusals
def test_refusals_leave_the_batch_usable(batches):
    import torch

    from collectivecrossing_amd import SideHeads, _abi
    from collectivecrossing_amd._abi import CcxSlotGroup

    batch, other = batches(8, 64), batches(3, 64)
    E, N, L = 64, 8, batch.obs_len
    mk = lambda **kw: batch.mlp_head(**{"H": 64, **kw})  # noqa: E731
    for heads in ({}, [mk()], {"boarding": mk(), "exiting": mk(H=32)}, {"boarding": mk(), "exiting": mk(O=1)},
                  {"boarding": mk(), "exiting": mk(activation="relu")}, {"boarding": mk(), "exiting": mk(L=L + 2)},
                  {"boarding": mk(), "all": mk()}, {"boarding": mk(), (4, 5): mk()}, {"boarding": other.mlp_head(64)},
                  {"boarding": torch.nn.Linear(3, 3)}, {(): mk()}, {0: mk()}, {"nobody_7": mk()}, {1 << 8: mk()},
                  {(a,): mk(H=16) for a in range(8)} | {"exiting_0": mk(H=16)}):
        with pytest.raises(ValueError):
            SideHeads(batch, heads)
    sides = SideHeads(batch, {"boarding": mk(), "exiting": mk()})
    critics = SideHeads(batch, {"boarding": mk(O=1), "exiting": mk(O=1)})
    x = torch.randn((E, N, L), device="cuda")
    shifted = torch.empty(E * N * L + 1, dtype=torch.float32, device="cuda")[1:].view(E, N, L)
    for bad in (x.double(), x[..., :-1].contiguous(), x[:, :-1].contiguous(), x.view(E * N, L), x.transpose(0, 1), x.cpu(), shifted):
        with pytest.raises(ValueError):
            with torch.no_grad():
                sides(bad)
    with torch.no_grad():
        for kw in (dict(out=torch.empty((E, N, 4), device="cuda")), dict(hidden_out=torch.empty((E, N, 32), device="cuda")),
                   dict(hidden_out=torch.empty(E * N * 64 + 1, device="cuda")[1:].view(E, N, 64))):
            with pytest.raises(ValueError):
                sides(x, **kw)
    with pytest.raises(ValueError):
        sides(x, out=torch.empty((E, N, 5), device="cuda"))                    # under grad: the autograd path allocates
    with pytest.raises(ValueError):
        sides(x.clone().requires_grad_(True))
    for call in (lambda: critics.sample_actions(x), lambda: sides.sample_actions(x.double()), lambda: sides.sample_actions(x[:-1]),
                 lambda: sides.sample_actions(shifted), lambda: sides.sample_actions(x, torch.zeros((E, N), dtype=torch.int32, device="cuda")),
                 lambda: sides.sample_actions(x, logits_out=torch.empty((E, N, 4), device="cuda")), lambda: sides.sample_actions(x, out=(1, 2)),
                 lambda: sides.alloc_backward((4, E, N + 1)), lambda: sides.backward_into(x, x, x),
                 lambda: sides.backward_into(x, torch.empty((E, N, 64), device="cuda"), torch.empty((E, N, 5), device="cuda"), out=[1, 2])):
        with pytest.raises(ValueError):
            call()
    with torch.no_grad():
        empty = sides(torch.empty((0, N, L), device="cuda"))
    assert tuple(empty.shape) == (0, N, 5) and tuple(sides(torch.empty((2, 0, N, L), device="cuda")).shape) == (2, 0, N, 5)
    # the library's own refusals (the wrapper refuses first, so they are reached through the bindings)
    lib, h = batch._lib, batch._h
    y = torch.empty((E, N, 5), device="cuda")
    heads = [hd for _, hd in sides.groups]

    def table(*masks, null=False):
        t = (CcxSlotGroup * max(1, len(masks)))()
        for row, mask, hd in zip(t, masks, itertools.cycle(heads)):
            row.slots, row.w1t, row.b1, row.w2, row.b2 = mask, hd.w1t.data_ptr(), hd.b1.data_ptr(), hd.w2.data_ptr(), hd.b2.data_ptr()
        if null:
            t[0].w2 = None
        return len(masks), t

    ok = table(0x1F, 0xE0)
    for args, word in (((None, E, N, L, 64, 5, 0, x.data_ptr(), *ok, y.data_ptr(), None), "NULL handle"),
                       ((h, E, N, L, 64, 5, 0, None, *ok, y.data_ptr(), None), "NULL"),
                       ((h, E, N, L, 64, 5, 0, x.data_ptr(), 2, None, y.data_ptr(), None), "NULL groups"),
                       ((h, E, N, L, 64, 5, 0, x.data_ptr(), *table(0x1F, 0xE0, null=True), y.data_ptr(), None), "NULL parameter"),
                       ((h, 0, N, L, 64, 5, 0, x.data_ptr(), *ok, y.data_ptr(), None), "M = 0"),
                       ((h, E, 65, L, 64, 5, 0, x.data_ptr(), *ok, y.data_ptr(), None), "N = 65"),
                       ((h, E, N, L, 24, 5, 0, x.data_ptr(), *ok, y.data_ptr(), None), "multiple of 16"),
                       ((h, E, N, L, 64, 9, 0, x.data_ptr(), *ok, y.data_ptr(), None), "O = 9"),
                       ((h, E, N, L, 64, 5, 2, x.data_ptr(), *ok, y.data_ptr(), None), "activation"),
                       ((h, E, N, L, 64, 5, 0, x.data_ptr(), 0, ok[1], y.data_ptr(), None), "num_groups = 0"),
                       ((h, E, N, L, 64, 5, 0, x.data_ptr(), *table(*(1 << a for a in range(8)), 0), y.data_ptr(), None), "num_groups = 9"),
                       ((h, E, N, L, 64, 5, 0, x.data_ptr(), *table(0x1F, 0), y.data_ptr(), None), "empty"),
                       ((h, E, N, L, 64, 5, 0, x.data_ptr(), *table(0x1F, 0x1E0), y.data_ptr(), None), "at or above N"),
                       ((h, E, N, L, 64, 5, 0, x.data_ptr(), *table(0x1F, 0xF0), y.data_ptr(), None), "overlaps"),
                       ((h, E, N, L, 64, 5, 0, shifted.data_ptr(), *ok, y.data_ptr(), None), "aligned"),
                       ((h, E, N, L, 64, 5, 0, x.data_ptr(), *ok, y.data_ptr(), y.data_ptr() + 4), "aligned")):
        assert lib.ccx_sides_forward(*args) == _abi.EINVAL, args
        assert word in lib.ccx_last_error().decode(), (word, lib.ccx_last_error())
    a = torch.empty((E, N), dtype=torch.uint8, device="cuda")
    for args, word in (((h, 24, 0, x.data_ptr(), *ok, None, 0, a.data_ptr(), None, None, None), "multiple of 16"),
                       ((h, 64, 0, None, *ok, None, 0, a.data_ptr(), None, None, None), "NULL"),
                       ((h, 64, 0, x.data_ptr(), *ok, None, 0, None, None, None, None), "NULL"),
                       ((h, 64, 0, x.data_ptr(), *table(0x1F, 0x30, 0x20), None, 0, a.data_ptr(), None, None, None), "overlaps"),
                       ((h, 64, 0, shifted.data_ptr(), *ok, None, 0, a.data_ptr(), None, None, None), "aligned")):
        assert lib.ccx_sides_sample_actions(*args) == _abi.EINVAL, args
        assert word in lib.ccx_last_error().decode(), (word, lib.ccx_last_error())
    hid = torch.empty((E, N, 64), device="cuda")
    gy = torch.empty((E, N, 5), device="cuda")
    ws = torch.empty((1 << 20,), dtype=torch.uint8, device="cuda")
    g = [torch.empty(s, device="cuda") for s in ((L, 64), (64,), (5, 64), (5,))]
    base = (x.data_ptr(), hid.data_ptr(), gy.data_ptr(), heads[0].w2.data_ptr(), ws.data_ptr(), *(t.data_ptr() for t in g), None)
    for args, word in (((None, E, N, 0x1F, L, 64, 5, 0, *base), "NULL handle"), ((h, E, N, 0, L, 64, 5, 0, *base), "empty"),
                       ((h, E, N, 0x100, L, 64, 5, 0, *base), "at or above N"), ((h, 0, N, 0x1F, L, 64, 5, 0, *base), "M = 0"),
                       ((h, E, N, 0x1F, L, 64, 5, 0, None, *base[1:]), "NULL"), ((h, E, N, 0x1F, L, 40, 5, 0, *base), "multiple of 16"),
                       ((h, E, N, 0x1F, L, 64, 5, 0, *base[:4], ws.data_ptr() + 4, *base[5:]), "8-byte"),
                       ((h, E, N, 0x1F, L, 64, 5, 0, shifted.data_ptr(), *base[1:]), "16-byte")):
        assert lib.ccx_sides_backward(*args) == _abi.EINVAL, args
        assert word in lib.ccx_last_error().decode(), (word, lib.ccx_last_error())
    with torch.no_grad():
        again = sides(x)
        want = torch.cat([hd.to_sequential()(x[:, sl]) for hd, sl in zip(heads, (slice(0, 5), slice(5, 8)))], 1)
    batch.synchronize()
    assert float((again - want).abs().max()) < 1e-5
