"""The perceptron kernels over the whole legal (L, H, O) range (include/ccx.h: CCX_MLP, CCX_SIDES): the rule of each op
depends on neither the rows of a backward sub-tile, the waves of a forward workgroup, the LDS a launch asks for nor the
tile grid, and the shapes of tests/_mlp_shape_classes.py select every one of those branches
(tests/test_mlp_shape_classes.py asserts that on the CPU, from the library's own functions).  ``ccx_mlp_forward``,
``ccx_mlp_backward``, ``ccx_sides_forward`` and ``ccx_sides_backward`` bit for bit against a reference on row counts around
one sub-tile, two sub-tiles and one block, into buffers filled with 0xEE; the fused obs -> actions launches on the 50-agent
workload's 206-float rows.  The reference is the NumPy spec (tests/_mlp_spec.py, tests/_mlp_backward_spec.py) where its
Python loops take seconds, and the host-compiled rule of csrc/ccx_mlp_grad.h elsewhere, which
tests/test_mlp_backward_host_rule.py shows equal to the NumPy spec on every one of these shapes; every assertion message
names the one it used.  Finite inputs only: what a NaN row does is tests/test_gpu_mlp.py's and
tests/test_gpu_mlp_backward.py's business."""

import numpy as np
import pytest
from _mlp_backward_spec import NAMES, make_mlp_backward_case, mlp_backward_spec
from _mlp_host_rule import compiler, host_backward, load_backward
from _mlp_shape_classes import (BACKWARD, EVERY_G, FORWARD_ROWS, NUMPY_SPEC_FINAL_SUMS, SIDES_BACKWARD, SIDES_FORWARD, backward_rows,
                                by_dims)
from _mlp_spec import RELU, TANH, bits32, linear_init, make_mlp_case, mlp_spec
from _qlearn_spec import q_actions_spec
from _reset_obs_spec import make_config
from _sample_spec import sample_spec

pytestmark = pytest.mark.gpu

ACT = {TANH: "tanh", RELU: "relu"}
SEED = 0x0123_4567_89AB_CDEF
FILL = 0xEE
FILL32 = int(np.frombuffer(bytes([FILL] * 4), np.uint32)[0])
OUTS = NAMES + ("ga",)
NUMPY, HOST = "the NumPy spec", "the host-compiled rule (csrc/ccx_mlp_grad.h)"
IDS = dict(ids=lambda s: f"{s.L}-{s.H}-{s.O}")


@pytest.fixture(scope="module")
def batches():
    import torch

    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    from collectivecrossing_amd.batched import BatchedCollectiveCrossing

    made = {}

    def get(N):
        if N not in made:
            made[N] = BatchedCollectiveCrossing(make_config(N, max_steps=12), 4)
        return made[N]

    yield get
    for b in made.values():
        b.close()


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    cxx = compiler()
    assert cxx is not None, "the reference of the large shapes needs a host C++ compiler (c++, clang++ or ROCm's clang++)"
    return load_backward(cxx, tmp_path_factory.mktemp("mlp_shapes_host_rule"))


def backward_reference(host, L, H, O, act, x, hidden, grad_y, w2, rows, calls=1):
    """({M: dict(w1t, b1, w2, b2, ga) for the first M rows}, the reference's name).  The NumPy spec where the final sums its
    Python loop takes -- one per output element and row count, about 30 us each, in every one of the test's ``calls`` -- stay
    under NUMPY_SPEC_FINAL_SUMS (three seconds); the host-compiled rule elsewhere."""
    if ((L + 1) * H + O * (H + 1)) * len(rows) * calls < NUMPY_SPEC_FINAL_SUMS:
        return mlp_backward_spec(x, hidden, grad_y, w2, act, rows=rows), NUMPY
    return {m: host_backward(host, x[:m], hidden[:m], grad_y[:m], w2, act) for m in rows}, HOST


def prefilled(shape, dtype=None):
    import torch

    t = torch.empty(shape, dtype=dtype or torch.float32, device="cuda")
    t.view(torch.uint8).fill_(FILL)
    return t


def cuda(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def head_with(batch, c, L, H, O, act):
    import torch

    head = batch.mlp_head(H, O, ACT[act], L=L)
    with torch.no_grad():
        for name in NAMES:
            getattr(head, name).copy_(torch.from_numpy(c[name]))
    return head


def slots_of(mask):
    return [a for a in range(64) if mask >> a & 1]


# ------------------------------------------------------------------------------------------------- 1. forward
@pytest.mark.parametrize("L,H,O,act", tuple(s.dims for s in BACKWARD) + EVERY_G)
def test_forward_equals_the_spec(batches, L, H, O, act):
    import torch

    batch = batches(8)
    c = make_mlp_case(max(FORWARD_ROWS), L, H, O, seed=L * 7 + H, adversarial=False)
    want_y, want_h = mlp_spec(c["x"], c["w1t"], c["b1"], c["w2"], c["b2"], act)
    assert np.isfinite(want_y).all() and np.isfinite(want_h).all() and want_y.any() and want_h.any()
    head = head_with(batch, c, L, H, O, act)
    x_all = cuda(c["x"])
    for rows in FORWARD_ROWS:
        x = x_all[:rows].clone()
        y, hid = prefilled((rows, O)), prefilled((rows, H))
        torch.cuda.synchronize()
        batch._mlp_forward(head, x, y, hid)
        with torch.no_grad():
            plain = head(x)
        batch.synchronize()
        tag = f"{rows} rows of ({L}, {H}, {O}) {ACT[act]} against {NUMPY}"
        np.testing.assert_array_equal(bits32(y.cpu().numpy()), bits32(want_y[:rows]), err_msg=f"y, {tag}")
        np.testing.assert_array_equal(bits32(hid.cpu().numpy()), bits32(want_h[:rows]), err_msg=f"hidden, {tag}")
        np.testing.assert_array_equal(bits32(plain.cpu().numpy()), bits32(want_y[:rows]), err_msg=f"head(x), {tag}")


# ------------------------------------------------------------------------------------------------- 2. backward, adjacent rows
def _np(res):
    return dict(w1t=res.w1t.cpu().numpy(), b1=res.b1.cpu().numpy(), w2=res.w2.cpu().numpy(), b2=res.b2.cpu().numpy(),
                ga=None if res.grad_a is None else res.grad_a.cpu().numpy())


def assert_bits(got, want, tag, names=OUTS):
    for name in names:
        assert got[name].shape == want[name].shape, (name, tag)
        np.testing.assert_array_equal(bits32(got[name]), bits32(want[name]), err_msg=f"{name}, {tag}")


@pytest.mark.parametrize("s", BACKWARD, **IDS)
def test_backward_equals_the_reference(batches, host, s):
    import torch

    batch = batches(8)
    L, H, O, act = s.dims
    rows_set = backward_rows(s.r_adjacent)
    c = make_mlp_backward_case(max(rows_set), L, H, O, act, seed=L * 7 + H)
    want, ref = backward_reference(host, L, H, O, act, c["x"], c["hidden"], c["grad_y"], c["w2"], rows_set)
    assert all(np.isfinite(want[257][k]).all() and want[257][k].any() for k in OUTS)
    head = head_with(batch, c, L, H, O, act)
    xd, hd, gd = (cuda(c[k]) for k in ("x", "hidden", "grad_y"))
    for rows in rows_set:
        x, hidden, gy = xd[:rows].clone(), hd[:rows].clone(), gd[:rows].clone()
        out = batch.alloc_mlp_backward(head, (rows,), want_grad_a=True)
        assert out.workspace.numel() == -(-rows // 256) * (L * H + H + O * H + O) * 8
        for t in (out.w1t, out.b1, out.w2, out.b2, out.grad_a, out.workspace):
            t.view(torch.uint8).fill_(FILL)
        torch.cuda.synchronize()
        assert batch.mlp_backward(head, x, hidden, gy, out=out) is out
        bare = batch.mlp_backward(head, x, hidden, gy)
        batch.synchronize()
        tag = f"{rows} rows of ({L}, {H}, {O}) {ACT[act]}, sub-tiles of {s.r_adjacent} rows, against {ref}"
        assert_bits(_np(out), want[rows], tag)                               # every element: nothing of the fill is left
        assert bare.grad_a is None
        assert_bits(_np(bare), want[rows], f"without grad_a, {tag}", NAMES)


# ------------------------------------------------------------------------------------------------- 3. backward, picked rows
def make_sides(batch, keys, L, H, O, act, seed):
    from collectivecrossing_amd import SideHeads

    heads, params = {}, {}
    for i, key in enumerate(keys):
        c = make_mlp_case(1, L, H, O, seed=seed + 31 * i, adversarial=False)
        heads[key] = head_with(batch, c, L, H, O, act)
        params[id(heads[key])] = c
    sides = SideHeads(batch, heads)
    return sides, [params[id(h)] for _, h in sides.groups]


def picked_ms(R):
    """env-rows M such that M (one slot) and 2 M (two slots) are the row counts around sub-tiles of R rows and one block"""
    rows = backward_rows(R)
    return tuple(sorted({m for r in rows for m in (r, r // 2, (r + 1) // 2) if m >= 1}))


@pytest.mark.parametrize("L,H,O", SIDES_BACKWARD)
def test_picked_rows_backward_equals_the_reference_and_the_gathered_call(batches, host, L, H, O):
    import torch

    from collectivecrossing_amd import MlpGradResult

    s = by_dims(L, H, O)
    act, N = s.act, 3
    batch = batches(N)
    sides, _ = make_sides(batch, ("boarding", "exiting"), L, H, O, act, seed=L + H)
    assert [slots_of(m) for m, _ in sides.groups] == [[0, 1], [2]]
    Ms = picked_ms(s.r_picked)
    Mmax = max(Ms)
    c = make_mlp_backward_case(Mmax * N, L, H, O, act, seed=L * 3 + H)
    x_all, h_all, gy_all = (c[k].reshape(Mmax, N, -1) for k in ("x", "hidden", "grad_y"))
    refs = []
    for mask, head in sides.groups:
        sl = slots_of(mask)
        g = [np.ascontiguousarray(a[:, sl]).reshape(Mmax * len(sl), -1) for a in (x_all, h_all, gy_all)]
        refs.append(backward_reference(host, L, H, O, act, *g, head.w2.detach().cpu().numpy(), [m * len(sl) for m in Ms], calls=len(sides.groups)))
    xd, hd, gd = (cuda(a) for a in (x_all, h_all, gy_all))
    f = torch.float32
    for M in Ms:
        x, hid, gy = xd[:M].clone(), hd[:M].clone(), gd[:M].clone()
        outs = [MlpGradResult(*(prefilled(shape) for shape in ((L, H), (H,), (O, H), (O,))), prefilled((M, N, H)), None) for _ in sides.groups]
        torch.cuda.synchronize()
        got = sides.backward_into(x, hid, gy, out=outs)
        batch.synchronize()
        for (mask, head), o, (want, ref) in zip(sides.groups, got, refs):
            sl = slots_of(mask)
            S = len(sl)
            tag = (f"M = {M}, slots {sl} ({M * S} selected rows) of ({L}, {H}, {O}) {ACT[act]}, sub-tiles of {s.r_picked} rows "
                   f"(picked) and {s.r_adjacent} (adjacent)")
            gathered = batch.mlp_backward(head, x[:, sl].contiguous(), hid[:, sl].contiguous(), gy[:, sl].contiguous(), want_grad_a=True)
            batch.synchronize()
            ga = o.grad_a.cpu().numpy()
            mine = dict(_np(o), ga=np.ascontiguousarray(ga[:, sl]).reshape(M * S, H))
            theirs = _np(gathered)
            theirs["ga"] = theirs["ga"].reshape(M * S, H)
            assert_bits(mine, want[M * S], f"{tag}, against {ref}")
            assert_bits(mine, theirs, f"{tag}, against mlp_backward on the gathered rows")
            rest = np.ones(N, bool)
            rest[sl] = False
            assert (bits32(ga)[:, rest] == FILL32).all(), f"grad_a outside the group's rows was written, {tag}"
            assert o.grad_a.dtype == f and all(np.isfinite(want[M * S][k]).all() for k in OUTS)


# ------------------------------------------------------------------------------------------------- 4. sides forward
@pytest.mark.parametrize("L,H,O", SIDES_FORWARD)
@pytest.mark.parametrize("keys", (((0, 2),), ((1,),)), ids=("slots-0-2", "slot-1"))
def test_sides_forward_equals_the_spec_on_the_gathered_rows(batches, keys, L, H, O):
    """One group of two slots (2 M selected rows) and one of a single slot (M selected rows: the forward's own row counts);
    the slots of no group keep the fill."""
    import torch

    act, N = by_dims(L, H, O).act, 3
    batch = batches(N)
    sides, params = make_sides(batch, keys, L, H, O, act, seed=L + H + 5)
    assert not sides.all_owned
    Mmax = max(FORWARD_ROWS)
    x_all = make_mlp_case(Mmax * N, L, 16, 1, seed=L * 5 + H, adversarial=False)["x"].reshape(Mmax, N, L)
    want = []
    for (mask, _), c in zip(sides.groups, params):
        g = np.ascontiguousarray(x_all[:, slots_of(mask), :]).reshape(-1, L)
        want.append(mlp_spec(g, c["w1t"], c["b1"], c["w2"], c["b2"], act))
    xd = cuda(x_all)
    for M in FORWARD_ROWS:
        x = xd[:M].clone()
        y, hid = prefilled((M, N, O)), prefilled((M, N, H))
        torch.cuda.synchronize()
        with torch.no_grad():
            assert sides(x, out=y, hidden_out=hid) is y
        batch.synchronize()
        yb, hb = bits32(y.cpu().numpy()), bits32(hid.cpu().numpy())
        owned = np.zeros(N, bool)
        for (mask, _), (wy, wh) in zip(sides.groups, want):
            sl = slots_of(mask)
            owned[sl] = True
            S = len(sl)
            tag = f"M = {M}, slots {sl} ({M * S} selected rows) of ({L}, {H}, {O}) {ACT[act]} against {NUMPY}"
            np.testing.assert_array_equal(yb[:, sl].reshape(M * S, O), bits32(wy[:M * S]), err_msg=f"y, {tag}")
            np.testing.assert_array_equal(hb[:, sl].reshape(M * S, H), bits32(wh[:M * S]), err_msg=f"hidden, {tag}")
            assert np.isfinite(wy).all() and wy.any()
        assert (yb[:, ~owned] == FILL32).all() and (hb[:, ~owned] == FILL32).all(), f"rows of unowned slots were written, M = {M}"


# ------------------------------------------------------------------------------------------------- 5. fused launches, L = 206
@pytest.fixture(scope="module")
def fifty():
    """Three envs of the 50-agent workload ten greedy steps in: 150 rows of 206 floats, two tiles and a tail of 22."""
    import bench

    from collectivecrossing_amd.batched import BatchedCollectiveCrossing

    batch = BatchedCollectiveCrossing(bench.workload_config("c5_50")[0], 3)
    assert (batch.num_agents, batch.obs_len) == (50, 206)
    batch.make_reset_pool(seed0=5, size=64)
    batch.reset_from_pool()
    batch.set_rng_seed(SEED)
    batch.rollout_greedy(10, want_obs=False)
    obs, masks = batch.observe(), batch.action_masks()
    st = batch.get_state()
    state = (st["terminated"], st["truncated"], st["step_count"], st["episode"])
    yield batch, obs, masks, state
    batch.close()


def spread_params(L, H, O, seed):
    """Linear-style parameters with the first layer scaled down (observation rows hold coordinates) and the second up, so
    that the outputs spread and every action is taken."""
    w1t, b1, w2, b2 = linear_init(L, H, O, seed=seed)
    return dict(w1t=(w1t * np.float32(0.25)).astype(np.float32), b1=b1, w2=(w2 * np.float32(4.0)).astype(np.float32), b2=b2)


@pytest.mark.parametrize("H", (64, 256))
def test_fused_sampling_at_a_long_row_equals_the_two_launches_and_the_specs(fifty, H):
    import torch

    batch, obs, masks, state = fifty
    E, N, L = 3, 50, 206
    c = spread_params(L, H, 5, seed=H)
    head = head_with(batch, c, L, H, 5, TANH)
    obs_np, masks_np = obs.cpu().numpy(), masks.cpu().numpy()
    want_logits = mlp_spec(obs_np.reshape(E * N, L), c["w1t"], c["b1"], c["w2"], c["b2"], TANH)[0].reshape(E, N, 5)
    assert np.isfinite(want_logits).all()
    seen = set()
    for masked in (True, False):
        for det in (False, True):
            m, m_np = (masks, masks_np) if masked else (None, None)
            tag = f"H {H} masked {masked} deterministic {det}"
            lo = prefilled((E, N, 5))
            fused = batch.mlp_sample_actions(head, obs, m, deterministic=det, want_logp=True, want_entropy=True, logits_out=lo)
            with torch.no_grad():
                logits = head(obs)
            two = batch.sample_actions(logits, m, deterministic=det, want_logp=True, want_entropy=True)
            bare = batch.mlp_sample_actions(head, obs, m, deterministic=det, want_logp=False)
            batch.synchronize()
            want = dict(zip(("actions", "logp", "entropy"), sample_spec(want_logits, m_np, *state, seed=SEED, deterministic=det)))
            np.testing.assert_array_equal(bits32(lo.cpu().numpy()), bits32(logits.cpu().numpy()), err_msg=f"logits_out against head(obs), {tag}")
            np.testing.assert_array_equal(bits32(lo.cpu().numpy()), bits32(want_logits), err_msg=f"logits_out against {NUMPY}, {tag}")
            for name in ("actions", "logp", "entropy"):
                got = getattr(fused, name).cpu().numpy()
                view = bits32 if got.dtype == np.float32 else np.asarray
                np.testing.assert_array_equal(view(got), view(getattr(two, name).cpu().numpy()), err_msg=f"{name} against the two launches, {tag}")
                np.testing.assert_array_equal(view(got), view(want[name]), err_msg=f"{name} against the NumPy specs composed, {tag}")
            np.testing.assert_array_equal(bare.actions.cpu().numpy(), want["actions"], err_msg=f"no statistics, {tag}")
            seen |= set(np.unique(want["actions"]).tolist())
    assert len(seen - {255}) >= 4, seen                                     # the draws spread: no degenerate policy


@pytest.mark.parametrize("H", (64, 256))
def test_fused_q_actions_at_a_long_row_equals_the_kernels_composed_and_the_specs(fifty, H):
    import torch
    from _dueling_spec import dueling_spec

    from collectivecrossing_amd import QLearning

    batch, obs, masks, state = fifty
    E, N, L, O = 3, 50, 206, 6
    ql = QLearning(batch)
    c = spread_params(L, H, O, seed=H + 1)
    head = head_with(batch, c, L, H, O, TANH)
    obs_np, masks_np = obs.cpu().numpy(), masks.cpu().numpy()
    want_q = dueling_spec(mlp_spec(obs_np.reshape(E * N, L), c["w1t"], c["b1"], c["w2"], c["b2"], TANH)[0]).reshape(E, N, 5)
    assert np.isfinite(want_q).all()
    explored = 0
    for masked in (True, False):
        m, m_np = (masks, masks_np) if masked else (None, None)
        for eps in (None, 0.25):
            tag = f"H {H} O {O} masked {masked} eps {eps}"
            if eps is not None:
                ql.epsilon = eps
            out = ql.alloc_q_actions(want_explored=True)
            out.actions.fill_(FILL)
            out.explored.fill_(FILL)
            q_out = prefilled((E, N, 5))
            assert ql.mlp_q_actions(head, obs, m, greedy=eps is None, q_out=q_out, out=out) is out
            with torch.no_grad():
                q = ql.dueling(head(obs))
            two = ql.q_actions(q, m, greedy=eps is None, want_explored=True)
            batch.synchronize()
            want = q_actions_spec(want_q, m_np, *state, seed=SEED, epsilon=eps)
            np.testing.assert_array_equal(bits32(q_out.cpu().numpy()), bits32(q.cpu().numpy()), err_msg=f"q_out against the kernels composed, {tag}")
            np.testing.assert_array_equal(bits32(q_out.cpu().numpy()), bits32(want_q), err_msg=f"q_out against the NumPy specs composed, {tag}")
            for name, w in (("actions", want[0]), ("explored", want[1])):
                got = getattr(out, name).cpu().numpy()
                np.testing.assert_array_equal(got, getattr(two, name).cpu().numpy(), err_msg=f"{name} against the kernels composed, {tag}")
                np.testing.assert_array_equal(got, w, err_msg=f"{name} against the NumPy specs composed, {tag}")
            explored += int(want[1].sum())
    assert explored > 0
