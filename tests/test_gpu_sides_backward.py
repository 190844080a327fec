"""The backward pass of per-side policy heads on the device (include/ccx.h: CCX_SIDES, backward): ``backward_into`` per
group bit for bit against BOTH ``mlp_backward`` on the gathered, contiguous rows and the NumPy spec
(tests/_mlp_backward_spec.py) on those rows, on row counts that cross the 64-row sub-tiles and the 256-row blocks of the
SELECTED rows; ``grad_a`` written at a group's rows only; the autograd path through ``ppo_loss`` against an
``MlpHead(backward="device")`` twin; and the end-to-end property: logits re-evaluated on a [K, E, N, L] batch give
``approx_kl == 0`` and ``clip_frac == 0`` per side.  f32 values are compared as bit patterns."""

import numpy as np
import pytest
from _mlp_backward_spec import NAMES, make_mlp_backward_case, mlp_backward_spec
from _mlp_spec import RELU, TANH, bits32, make_mlp_case
from _reset_obs_spec import make_config
from _split_step_cases import make_config as make_grid_config

pytestmark = pytest.mark.gpu

ACT = {TANH: "tanh", RELU: "relu"}
SEED = 0x0123_4567_89AB_CDEF
FILL = 0xA5
# the forward's sets (tests/test_gpu_sides.py) and 513 selected rows: N = 3 has S = 2 and S = 1, so M = 255 / 256 / 257 / 513
# are those counts for the exiting side and M = 128 / 129 cross a block of the boarding side's 2 M
MS_N3 = (1, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257, 513)
# N = 8 has S = 5 and S = 3: 5 M and 3 M cross 64 at 12 / 13 and 21 / 22, 256 at 51 / 52 and 85 / 86; 3 * 171 = 513
MS_N8 = (1, 12, 13, 21, 22, 51, 52, 85, 86, 171, 1000)
SPEC_MS_N8 = (1, 13, 52, 86, 171)                                           # the spec walks its chains in Python


@pytest.fixture(scope="module")
def batches():
    import torch

    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    from collectivecrossing_amd.batched import BatchedCollectiveCrossing

    made = {}

    def get(N, E=64):
        if (N, E) not in made:
            # (64 agents exceed the config validator's cap for any grid: built without validation, as the recorded fixture is)
            cfg = make_config(N, max_steps=12) if N <= 8 else make_grid_config(32, 16, N, nb=N // 2, max_steps=12)
            b = BatchedCollectiveCrossing(cfg, E)
            b.make_reset_pool(seed0=5, size=256)
            made[N, E] = b
        return made[N, E]

    yield get
    for b in made.values():
        b.close()


def slots_of(mask):
    return [a for a in range(64) if mask >> a & 1]


def make_sides(batch, keys, L, H, O, act, seed=0, backward="torch"):
    import torch

    from collectivecrossing_amd import SideHeads

    heads = {}
    for i, key in enumerate(keys):
        c = make_mlp_case(1, L, H, O, seed=seed + 31 * i)
        head = batch.mlp_head(H, O, ACT[act], L=L, backward=backward)
        with torch.no_grad():
            for name in ("w1t", "b1", "w2", "b2"):
                getattr(head, name).copy_(torch.from_numpy(c[name]))
        heads[key] = head
    return SideHeads(batch, heads)


def _np(res):
    return {k: getattr(res, k).cpu().numpy() for k in NAMES}


def check_backward(batch, sides, N, Ms, spec_ms, act, seed):
    import torch

    from collectivecrossing_amd import MlpGradResult

    L, H, O = sides.L, sides.H, sides.O
    Mmax = max(Ms)
    c = make_mlp_backward_case(Mmax * N, L, H, O, act, seed=seed)
    x_all, h_all, gy_all = (c[k].reshape(Mmax, N, -1) for k in ("x", "hidden", "grad_y"))
    spec = []
    for mask, head in sides.groups:
        sl = slots_of(mask)
        g = [np.ascontiguousarray(a[:, sl]).reshape(Mmax * len(sl), -1) for a in (x_all, h_all, gy_all)]
        spec.append(mlp_backward_spec(*g, head.w2.detach().cpu().numpy(), act, rows=[m * len(sl) for m in spec_ms]) if spec_ms else {})
    xd, hd, gd = (torch.from_numpy(a).cuda() for a in (x_all, h_all, gy_all))
    fill = np.frombuffer(bytes([FILL] * 4), np.uint32)[0]
    f = torch.float32
    for M in Ms:
        x, hid, gy = xd[:M].clone(), hd[:M].clone(), gd[:M].clone()
        outs = [MlpGradResult(*(torch.empty(s, dtype=f, device="cuda") for s in ((L, H), (H,), (O, H), (O,))),
                              torch.empty((M, N, H), dtype=f, device="cuda"), None) for _ in sides.groups]
        for o in outs:
            for t in (o.w1t, o.b1, o.w2, o.b2, o.grad_a):
                t.view(torch.uint8).fill_(FILL)
        torch.cuda.synchronize()
        got = sides.backward_into(x, hid, gy, out=outs)
        bare = sides.backward_into(x, hid, gy)                             # allocates; no grad_a
        batch.synchronize()
        assert all(b.grad_a is None for b in bare)
        for k, ((mask, head), o, b) in enumerate(zip(sides.groups, got, bare)):
            sl = slots_of(mask)
            S = len(sl)
            tag = f"M = {M}, slots {sl} ({M * S} selected rows)"
            ref = batch.mlp_backward(head, x[:, sl].contiguous(), hid[:, sl].contiguous(), gy[:, sl].contiguous(), want_grad_a=True)
            batch.synchronize()
            ga = o.grad_a.cpu().numpy()
            for name in NAMES:
                np.testing.assert_array_equal(bits32(_np(o)[name]), bits32(_np(ref)[name]), err_msg=f"{name} against mlp_backward, {tag}")
                np.testing.assert_array_equal(bits32(_np(b)[name]), bits32(_np(ref)[name]), err_msg=f"{name} without grad_a, {tag}")
            np.testing.assert_array_equal(bits32(ga[:, sl]), bits32(ref.grad_a.cpu().numpy()), err_msg=f"grad_a against mlp_backward, {tag}")
            rest = np.ones(N, bool)
            rest[sl] = False
            assert (bits32(ga)[:, rest] == fill).all(), f"grad_a outside the group's rows was written, {tag}"
            if M in spec_ms:
                want = spec[k][M * S]
                for name in NAMES:
                    np.testing.assert_array_equal(bits32(_np(o)[name]), bits32(want[name]), err_msg=f"{name} against the spec, {tag}")
                np.testing.assert_array_equal(bits32(ga[:, sl].reshape(M * S, H)), bits32(want["ga"]), err_msg=f"grad_a against the spec, {tag}")
                assert all(np.isfinite(want[name]).all() for name in NAMES) and want["w1t"].any()


# ------------------------------------------------------------------------------------------------- 1. backward_into
def test_two_sides_of_three_agents(batches):
    batch = batches(3)
    sides = make_sides(batch, ("boarding", "exiting"), 18, 16, 5, TANH, seed=3)
    check_backward(batch, sides, 3, MS_N3, MS_N3, TANH, seed=4)


def test_two_sides_of_eight_agents(batches):
    batch = batches(8)
    sides = make_sides(batch, ("boarding", "exiting"), 38, 64, 5, TANH, seed=8)
    check_backward(batch, sides, 8, MS_N8, SPEC_MS_N8, TANH, seed=9)


def test_three_groups_with_unowned_slots_and_a_relu_critic(batches):
    batch = batches(8)
    sides = make_sides(batch, ((0, 2, 5), (1,), (6, 7)), 38, 32, 1, RELU, seed=5)
    check_backward(batch, sides, 8, (1, 22, 86, 257), (1, 86, 257), RELU, seed=6)


def test_an_odd_row_length(batches):
    batch = batches(4, 8)
    sides = make_sides(batch, ("boarding", "exiting"), 7, 16, 1, RELU, seed=7)
    check_backward(batch, sides, 4, (1, 65, 129), (1, 65, 129), RELU, seed=8)


def test_the_limits(batches):
    """L = 262, H = 256, O = 8: sub-tiles of 16 rows (ccx_mlp_grad::sub_rows; 8 rows begin at L = 372, which
    tests/test_gpu_mlp_shapes.py runs), the flat rows beside w2 in LDS (kernel against kernel: the spec's Python loop over
    69 000 elements is tests/test_mlp_backward_spec.py's business)."""
    batch = batches(64, 4)
    sides = make_sides(batch, (tuple(range(1, 64, 2)),), 262, 256, 8, TANH, seed=9)
    check_backward(batch, sides, 64, (5,), (), TANH, seed=10)


def test_static_buffers_and_a_shared_grad_a(batches):
    import torch

    batch = batches(8)
    sides = make_sides(batch, ("boarding", "exiting"), 38, 64, 5, TANH, seed=11)
    M, N = 40, 8
    c = make_mlp_backward_case(M * N, 38, 64, 5, TANH, seed=12)
    x, hid, gy = (torch.from_numpy(c[k].reshape(M, N, -1)).cuda() for k in ("x", "hidden", "grad_y"))
    out = sides.alloc_backward((M, N), want_grad_a=True)
    assert out[0].grad_a is out[1].grad_a and [o.workspace.numel() for o in out] == [(38 * 64 + 64 + 5 * 64 + 5) * 8] * 2
    for fill in (0xEE, 0x55):
        for o in out:
            for t in (o.w1t, o.b1, o.w2, o.b2, o.grad_a, o.workspace):
                t.view(torch.uint8).fill_(fill)
        torch.cuda.synchronize()
        got = sides.backward_into(x, hid, gy, out=out)
        assert all(g is o for g, o in zip(got, out))
        shaped = sides.backward_into(x.view(5, 8, N, 38), hid.view(5, 8, N, 64), gy.view(5, 8, N, 5), want_grad_a=True)
        batch.synchronize()
        assert tuple(shaped[0].grad_a.shape) == (5, 8, N, 64)
        for (mask, head), o, s in zip(sides.groups, got, shaped):
            sl = slots_of(mask)
            ref = batch.mlp_backward(head, x[:, sl].contiguous(), hid[:, sl].contiguous(), gy[:, sl].contiguous(), want_grad_a=True)
            batch.synchronize()
            for name in NAMES:
                np.testing.assert_array_equal(bits32(_np(o)[name]), bits32(_np(ref)[name]), err_msg=f"{name}, fill {fill:#x}")
                np.testing.assert_array_equal(bits32(_np(s)[name]), bits32(_np(ref)[name]), err_msg=f"{name}, a [5, 8] leading shape")
            np.testing.assert_array_equal(bits32(o.grad_a[:, sl].cpu().numpy()), bits32(ref.grad_a.cpu().numpy()))
            np.testing.assert_array_equal(bits32(s.grad_a.view(M, N, 64)[:, sl].cpu().numpy()), bits32(ref.grad_a.cpu().numpy()))


# ------------------------------------------------------------------------------------------------- 2. autograd
def _actor_loop(batch, actors, K):
    """K steps of sample_actions -> rollout from a state in which some agents are done; what a learner stores."""
    import torch

    E, N, L = batch.num_envs, batch.num_agents, batch.obs_len
    batch.reset_from_pool()
    batch.set_rng_seed(SEED)
    batch.rollout_greedy(6, want_obs=False)
    obs, masks = batch.observe(), batch.action_masks()
    rows = torch.empty((K, E, N, L), dtype=torch.float32, device="cuda")
    mk, acts = (torch.empty((K, E, N), dtype=torch.uint8, device="cuda") for _ in range(2))
    logp = torch.empty((K, E, N), dtype=torch.float32, device="cuda")
    out = batch.alloc_rollout(1)
    for s in range(K):
        rows[s].copy_(obs)
        mk[s].copy_(masks)
        res = actors.sample_actions(obs, masks)
        acts[s].copy_(res.actions)
        logp[s].copy_(res.logp)
        batch.rollout(res.actions[None], auto_reset=True, out=out, masks_out=masks, reset_obs="next")
        obs.copy_(out.obs[0])
    return rows, mk, acts, logp


def _policy_sides(batch, keys, seed, backward="torch"):
    import torch

    from collectivecrossing_amd import SideHeads

    torch.manual_seed(seed)
    heads = {}
    for key in keys:
        head = batch.mlp_head(64, backward=backward)
        with torch.no_grad():
            head.w2.mul_(4.0)
            head.w1t.mul_(0.25)
        heads[key] = head
    return SideHeads(batch, heads)


@pytest.mark.parametrize("keys", (("boarding", "exiting"), ("exiting",)))
def test_autograd_through_ppo_loss_equals_a_device_backward_twin(batches, keys):
    import torch

    batch = batches(8)
    E, N, K = 64, 8, 8
    actors = _policy_sides(batch, keys, seed=21)
    rows, mk, acts, logp = _actor_loop(batch, actors, K)
    gen = torch.Generator(device="cuda").manual_seed(5)
    adv = torch.randn((K, E, N), device="cuda", generator=gen)
    zeros = torch.zeros((K, E, N), device="cuda")
    with torch.no_grad():
        actors.heads[0].w2.mul_(1.01)                                      # one update later: the ratio is no longer 1
    logits = actors(rows)
    assert logits.requires_grad
    logits.retain_grad()
    with torch.no_grad():
        plain = actors(rows)
    np.testing.assert_array_equal(bits32(logits.detach().cpu().numpy()), bits32(plain.cpu().numpy()))   # the same bits under grad
    batch.ppo_loss(logits, zeros, acts, logp, adv, zeros, masks=mk).loss.backward()
    batch.synchronize()
    gl = logits.grad
    assert gl is not None and bool((gl != 0).any())
    for mask, head in actors.groups:
        sl = slots_of(mask)
        twin = batch.mlp_head(64, backward="device")
        with torch.no_grad():
            for p, q in zip(twin.parameters(), head.parameters()):
                p.copy_(q)
        twin(rows[:, :, sl].contiguous()).backward(gl[:, :, sl].contiguous())
        batch.synchronize()
        for name in NAMES:
            got, want = getattr(head, name).grad, getattr(twin, name).grad
            assert got is not None and bool((want != 0).any()), name
            np.testing.assert_array_equal(bits32(got.cpu().numpy()), bits32(want.cpu().numpy()), err_msg=f"{name}.grad, slots {sl}")


def test_frozen_members_get_no_gradient(batches):
    import torch

    batch = batches(8)
    sides = _policy_sides(batch, ("boarding", "exiting"), seed=22)
    for p in sides.heads[0].parameters():
        p.requires_grad_(False)
    x = torch.randn((3, 8, 8, 38), device="cuda")
    sides(x).sum().backward()
    batch.synchronize()
    assert all(p.grad is None for p in sides.heads[0].parameters()) and all(p.grad is not None for p in sides.heads[1].parameters())


# ------------------------------------------------------------------------------------------------- 3. the ratio is exactly 1
def test_approx_kl_and_clip_frac_are_zero_per_side_before_the_first_update(batches):
    import torch

    batch = batches(8)
    E, N, K = 64, 8, 8
    actors = _policy_sides(batch, ("boarding", "exiting"), seed=23)
    rows, mk, acts, logp = _actor_loop(batch, actors, K)
    gen = torch.Generator(device="cuda").manual_seed(6)
    adv = torch.randn((K, E, N), device="cuda", generator=gen)
    zeros = torch.zeros((K, E, N), device="cuda")
    with torch.no_grad():
        logits = actors(rows)                                              # ONE call on [K, E, N, L]
    live = acts != 255
    assert len(np.unique(acts.cpu().numpy())) == 6
    for i, (mask, _) in enumerate(actors.groups):
        valid = (live & actors.slot_mask(i).bool()).to(torch.uint8).contiguous()
        r = batch.ppo_loss(logits, zeros, acts, logp, adv, zeros, masks=mk, valid=valid)
        batch.synchronize()
        stats = r.stats.cpu().numpy()
        print(f"slots {slots_of(mask)}: approx_kl = {stats[4]!r}, clip_frac = {stats[5]!r}, count = {stats[6]!r}")
        assert stats[6] == float(valid.sum()) and stats[6] > 0
        assert stats[4] == 0.0 and stats[5] == 0.0
