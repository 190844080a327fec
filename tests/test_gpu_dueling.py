"""CCX_DUELING on the device (include/ccx.h): the dueling combine, forward and backward, against the NumPy spec
(tests/_dueling_spec.py) on row counts around a wave; ``dueling_into`` of several pairs; autograd down to an ``MlpHead``'s
parameters; and the fused actor launches ``mlp_q_actions`` / ``sides_q_actions`` against (i) the existing kernels composed
(``head(obs)`` -> ``dueling`` -> ``q_actions``) and (ii) the NumPy specs composed, in a stepped and auto-reset state, on slot
counts around one tile, plain (O = 5) and dueling (O = 6); the largest row; a captured actor step; the refusals; the example,
twice.  f32 values are compared as bit patterns (NaN payloads excepted: tests/_mlp_spec.bits32c)."""

import ctypes as C
import importlib.util
from pathlib import Path

import numpy as np
import pytest
from _dueling_spec import dueling_backward_spec, dueling_spec, make_dueling_rows
from _mlp_spec import RELU, TANH, bits32, bits32c, linear_init, mlp_spec
from _qlearn_spec import make_q_case, q_actions_spec
from _reset_obs_spec import make_config
from _split_step_cases import make_config as make_grid_config

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
SEED = 0x0123_4567_89AB_CDEF
FILL = 0xA5
FILL32 = int(np.frombuffer(bytes([FILL] * 4), np.uint32)[0])
ACT = {TANH: "tanh", RELU: "relu"}
ROWS = (1, 63, 64, 65, 257, 1000)


@pytest.fixture(scope="module")
def batches():
    import torch

    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    from collectivecrossing_amd.batched import BatchedCollectiveCrossing

    made = {}

    def get(N, E):
        if (N, E) not in made:
            cfg = make_config(N, max_steps=12) if N <= 8 else make_grid_config(32, 16, N, nb=N // 2, max_steps=40)
            b = BatchedCollectiveCrossing(cfg, E)
            assert b.num_agents == N
            b.make_reset_pool(seed0=7, size=64)
            made[N, E] = b
        return made[N, E]

    yield get
    for b in made.values():
        b.close()


@pytest.fixture(scope="module")
def ql8(batches):
    """One 8-agent batch and its QLearning for the row-wise tests (they never read the env state)."""
    from collectivecrossing_amd import QLearning

    b = batches(8, 4)
    return b, QLearning(b)


def prefilled(shape, dtype=None):
    import torch

    t = torch.empty(shape, dtype=dtype or torch.float32, device="cuda")
    t.view(torch.uint8).fill_(FILL)
    return t


def cuda(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


# ------------------------------------------------------------------------------------------------- 1. the stand-alone kernels
@pytest.fixture(scope="module")
def rows_case():
    va, g = make_dueling_rows(max(ROWS), seed=11, special=True)
    return va, g, dueling_spec(va), dueling_backward_spec(g)


@pytest.mark.parametrize("M", ROWS)
def test_forward_and_backward_equal_the_spec(ql8, rows_case, M):
    batch, ql = ql8
    va, g, want_q, want_gva = rows_case
    q, gva = prefilled((M, 5)), prefilled((M, 6))
    assert ql.dueling(cuda(va[:M]), out=q) is q and ql.dueling_backward(cuda(g[:M]), out=gva) is gva
    fresh_q, fresh_g = ql.dueling(cuda(va[:M])), ql.dueling_backward(cuda(g[:M]))
    batch.synchronize()
    for got, want, name in ((q, want_q, "q"), (fresh_q, want_q, "q (allocated)"), (gva, want_gva, "grad_va"), (fresh_g, want_gva, "grad_va (allocated)")):
        np.testing.assert_array_equal(bits32c(got.cpu().numpy()), bits32c(want[:M]), err_msg=f"{name}, M = {M}")    # every element: no FILL left
    if M >= 64:
        assert np.isnan(want_q[:M]).any() and np.isinf(want_q[:M]).any()


def test_leading_shapes_and_zero_rows(ql8, rows_case):
    batch, ql = ql8
    va, g, want_q, want_gva = rows_case
    q = ql.dueling(cuda(va[:6 * 8 * 8].reshape(6, 8, 8, 6)))
    gva = ql.dueling_backward(cuda(g[:6 * 8 * 8].reshape(6, 8, 8, 5)))
    batch.synchronize()
    assert q.shape == (6, 8, 8, 5) and gva.shape == (6, 8, 8, 6)
    np.testing.assert_array_equal(bits32c(q.cpu().numpy().reshape(-1, 5)), bits32c(want_q[:384]))
    np.testing.assert_array_equal(bits32c(gva.cpu().numpy().reshape(-1, 6)), bits32c(want_gva[:384]))
    empty = cuda(va[:0].reshape(0, 8, 6))
    assert ql.dueling(empty).shape == (0, 8, 5) and ql.dueling_backward(cuda(g[:0])).shape == (0, 6)
    assert ql.dueling(empty.clone().requires_grad_()).shape == (0, 8, 5)


@pytest.mark.parametrize("num", (1, 3, 4))
def test_dueling_into_of_several_pairs_equals_single_calls(ql8, num):
    batch, ql = ql8
    M = 257
    vas = [cuda(make_dueling_rows(M, seed=20 + i, special=i == 1)[0]) for i in range(num)]
    qs = tuple(prefilled((M, 5)) for _ in range(num))
    got = ql.dueling_into(tuple(vas), qs)
    single = [ql.dueling(v) for v in vas]
    batch.synchronize()
    assert all(a is b for a, b in zip(got, qs))
    for i in range(num):
        np.testing.assert_array_equal(bits32(qs[i].cpu().numpy()), bits32(single[i].cpu().numpy()), err_msg=f"pair {i} of {num}")
        np.testing.assert_array_equal(bits32c(qs[i].cpu().numpy()), bits32c(dueling_spec(vas[i].cpu().numpy())))
    if num == 1:                                                         # a single pair may be given as two tensors
        again = prefilled((M, 5))
        ql.dueling_into(vas[0], again)
        batch.synchronize()
        np.testing.assert_array_equal(bits32(again.cpu().numpy()), bits32(qs[0].cpu().numpy()))


def test_autograd_reaches_the_parameters_of_a_dueling_head(ql8):
    import torch

    batch, ql = ql8
    M = 257
    torch.manual_seed(3)
    head = batch.mlp_head(16, O=6, backward="device")
    x = torch.randn((M, head.L), device="cuda")
    gq = torch.randn((M, 5), device="cuda")
    gq[::7] = 0.0                                                        # rows that do not count: td_loss_backward's +0.0
    q = ql.dueling(head(x))
    assert q.requires_grad and q.shape == (M, 5)
    q.backward(gq)
    with torch.no_grad():
        hidden = torch.empty((M, head.H), device="cuda")
        va = head(x, hidden_out=hidden)
        want_q = ql.dueling(va)
        gva = ql.dueling_backward(gq)
        ref = batch.mlp_backward(head, x, hidden, gva)
    batch.synchronize()
    assert torch.equal(q.detach().view(torch.int32), want_q.view(torch.int32))
    assert not gva[::7].view(torch.int32).any() and gva[1].abs().sum() > 0
    for p, g in zip((head.w1t, head.b1, head.w2, head.b2), (ref.w1t, ref.b1, ref.w2, ref.b2)):
        assert torch.equal(p.grad.view(torch.int32), g.view(torch.int32)) and torch.isfinite(p.grad).all() and p.grad.abs().sum() > 0
    with pytest.raises(ValueError, match="out="):
        ql.dueling(head(x), out=torch.empty((M, 5), device="cuda"))


def test_zero_gradient_rows_get_positive_zeros_although_va_holds_nan(ql8):
    import torch

    batch, ql = ql8
    M = 130
    va = cuda(make_dueling_rows(M, seed=4)[0])
    va[::3] = float("nan")
    va[1::3, 2] = float("inf")
    va.requires_grad_()
    gq = torch.randn((M, 5), device="cuda")
    gq[::3] = 0.0
    gq[1::3] = 0.0
    q = ql.dueling(va)
    q.backward(gq)
    batch.synchronize()
    assert torch.isnan(q[::3]).all() and va.grad.shape == (M, 6)
    assert not va.grad[::3].view(torch.int32).any() and not va.grad[1::3].view(torch.int32).any()      # +0.0: no bit set
    assert torch.isfinite(va.grad).all() and (va.grad[2::3] != 0).any()
    np.testing.assert_array_equal(bits32(va.grad.cpu().numpy()), bits32(dueling_backward_spec(gq.cpu().numpy())))


# ------------------------------------------------------------------------------------------------- 2. fused, one head
def stepped_state(batch, N, E):
    """test_q_actions_bits_in_a_stepped_state's state: 17 random steps with auto-reset at max_steps = 12 (a second episode,
    agents that have arrived), then the generator's dead slots and far counters in every other env.  Returns the state
    tuple of q_actions_spec, the dead slots, the rows, and the generator's masks."""
    import torch

    batch.reset_from_pool()
    batch.set_rng_seed(SEED)
    rng = np.random.default_rng(N * 100 + E)
    batch.rollout(torch.from_numpy(rng.integers(0, 5, size=(17, E, N), dtype=np.uint8)).cuda(), auto_reset=True, want_traj=False)
    case = make_q_case(E, N, seed=E * 100 + N)
    st = batch.get_state()
    half = np.arange(E) % 2 == 1
    batch.set_state(terminated=st["terminated"] | case["terminated"], truncated=st["truncated"] | case["truncated"],
                    step_count=np.where(half, case["step_count"], st["step_count"]).astype(np.int32),
                    episode=np.where(half, case["episode"], st["episode"]).astype(np.int32))
    st = batch.get_state()
    state = (st["terminated"], st["truncated"], st["step_count"], st["episode"])
    dead = (st["terminated"] | st["truncated"]) != 0
    assert dead.any() and not dead.all() and len(np.unique(st["step_count"])) > 2 and len(np.unique(st["episode"])) > 2
    return state, dead, batch.observe(), case["masks"]


def spec_q(obs_np, params, act, O):
    """The NumPy specs composed: CCX_MLP on the rows, then the dueling combine where O == 6."""
    y = mlp_spec(obs_np.reshape(-1, obs_np.shape[-1]), *params, act)[0]
    return (dueling_spec(y) if O == 6 else y).reshape(obs_np.shape[:-1] + (5,))


def head_with(batch, params, H, O, act):
    import torch

    head = batch.mlp_head(H, O, ACT[act])
    with torch.no_grad():
        for p, v in zip((head.w1t, head.b1, head.w2, head.b2), params):
            p.copy_(torch.from_numpy(v))
    return head


def choose_params(L, H, O, obs_np, masks_np, state, dead, first_seed):
    """Linear-style parameters (the second layer scaled up so that the Q-values spread), the first seed for which the CPU
    spec shows what a run has to exercise: an explored slot at the rate 0.25, and a live slot whose unmasked greedy action
    is masked off."""
    for seed in range(first_seed, first_seed + 50):
        w1t, b1, w2, b2 = linear_init(L, H, O, seed=seed)
        params = (w1t, b1, (w2 * np.float32(4.0)).astype(np.float32), b2)
        q = spec_q(obs_np, params, TANH, O)
        free = q_actions_spec(q, None, *state, seed=SEED, epsilon=None)[0]
        masked = q_actions_spec(q, masks_np, *state, seed=SEED, epsilon=None)[0]
        explored = q_actions_spec(q, masks_np, *state, seed=SEED, epsilon=0.25)[1]
        if explored.any() and ((free != masked) & ~dead).any():
            return params
    raise AssertionError("no seed gives an explored slot and a masked-off greedy candidate")


@pytest.mark.parametrize("H", (16, 64))                                   # wave 0 alone, and with three other waves
@pytest.mark.parametrize("N,E", [(3, 21), (3, 22), (8, 8), (8, 9)])      # 63 / 66 and 64 / 72 slots: around one tile
def test_mlp_q_actions_equals_the_kernels_composed_and_the_specs_composed(batches, N, E, H):
    import torch

    from collectivecrossing_amd import QLearning

    batch = batches(N, E)
    state, dead, obs, masks_np = stepped_state(batch, N, E)
    obs_np, masks = obs.cpu().numpy(), cuda(masks_np)
    ql = QLearning(batch)
    acts = (TANH, RELU) if (N, E, H) == (8, 9, 64) else (TANH,)
    for O, act in [(O, a) for O in (5, 6) for a in acts]:
        params = choose_params(batch.obs_len, H, O, obs_np, masks_np, state, dead, first_seed=10 * N + O)
        head = head_with(batch, params, H, O, act)
        want_q = spec_q(obs_np, params, act, O)
        for masked in (True, False):
            m, m_np = (masks, masks_np) if masked else (None, None)
            for eps in (None, 0.0, 0.25, 1.0):
                tag = f"N {N} E {E} H {H} O {O} {ACT[act]} masked {masked} eps {eps}"
                if eps is not None:
                    ql.epsilon = eps
                out = ql.alloc_q_actions(want_explored=True)
                out.actions.fill_(FILL)
                out.explored.fill_(FILL)
                q_out = prefilled((E, N, 5))
                fused = ql.mlp_q_actions(head, obs, m, greedy=eps is None, q_out=q_out, out=out)
                assert fused is out
                bare = ql.mlp_q_actions(head, obs, m, greedy=eps is None)            # no explored, no q_out
                with torch.no_grad():                                                # (i) the existing kernels composed
                    y = head(obs)
                    q = ql.dueling(y) if O == 6 else y
                two = ql.q_actions(q, m, greedy=eps is None, want_explored=True)
                batch.synchronize()
                assert bare.explored is None
                np.testing.assert_array_equal(fused.actions.cpu().numpy(), two.actions.cpu().numpy(), err_msg="actions, kernels " + tag)
                np.testing.assert_array_equal(fused.explored.cpu().numpy(), two.explored.cpu().numpy(), err_msg="explored, kernels " + tag)
                np.testing.assert_array_equal(bits32(q_out.cpu().numpy()), bits32(q.cpu().numpy()), err_msg="q_out, kernels " + tag)
                np.testing.assert_array_equal(bare.actions.cpu().numpy(), fused.actions.cpu().numpy(), err_msg="bare " + tag)
                want = q_actions_spec(want_q, m_np, *state, seed=SEED, epsilon=eps)   # (ii) the specs composed
                np.testing.assert_array_equal(fused.actions.cpu().numpy(), want[0], err_msg="actions, specs " + tag)
                np.testing.assert_array_equal(fused.explored.cpu().numpy(), want[1], err_msg="explored, specs " + tag)
                np.testing.assert_array_equal(bits32c(q_out.cpu().numpy()), bits32c(want_q), err_msg="q_out, specs " + tag)
                assert (want[0][dead] == 255).all() and not want[1][dead].any() and (want[0][~dead] <= 4).all()
                if eps == 0.25 and masked and act == TANH:
                    assert want[1].any() and not want[1].all(), tag
                if eps is None and masked and act == TANH:
                    free = q_actions_spec(want_q, None, *state, seed=SEED, epsilon=None)[0]
                    assert ((free != want[0]) & ~dead).any(), "no masked-off greedy candidate: " + tag


# ------------------------------------------------------------------------------------------------- 3. fused, sides
def sides_with(batch, keys, H, O, seed):
    from collectivecrossing_amd import SideHeads

    heads, params = {}, []
    for i, key in enumerate(keys):
        w1t, b1, w2, b2 = linear_init(batch.obs_len, H, O, seed=seed + 31 * i)
        p = (w1t, b1, (w2 * np.float32(4.0)).astype(np.float32), b2)
        heads[key] = head_with(batch, p, H, O, TANH)
        params.append((id(heads[key]), p))
    sides = SideHeads(batch, heads)
    by_id = dict(params)
    return sides, [by_id[id(h)] for _, h in sides.groups]


def slots_of(mask):
    return [a for a in range(64) if mask >> a & 1]


@pytest.mark.parametrize("E,N", ((64, 3), (100, 3), (64, 8), (100, 8)))
def test_sides_q_actions_equals_the_kernels_composed_and_the_specs_composed(batches, E, N):
    import torch

    from collectivecrossing_amd import QLearning

    batch = batches(N, E)
    state, dead, obs, masks_np = stepped_state(batch, N, E)
    obs_np, masks = obs.cpu().numpy(), cuda(masks_np)
    ql = QLearning(batch)
    seen = set()
    for O in (5, 6):
        for keys in (("boarding", "exiting"), ("boarding",)):
            sides, params = sides_with(batch, keys, 64, O, seed=N + O)
            owned = np.array([bool(sides.owned >> a & 1) for a in range(N)])
            assert owned.all() == (len(keys) == 2)
            want_q = np.zeros((E, N, 5), np.float32)
            for (mask, _), p in zip(sides.groups, params):
                sl = slots_of(mask)
                want_q[:, sl] = spec_q(np.ascontiguousarray(obs_np[:, sl]), p, TANH, O)
            for masked, eps in ((True, 0.25), (False, 0.25), (True, None), (False, 1.0), (True, 0.0)):
                m, m_np = (masks, masks_np) if masked else (None, None)
                tag = f"E {E} N {N} O {O} owned {sides.owned:#x} masked {masked} eps {eps}"
                if eps is not None:
                    ql.epsilon = eps
                out = ql.alloc_q_actions(want_explored=True)
                out.actions.fill_(FILL)
                out.explored.fill_(FILL)
                q_out = prefilled((E, N, 5))
                fused = ql.sides_q_actions(sides, obs, m, greedy=eps is None, q_out=q_out, out=out)
                bare = ql.sides_q_actions(sides, obs, m, greedy=eps is None)
                with torch.no_grad():
                    y = sides(obs)                                                   # (+0.0 at unowned rows)
                    q = ql.dueling(y) if O == 6 else y
                two = ql.q_actions(q, m, greedy=eps is None, want_explored=True)
                batch.synchronize()
                fa, fe, fq = fused.actions.cpu().numpy(), fused.explored.cpu().numpy(), q_out.cpu().numpy()
                np.testing.assert_array_equal(fa[:, owned], two.actions.cpu().numpy()[:, owned], err_msg="actions, kernels " + tag)
                np.testing.assert_array_equal(fe[:, owned], two.explored.cpu().numpy()[:, owned], err_msg="explored, kernels " + tag)
                np.testing.assert_array_equal(bits32(fq)[:, owned], bits32(q.cpu().numpy())[:, owned], err_msg="q_out, kernels " + tag)
                want = q_actions_spec(want_q, m_np, *state, seed=SEED, epsilon=eps)
                np.testing.assert_array_equal(fa[:, owned], want[0][:, owned], err_msg="actions, specs " + tag)
                np.testing.assert_array_equal(fe[:, owned], want[1][:, owned], err_msg="explored, specs " + tag)
                np.testing.assert_array_equal(bits32c(fq)[:, owned], bits32c(want_q)[:, owned], err_msg="q_out, specs " + tag)
                # slots that no group owns: 255 / 0 / the prefill untouched
                assert (fa[:, ~owned] == 255).all() and not fe[:, ~owned].any() and (bits32(fq)[:, ~owned] == FILL32).all(), tag
                np.testing.assert_array_equal(bare.actions.cpu().numpy(), fa, err_msg="bare " + tag)
                assert (fa[dead] == 255).all()
                seen |= set(np.unique(fa).tolist())
    assert seen == {0, 1, 2, 3, 4, 255}


@pytest.mark.parametrize("E,N", ((100, 3), (64, 8)))
def test_one_group_all_equals_mlp_q_actions(batches, E, N):
    from collectivecrossing_amd import QLearning

    batch = batches(N, E)
    _, _, obs, masks_np = stepped_state(batch, N, E)
    masks = cuda(masks_np)
    ql = QLearning(batch, epsilon=0.3)
    for O in (5, 6):
        sides, _ = sides_with(batch, ("all",), 64, O, seed=6)
        head = sides.groups[0][1]
        for m, greedy in ((masks, False), (None, False), (masks, True)):
            qa, qb = prefilled((E, N, 5)), prefilled((E, N, 5))
            a = ql.sides_q_actions(sides, obs, m, greedy=greedy, want_explored=True, q_out=qa)
            b = ql.mlp_q_actions(head, obs, m, greedy=greedy, want_explored=True, q_out=qb)
            batch.synchronize()
            np.testing.assert_array_equal(a.actions.cpu().numpy(), b.actions.cpu().numpy())
            np.testing.assert_array_equal(a.explored.cpu().numpy(), b.explored.cpu().numpy())
            np.testing.assert_array_equal(bits32(qa.cpu().numpy()), bits32(qb.cpu().numpy()))


def test_the_largest_row(batches):
    """N = 64, L = 262, H = 256 (sixteen waves), O = 6: the LDS opt-in above 64 KB, for both fused kernels."""
    import torch

    from collectivecrossing_amd import QLearning, SideHeads

    E, N = 2, 64
    batch = batches(N, E)
    assert batch.obs_len == 262
    batch.reset_from_pool()
    batch.set_rng_seed(SEED)
    obs = batch.observe()
    ql = QLearning(batch, epsilon=0.5)
    params = linear_init(262, 256, 6, seed=9)
    head = head_with(batch, params, 256, 6, TANH)
    sides = SideHeads(batch, {tuple(range(1, 64, 2)): head})
    st = batch.get_state()
    state = (st["terminated"], st["truncated"], st["step_count"], st["episode"])
    want_q = spec_q(obs.cpu().numpy(), params, TANH, 6)
    want = q_actions_spec(want_q, None, *state, seed=SEED, epsilon=0.5)
    qa, qb = prefilled((E, N, 5)), prefilled((E, N, 5))
    a = ql.mlp_q_actions(head, obs, want_explored=True, q_out=qa)
    b = ql.sides_q_actions(sides, obs, want_explored=True, q_out=qb)
    with torch.no_grad():
        two = ql.q_actions(ql.dueling(head(obs)), want_explored=True)
    batch.synchronize()
    np.testing.assert_array_equal(a.actions.cpu().numpy(), want[0])
    np.testing.assert_array_equal(a.explored.cpu().numpy(), want[1])
    np.testing.assert_array_equal(a.actions.cpu().numpy(), two.actions.cpu().numpy())
    np.testing.assert_array_equal(bits32c(qa.cpu().numpy()), bits32c(want_q))
    odd = np.arange(N) % 2 == 1
    np.testing.assert_array_equal(b.actions.cpu().numpy()[:, odd], want[0][:, odd])
    np.testing.assert_array_equal(b.explored.cpu().numpy()[:, odd], want[1][:, odd])
    np.testing.assert_array_equal(bits32c(qb.cpu().numpy())[:, odd], bits32c(want_q)[:, odd])
    assert (b.actions.cpu().numpy()[:, ~odd] == 255).all() and (bits32(qb.cpu().numpy())[:, ~odd] == FILL32).all()


# ------------------------------------------------------------------------------------------------- 4. a captured actor step
def test_captured_actor_step_with_a_changing_rate_equals_eager_steps():
    import torch

    from collectivecrossing_amd import QLearning, SideHeads
    from collectivecrossing_amd.batched import BatchedCollectiveCrossing
    from collectivecrossing_amd.qlearn import QActions

    E, N = 64, 8
    rates = (1.0, 0.0, 0.3)
    env = BatchedCollectiveCrossing(make_config(N, max_steps=12), E)
    env.make_reset_pool(seed0=5, size=256)
    env.reset_from_pool()
    env.set_rng_seed(SEED)
    start = env.get_state()
    side = torch.cuda.Stream()
    env.use_stream(side)
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        ql = QLearning(env)
        torch.manual_seed(2)
        online = SideHeads(env, {s: env.mlp_head(16, O=6) for s in ("boarding", "exiting")})
        with torch.no_grad():
            for p in online.parameters():
                p.mul_(3.0)
        obs, masks = env.observe(), env.action_masks()
        actions = torch.empty((1, E, N), dtype=torch.uint8, device="cuda")
        chosen = QActions(actions[0], torch.empty((E, N), dtype=torch.uint8, device="cuda"))
        out = env.alloc_rollout(1)

        def body():
            ql.sides_q_actions(online, obs, masks, out=chosen)
            env.rollout(actions, auto_reset=True, out=out, masks_out=masks, reset_obs="next")
            obs.copy_(out.obs[0])

        def run(step):
            hist = []
            for rate in rates:
                ql.epsilon = rate
                step()
                side.synchronize()
                hist.append((actions[0].cpu().numpy(), chosen.explored.cpu().numpy(), out.reward[0].cpu().numpy()))
            return hist

        eager = run(body)
        live = eager[0][0] != 255
        assert eager[0][1][live].all() and not eager[1][1].any() and 0 < eager[2][1].sum() < live.sum()
        env.set_state(**start)
        env.observe(out=obs)
        env.action_masks(out=masks)
        side.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            body()
        side.synchronize()
        replayed = run(graph.replay)
        for s, (e, r) in enumerate(zip(eager, replayed)):
            for name, x, y in zip(("actions", "explored", "reward"), e, r):
                np.testing.assert_array_equal(x, y, err_msg=f"step {s}: {name}")
    env.use_stream(None)
    env.close()


# ------------------------------------------------------------------------------------------------- 5. refusals
def test_refusals_leave_the_batch_usable(batches):
    import torch

    from collectivecrossing_amd import QLearning, SideHeads, _abi
    from collectivecrossing_amd.qlearn import QActions

    E, N, M = 21, 3, 65
    batch, other = batches(N, E), batches(8, 8)
    batch.reset_from_pool()
    ql = QLearning(batch, epsilon=0.5)
    L = batch.obs_len
    obs = batch.observe()
    head5, head6, head3 = batch.mlp_head(16), batch.mlp_head(16, O=6), batch.mlp_head(16, O=3)
    short, foreign = batch.mlp_head(16, L=L - 1), other.mlp_head(16, L=L)
    mk = torch.full((E, N), 0x1F, dtype=torch.uint8, device="cuda")
    shifted = torch.empty(E * N * L + 1, device="cuda")[1:].view(E, N, L)
    assert shifted.is_contiguous() and shifted.data_ptr() % 16
    good = ql.mlp_q_actions(head6, obs, mk, want_explored=True)
    bad_calls = [dict(head=head3), dict(head=short), dict(head=foreign), dict(head=object()), dict(obs=obs.double()), dict(obs=obs[:-1]),
                 dict(obs=obs.cpu()), dict(obs=shifted), dict(obs=None), dict(masks=mk.int()), dict(masks=mk[:-1]),
                 dict(q_out=torch.empty((E, N, 6), device="cuda")), dict(q_out=torch.empty((E, N, 5), dtype=torch.float64, device="cuda")),
                 dict(out=(1, 2)), dict(out=QActions(torch.empty((E, N + 1), dtype=torch.uint8, device="cuda"), None))]
    for kw in bad_calls:
        args = dict(head=head6, obs=obs, masks=mk)
        args.update(kw)
        with pytest.raises(ValueError):
            ql.mlp_q_actions(**args)
    sides6 = SideHeads(batch, {"boarding": batch.mlp_head(16, O=6), "exiting": batch.mlp_head(16, O=6)})
    sides3 = SideHeads(batch, {"all": head3})
    for kw in (dict(sides=sides3), dict(sides=SideHeads(other, {"all": foreign})), dict(sides=head6), dict(obs=obs.half()), dict(obs=shifted),
               dict(obs=obs[:, :-1]), dict(masks=mk.bool()), dict(out=batch.alloc_sample())):
        args = dict(sides=sides6, obs=obs, masks=mk)
        args.update(kw)
        with pytest.raises(ValueError):
            ql.sides_q_actions(**args)
    va = torch.zeros((M, 6), device="cuda")
    va_shift = torch.empty(M * 6 + 1, device="cuda")[1:].view(M, 6)
    q_shift = torch.empty(M * 5 + 1, device="cuda")[1:].view(M, 5)
    for bad in (va.double(), va[:, :5], va.cpu(), va_shift, None, va.t().contiguous().t()):
        with pytest.raises(ValueError):
            ql.dueling(bad)
    for kw in (dict(out=q_shift), dict(out=torch.empty((M, 6), device="cuda")), dict(out=torch.empty((M - 1, 5), device="cuda"))):
        with pytest.raises(ValueError):
            ql.dueling(va, **kw)
    with pytest.raises(ValueError, match="out="):
        ql.dueling(va.clone().requires_grad_(), out=torch.empty((M, 5), device="cuda"))
    qs = [torch.empty((M, 5), device="cuda") for _ in range(5)]
    for a, b in (((va,) * 5, tuple(qs)), ((), ()), ((va, va), (qs[0],)), ((va, va[:-1]), (qs[0], qs[1])), ((va,), (q_shift,)), (7, 8)):
        with pytest.raises(ValueError):
            ql.dueling_into(a, b)
    for bad, kw in ((q_shift, {}), (qs[0].double(), {}), (va, {}), (qs[0], dict(out=va_shift)), (qs[0], dict(out=qs[1])), (None, {})):
        with pytest.raises(ValueError):
            ql.dueling_backward(bad, **kw)
    # the library's own refusals (the wrapper refuses first, so they are reached through the bindings)
    lib, h = batch._lib, batch._h
    tab = lambda *ts: (C.c_void_p * len(ts))(*(None if t is None else t if isinstance(t, int) else t.data_ptr() for t in ts))  # noqa: E731
    assert lib.ccx_dueling_forward(h, M, 1, tab(va), tab(qs[0])) == _abi.OK
    for args, word in (((None, M, 1, tab(va), tab(qs[0])), "NULL handle"), ((h, 0, 1, tab(va), tab(qs[0])), "rows"),
                       ((h, M, 0, tab(va), tab(qs[0])), "num"), ((h, M, 5, tab(va), tab(qs[0])), "num"), ((h, M, 1, None, tab(qs[0])), "NULL"),
                       ((h, M, 2, tab(va, None), tab(qs[0], qs[1])), "NULL"), ((h, M, 1, tab(va_shift), tab(qs[0])), "aligned"),
                       ((h, M, 2, tab(va, va), tab(qs[0], q_shift)), "aligned"), ((h, 1 << 40, 1, tab(va), tab(qs[0])), "workgroups"),
                       ((h, 64 * 0x7FFFFFFF, 4, tab(va, va, va, va), tab(*qs[:4])), "workgroups")):   # (refused before any launch)
        assert lib.ccx_dueling_forward(*args) == _abi.EINVAL, word
        assert word in lib.ccx_last_error().decode(), (word, lib.ccx_last_error())
    gva = torch.empty((M, 6), device="cuda")
    assert lib.ccx_dueling_backward(h, M, qs[0].data_ptr(), gva.data_ptr()) == _abi.OK
    for args, word in (((None, M, qs[0].data_ptr(), gva.data_ptr()), "NULL handle"), ((h, 0, qs[0].data_ptr(), gva.data_ptr()), "rows"),
                       ((h, M, None, gva.data_ptr()), "NULL"), ((h, M, qs[0].data_ptr(), None), "NULL"),
                       ((h, M, q_shift.data_ptr(), gva.data_ptr()), "aligned"), ((h, M, qs[0].data_ptr(), va_shift.data_ptr()), "aligned")):
        assert lib.ccx_dueling_backward(*args) == _abi.EINVAL, word
        assert word in lib.ccx_last_error().decode(), (word, lib.ccx_last_error())
    acts = torch.empty((E, N), dtype=torch.uint8, device="cuda")
    p6 = [t.data_ptr() for t in (head6.w1t, head6.b1, head6.w2, head6.b2)]
    tail = (None, None, acts.data_ptr(), None, None)
    for args, word in (((None, 16, 0, 6, obs.data_ptr(), *p6, *tail), "NULL handle"), ((h, 16, 0, 7, obs.data_ptr(), *p6, *tail), "O = 7"),
                       ((h, 16, 0, 4, obs.data_ptr(), *p6, *tail), "O = 4"), ((h, 16, 0, 6, None, *p6, *tail), "NULL"),
                       ((h, 16, 0, 6, shifted.data_ptr(), *p6, *tail), "aligned"), ((h, 24, 0, 6, obs.data_ptr(), *p6, *tail), "H = 24")):
        assert lib.ccx_mlp_q_actions(*args) == _abi.EINVAL, word
        assert word in lib.ccx_last_error().decode(), (word, lib.ccx_last_error())
    table = sides6._table()
    for args, word in (((None, 16, 0, 6, obs.data_ptr(), 2, table, *tail), "NULL handle"), ((h, 16, 0, 8, obs.data_ptr(), 2, table, *tail), "O = 8"),
                       ((h, 16, 0, 6, obs.data_ptr(), 0, table, *tail), "num_groups"), ((h, 16, 0, 6, shifted.data_ptr(), 2, table, *tail), "aligned")):
        assert lib.ccx_sides_q_actions(*args) == _abi.EINVAL, word
        assert word in lib.ccx_last_error().decode(), (word, lib.ccx_last_error())
    batch.synchronize()
    again = ql.mlp_q_actions(head6, obs, mk, want_explored=True)
    ql.sides_q_actions(sides6, obs, mk)
    ql.mlp_q_actions(head5, obs)
    batch.synchronize()
    assert torch.equal(again.actions, good.actions) and torch.equal(again.explored, good.explored)
    assert not ql.dueling(va).view(torch.int32).any() and not ql.dueling_backward(qs[0].zero_()).view(torch.int32).any()


# ------------------------------------------------------------------------------------------------- 6. end to end
def test_the_examples_loop_twice():
    import torch

    spec = importlib.util.spec_from_file_location("dqn_dueling", ROOT / "examples" / "dqn_dueling.py")
    example = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(example)
    kw = dict(num_envs=64, updates=20, ring_steps=16, batch=256, warmup_steps=8, target_every=5, anneal_updates=10, hidden=16,
              log_every=0)
    first, counts, stats, (leaf, pstate) = example.train(**kw)
    second, counts2, _, (leaf2, pstate2) = example.train(**kw)
    assert counts == counts2 == (20, 0)
    assert sum(tuple(p.shape) == (6, 16) for p in first) == 2            # two heads of six outputs
    assert all(torch.isfinite(p).all() for p in first) and all(np.isfinite(s).all() and s[6] > 0 for s in map(np.array, stats))
    assert example.same_bits(first, second), "two runs from the same seeds must end with the same parameter bits"
    assert torch.equal(leaf, leaf2) and torch.equal(pstate, pstate2), "and with the same leaves"
