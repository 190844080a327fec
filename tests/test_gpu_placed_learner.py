"""The learner-side ops on arrays at their minimum legal placement, inside guard bands (tests/_placed.py).

One test per exported op that takes device arrays.  The inputs come from the op's own spec module, at sizes that take
the piece and tail logic of csrc/ccx_rows.h through every branch (rows M = 1, 3, 65, 127, 192: ``5 M % 4`` = 1, 3, 1, 3, 0
and a tail wave of 1, 3, 1, 63 or 0 live rows).  Each op runs once on ordinary tensors -- the existing tests pin that run
to its spec -- and once with EVERY array moved to the weakest address include/ccx.h allows for that pointer: +16 and
+112 for the 16-byte ones (logit, Q, observation, hidden and compact rows, Adam's tensors), +8 for f64 and i64 arrays,
+4 for the other f32 arrays (``y``, ``logp``, ``entropy``, weights, biases, their gradients, stats), +1 for u8.  Asserted:
bit-equal outputs, 4096 untouched sentinel bytes on either side of every output and input, unchanged input bytes.
Workspaces the Python layer owns stay where it puts them.
"""
import numpy as np
import pytest
from _placed import PlacedCall

pytestmark = pytest.mark.gpu

ROWS = (1, 3, 65, 127, 192)
BATCHES = ((5, 3), (13, 8))             # (E, N)
OFF16 = (16, 112)
K = 3
SEED = 0x0123_4567_89AB_CDEF
A8, A4, A1 = 8, 4, 1                    # the residues of the 8-, 4- and 1-byte pointers (= their alignment)


@pytest.fixture(scope="module")
def batches():
    import torch

    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    from _reset_obs_spec import make_config

    from collectivecrossing_amd.batched import BatchedCollectiveCrossing

    made = {}

    def get(E, N, tag=""):
        if (E, N, tag) not in made:
            b = BatchedCollectiveCrossing(make_config(N, max_steps=12), E)
            b.make_reset_pool(seed0=5, size=64)
            b.reset_from_pool()
            b.set_rng_seed(SEED)
            made[E, N, tag] = b
        return made[E, N, tag]

    yield get
    for b in made.values():
        b.close()


def _dev(a):
    import torch
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


class P(PlacedCall):
    """Shorthands: the residue is the alignment for the 8-, 4- and 1-byte pointers; ``off16`` for the 16-byte ones."""

    def __init__(self, ctx, off16):
        super().__init__(f"{ctx} (16-byte arrays at +{off16})")
        self.off16 = off16

    def i16(self, name, a):
        return self.inp(name, a, self.off16, 16)

    def i8(self, name, a):
        return self.inp(name, a, A8, 8)

    def i4(self, name, a):
        return self.inp(name, a, A4, 4)

    def i1(self, name, a):
        return self.inp(name, a, A1, 1)

    def o16(self, name, shape):
        import torch
        return self.out(name, shape, torch.float32, self.off16, 16)

    def o4(self, name, shape):
        import torch
        return self.out(name, shape, torch.float32, A4, 4)

    def o1(self, name, shape):
        import torch
        return self.out(name, shape, torch.uint8, A1, 1)

    def o8(self, name, shape, dtype):
        return self.out(name, shape, dtype, A8, 8)

    def ws(self, name, nbytes):
        """A caller-owned workspace at +8 (at least 8 bytes, as the Python layer allocates them)."""
        return self.scratch(name, max(8, int(nbytes)), A8, 8)


def _set_slots(batch, case):
    batch.set_state(terminated=case["terminated"], truncated=case["truncated"], step_count=case["step_count"],
                    episode=case["episode"])


# ------------------------------------------------------------------------------------------------ trajectory ops
@pytest.mark.parametrize("E,N", BATCHES)
def test_compute_gae(batches, E, N):
    from _gae_spec import make_gae_case

    from collectivecrossing_amd.learner import GaeResult
    b = batches(E, N)
    c = make_gae_case(K, E, N, seed=3)
    want = b.compute_gae((_dev(c["reward"]), _dev(c["agent_flags"]), _dev(c["env_flags"])), _dev(c["values"]),
                         _dev(c["last_values"]), _dev(c["final_values"]))
    p = P(f"compute_gae K={K} E={E} N={N}", 16)
    out = GaeResult(p.o4("advantages", (K, E, N)), p.o4("returns", (K, E, N)), p.o1("valid", (K, E, N)))
    b.compute_gae((p.i8("reward", c["reward"]), p.i1("agent_flags", c["agent_flags"]), p.i1("env_flags", c["env_flags"])),
                  p.i4("values", c["values"]), p.i4("last_values", c["last_values"]), p.i4("final_values", c["final_values"]),
                  out=out)
    p.check(dict(advantages=want.advantages, returns=want.returns, valid=want.valid))


@pytest.mark.parametrize("E,N", BATCHES)
def test_update_episode_stats(batches, E, N):
    from _episode_stats_spec import make_trajectory
    reward, af, ef = make_trajectory(K, E, N, seed=4)
    A, B = batches(E, N, "stats_a"), batches(E, N, "stats_b")
    for b in (A, B):
        b.track_episodes(log_capacity=64)
    A.update_episode_stats(_dev(reward), _dev(af), _dev(ef))
    p = P(f"update_episode_stats K={K} E={E} N={N}", 16)
    B.update_episode_stats(p.i8("reward", reward), p.i1("agent_flags", af), p.i1("env_flags", ef))
    p.check({})
    sa, sb = A.episode_stats(), B.episode_stats()
    for f in ("ret", "live_steps", "steps", "closed", "finished", "last_ret", "last_live_steps", "last_steps", "last_end", "log_count"):
        ga, gb = getattr(sa, f).cpu().numpy(), getattr(sb, f).cpu().numpy()
        assert np.array_equal(ga.reshape(-1).view(np.uint8), gb.reshape(-1).view(np.uint8)), (p.ctx, f)
    ra, rb = A.finished_episodes(), B.finished_episodes()
    assert len(ra) == len(rb) > 0
    for f in ("env", "episode", "steps", "end", "ret", "live_steps"):
        assert np.array_equal(getattr(ra, f).reshape(-1).view(np.uint8), getattr(rb, f).reshape(-1).view(np.uint8)), (p.ctx, f)


# ------------------------------------------------------------------------------------------------ [E, N] ops
@pytest.mark.parametrize("off16", OFF16)
@pytest.mark.parametrize("E,N", BATCHES)
def test_sample_actions(batches, E, N, off16):
    from _sample_spec import make_sample_case

    from collectivecrossing_amd.learner import SampleResult
    b = batches(E, N)
    c = make_sample_case(E, N, seed=5)
    _set_slots(b, c)
    for det in (False, True):
        want = b.sample_actions(_dev(c["logits_masked"]), _dev(c["masks"]), deterministic=det, want_entropy=True)
        p = P(f"sample_actions E={E} N={N} deterministic={det}", off16)
        out = SampleResult(p.o1("actions", (E, N)), p.o4("logp", (E, N)), p.o4("entropy", (E, N)))
        b.sample_actions(p.i16("logits", c["logits_masked"]), p.i1("masks", c["masks"]), deterministic=det, out=out)
        p.check(dict(actions=want.actions, logp=want.logp, entropy=want.entropy))


@pytest.mark.parametrize("off16", OFF16)
@pytest.mark.parametrize("E,N", BATCHES)
def test_q_actions(batches, E, N, off16):
    from _qlearn_spec import make_q_case

    from collectivecrossing_amd.qlearn import QActions, QLearning
    b = batches(E, N)
    c = make_q_case(E, N, seed=6)
    _set_slots(b, c)
    ql = QLearning(b, epsilon=0.4)
    for greedy in (False, True):
        want = ql.q_actions(_dev(c["q_masked"]), _dev(c["masks"]), greedy=greedy, want_explored=True)
        p = P(f"q_actions E={E} N={N} greedy={greedy}", off16)
        out = QActions(p.o1("actions", (E, N)), p.o1("explored", (E, N)))
        ql.q_actions(p.i16("q", c["q_masked"]), p.i1("masks", c["masks"]), greedy=greedy, out=out)
        p.check(dict(actions=want.actions, explored=want.explored))


# ------------------------------------------------------------------------------------------------ row ops
@pytest.mark.parametrize("off16", OFF16)
@pytest.mark.parametrize("M", ROWS)
def test_evaluate_actions_and_backward(batches, M, off16):
    from _evaluate_spec import case_args, make_evaluate_case

    from collectivecrossing_amd.learner import EvalResult
    b = batches(*BATCHES[0])
    logits, actions, masks, glp, gent = case_args(make_evaluate_case(M, 1, seed=7), masked=True)
    want = b.evaluate_actions(_dev(logits), _dev(actions), _dev(masks))
    want_g = b.evaluate_actions_backward(_dev(logits), _dev(actions), _dev(masks), _dev(glp), _dev(gent))
    p = P(f"evaluate_actions M={M}", off16)
    li, ai, mi = p.i16("logits", logits), p.i1("actions", actions), p.i1("masks", masks)
    b.evaluate_actions(li, ai, mi, out=EvalResult(p.o4("logp", (M,)), p.o4("entropy", (M,))))
    b.evaluate_actions_backward(li, ai, mi, p.i4("grad_logp", glp), p.i4("grad_entropy", gent), out=p.o16("grad_logits", (M, 5)))
    p.check(dict(logp=want.logp, entropy=want.entropy, grad_logits=want_g))


@pytest.mark.parametrize("off16", OFF16)
@pytest.mark.parametrize("M", ROWS)
def test_masked_moments_ppo_loss_and_backward(batches, M, off16):
    import torch
    from _ppo_loss_spec import case_args, make_ppo_case

    from collectivecrossing_amd.learner import PpoLossResult
    b = batches(*BATCHES[0])
    kw = case_args(make_ppo_case(M, seed=8), masked=True)
    t = {k: _dev(v) for k, v in kw.items()}
    norm = b.masked_moments(t["advantages"], t["valid"])
    want = b.ppo_loss(**t, norm=norm)
    gl_loss = torch.tensor([0.75], dtype=torch.float32, device="cuda")
    want_gl, want_gv = b.ppo_loss_backward(**t, norm=norm, stats=want.stats, grad_loss=gl_loss)
    p = P(f"masked_moments / ppo_loss M={M}", off16)
    pt = dict(logits=p.i16("logits", kw["logits"]), values=p.i4("values", kw["values"]), actions=p.i1("actions", kw["actions"]),
              logp_old=p.i4("logp_old", kw["logp_old"]), advantages=p.i4("advantages", kw["advantages"]),
              returns=p.i4("returns", kw["returns"]), masks=p.i1("masks", kw["masks"]), valid=p.i1("valid", kw["valid"]))
    need = int(b._lib.ccx_ppo_workspace_bytes(M))
    pnorm = b.masked_moments(pt["advantages"], pt["valid"], out=p.o4("norm", (4,)), workspace=p.ws("moments workspace", need))
    stats = p.o4("stats", (8,))
    b.ppo_loss(**pt, norm=pnorm, out=PpoLossResult(stats[0], stats, p.ws("loss workspace", need)))
    # the backward reads the forward's stats where the forward left them, and writes both gradients
    b.ppo_loss_backward(**pt, norm=pnorm, stats=stats, grad_loss=p.i4("grad_loss", gl_loss),
                        out=PpoLossResult(stats[0], stats, None, p.o16("grad_logits", (M, 5)), p.o4("grad_values", (M,))))
    p.check(dict(norm=norm, stats=want.stats, grad_logits=want_gl, grad_values=want_gv))


@pytest.mark.parametrize("off16", OFF16)
@pytest.mark.parametrize("M", ROWS)
def test_td_loss_and_backward(batches, M, off16):
    import torch
    from _qlearn_spec import make_td_case, td_args

    from collectivecrossing_amd.qlearn import QLearning, TdLossResult
    ql = QLearning(batches(*BATCHES[0]))
    kw = td_args(make_td_case(M, seed=9))
    t = {k: _dev(v) for k, v in kw.items()}
    want = ql.td_loss(**t, want_td_error=True)
    gl_loss = torch.tensor([1.5], dtype=torch.float32, device="cuda")
    want_g = ql.td_loss_backward(**t, stats=want.stats, grad_loss=gl_loss)
    p = P(f"td_loss M={M}", off16)
    pt = dict(q=p.i16("q", kw["q"]), actions=p.i1("actions", kw["actions"]), reward=p.i8("reward", kw["reward"]),
              done=p.i1("done", kw["done"]), q_next_target=p.i16("q_next_target", kw["q_next_target"]),
              q_next_online=p.i16("q_next_online", kw["q_next_online"]), masks_next=p.i1("masks_next", kw["masks_next"]),
              valid=p.i1("valid", kw["valid"]), weights=p.i4("weights", kw["weights"]))
    stats = p.o4("stats", (8,))
    ql.td_loss(**pt, out=TdLossResult(stats[0], stats, p.o4("td_error", (M,)), p.ws("workspace", ql.batch._lib.ccx_td_workspace_bytes(M))))
    ql.td_loss_backward(**pt, stats=stats, grad_loss=p.i4("grad_loss", gl_loss), out=p.o16("grad_q", (M, 5)))
    p.check(dict(stats=want.stats, td_error=want.td_error, grad_q=want_g))


# ------------------------------------------------------------------------------------------------ policy heads
PARAMS = ("w1t", "b1", "w2", "b2")
HEADS = [(16, 3), (64, 3), (16, 8), (64, 8)]            # (H, N): L = 18 (odd row length in 16-byte units) and L = 38


def _head(batch, H, O, L, case, p=None, tag=""):
    """An MlpHead holding ``case``'s parameters; with ``p`` every parameter sits at +4 inside guard bands (inputs of ``p``)."""
    import torch
    head = batch.mlp_head(H, O, "tanh", L=L)
    with torch.no_grad():
        for name in PARAMS:
            if p is None:
                getattr(head, name).copy_(torch.from_numpy(case[name]))
            else:
                getattr(head, name).data = p.i4(f"{tag}{name}", case[name])
    return head


@pytest.mark.parametrize("off16", OFF16)
@pytest.mark.parametrize("H,N", HEADS)
def test_mlp_forward_and_backward(batches, H, N, off16):
    from _mlp_backward_spec import make_mlp_backward_case

    import torch

    from collectivecrossing_amd.learner import MlpGradResult
    b = batches(*BATCHES[0])
    L, O = 6 + 4 * N, 5
    for M in ROWS:
        c = make_mlp_backward_case(M, L, H, O, seed=10 + M)
        head = _head(b, H, O, L, c)
        with torch.no_grad():
            want_hidden = torch.empty((M, H), dtype=torch.float32, device="cuda")
            want_y = head(_dev(c["x"]), hidden_out=want_hidden)
            want = b.mlp_backward(head, _dev(c["x"]), _dev(c["hidden"]), _dev(c["grad_y"]), want_grad_a=True)
        p = P(f"MlpHead L={L} H={H} O={O} M={M}", off16)
        phead = _head(b, H, O, L, c, p)
        with torch.no_grad():
            x = p.i16("x", c["x"])
            assert phead(x, out=p.o4("y", (M, O)), hidden_out=p.o16("hidden_out", (M, H))) is p.outs["y"][0]
            out = MlpGradResult(p.o4("grad_w1t", (L, H)), p.o4("grad_b1", (H,)), p.o4("grad_w2", (O, H)), p.o4("grad_b2", (O,)),
                                p.o16("grad_a", (M, H)), p.ws("workspace", b._lib.ccx_mlp_backward_workspace_bytes(M, L, H, O)))
            b.mlp_backward(phead, x, p.i16("hidden", c["hidden"]), p.i4("grad_y", c["grad_y"]), out=out)
        p.check(dict(y=want_y, hidden_out=want_hidden, grad_w1t=want.w1t, grad_b1=want.b1, grad_w2=want.w2, grad_b2=want.b2,
                     grad_a=want.grad_a))


@pytest.mark.parametrize("off16", OFF16)
@pytest.mark.parametrize("H", [16, 64])
@pytest.mark.parametrize("E,N", BATCHES)
def test_mlp_sample_actions(batches, E, N, H, off16):
    import torch
    from _mlp_spec import make_mlp_case
    from _sample_spec import make_sample_case

    from collectivecrossing_amd.learner import SampleResult
    b = batches(E, N)
    L = b.obs_len
    c = make_mlp_case(E * N, L, H, 5, seed=11, adversarial=False)
    s = make_sample_case(E, N, seed=12)
    _set_slots(b, s)
    obs = c["x"].reshape(E, N, L)
    head = _head(b, H, 5, L, c)
    with torch.no_grad():
        want_logits = torch.empty((E, N, 5), dtype=torch.float32, device="cuda")
        want = b.mlp_sample_actions(head, _dev(obs), _dev(s["masks"]), want_entropy=True, logits_out=want_logits)
        p = P(f"mlp_sample_actions E={E} N={N} H={H}", off16)
        phead = _head(b, H, 5, L, c, p)
        out = SampleResult(p.o1("actions", (E, N)), p.o4("logp", (E, N)), p.o4("entropy", (E, N)))
        b.mlp_sample_actions(phead, p.i16("obs", obs), p.i1("masks", s["masks"]), logits_out=p.o4("logits_out", (E, N, 5)), out=out)
    p.check(dict(actions=want.actions, logp=want.logp, entropy=want.entropy, logits_out=want_logits))


@pytest.mark.parametrize("off16", OFF16)
@pytest.mark.parametrize("H", [16, 64])
@pytest.mark.parametrize("E,N", BATCHES)
def test_side_heads_forward_sample_and_backward(batches, E, N, H, off16):
    import torch
    from _mlp_backward_spec import make_mlp_backward_case
    from _mlp_spec import make_mlp_case
    from _sample_spec import make_sample_case

    from collectivecrossing_amd import SideHeads
    from collectivecrossing_amd.learner import MlpGradResult, SampleResult
    b = batches(E, N)
    L, O = b.obs_len, 5
    cases = [make_mlp_case(1, L, H, O, seed=13 + 31 * i) for i in range(2)]
    rows = make_mlp_backward_case(E * N, L, H, O, seed=14)
    x, grad_y = rows["x"].reshape(E, N, L), rows["grad_y"].reshape(E, N, O)
    s = make_sample_case(E, N, seed=15)
    _set_slots(b, s)
    with torch.no_grad():
        sides = SideHeads(b, {"boarding": _head(b, H, O, L, cases[0]), "exiting": _head(b, H, O, L, cases[1])})
        want_hidden = torch.empty((E, N, H), dtype=torch.float32, device="cuda")
        want_y = sides(_dev(x), hidden_out=want_hidden)
        want_logits = torch.empty((E, N, 5), dtype=torch.float32, device="cuda")
        want_s = sides.sample_actions(_dev(x), _dev(s["masks"]), want_entropy=True, logits_out=want_logits)
        want_g = sides.backward_into(_dev(x), want_hidden, _dev(grad_y), want_grad_a=True)
        p = P(f"SideHeads E={E} N={N} H={H}", off16)
        psides = SideHeads(b, {"boarding": _head(b, H, O, L, cases[0], p, "boarding."), "exiting": _head(b, H, O, L, cases[1], p, "exiting.")})
        px = p.i16("x", x)
        psides(px, out=p.o4("y", (E, N, O)), hidden_out=p.o16("hidden_out", (E, N, H)))
        psides.sample_actions(px, p.i1("masks", s["masks"]), logits_out=p.o4("logits_out", (E, N, 5)),
                              out=SampleResult(p.o1("actions", (E, N)), p.o4("logp", (E, N)), p.o4("entropy", (E, N))))
        grad_a = p.o16("grad_a", (E, N, H))
        outs = [MlpGradResult(p.o4(f"{g}.grad_w1t", (L, H)), p.o4(f"{g}.grad_b1", (H,)), p.o4(f"{g}.grad_w2", (O, H)),
                              p.o4(f"{g}.grad_b2", (O,)), grad_a,
                              p.ws(f"{g}.workspace", b._lib.ccx_mlp_backward_workspace_bytes(E * bin(mask).count("1"), L, H, O)))
                for g, mask in zip(("boarding", "exiting"), psides.masks)]
        psides.backward_into(px, p.i16("hidden", want_hidden), p.i4("grad_y", grad_y), out=outs)
    expected = dict(y=want_y, hidden_out=want_hidden, logits_out=want_logits, actions=want_s.actions, logp=want_s.logp,
                    entropy=want_s.entropy, grad_a=want_g[0].grad_a)
    for g, w in zip(("boarding", "exiting"), want_g):
        expected.update({f"{g}.grad_w1t": w.w1t, f"{g}.grad_b1": w.b1, f"{g}.grad_w2": w.w2, f"{g}.grad_b2": w.b2})
    assert want_g[0].grad_a is want_g[1].grad_a
    p.check(expected)


# ------------------------------------------------------------------------------------------------ the optimiser
@pytest.mark.parametrize("off16", OFF16)
def test_device_adam_step(batches, off16):
    import torch
    from _adam_spec import make_adam_case
    b = batches(*BATCHES[0])
    numels = (1, 17, 4100)
    params, grad_steps = make_adam_case(numels, seed=16, steps=3)
    hyper = dict(lr=1e-2, weight_decay=0.01, max_grad_norm=0.5)
    A = b.adam([_dev(x) for x in params], **hyper)
    p = P(f"DeviceAdam.step numels={numels}", off16)
    # params, m and v are updated in place: outputs that start from the same bytes as the ordinary run's
    pp = []
    for i, x in enumerate(params):
        v = p.o16(f"param[{i}]", x.shape)
        v.copy_(_dev(x))
        pp.append(v)
    B = b.adam(pp, **hyper)
    for i in range(len(numels)):
        B.m[i] = p.o16(f"m[{i}]", params[i].shape).zero_()
        B.v[i] = p.o16(f"v[{i}]", params[i].shape).zero_()
    start = B.state.clone()
    B.state = p.o8("state", (64,), torch.uint8)
    B.state.copy_(start)
    B.stats = p.o4("stats", (4,)).zero_()
    B.workspace = p.ws("workspace", B.workspace.numel())
    for s, grads in enumerate(grad_steps):
        A.step(grads=[_dev(g) for g in grads])
        B.step(grads=[p.inp(f"grad[{i}] of step {s}", g, off16, 16) for i, g in enumerate(grads)])
    assert A.counts() == B.counts() == (3, 0)
    expected = dict(state=A.state, stats=A.stats)
    for i in range(len(numels)):
        expected.update({f"param[{i}]": A.params[i], f"m[{i}]": A.m[i], f"v[{i}]": A.v[i]})
    p.check(expected)


# ------------------------------------------------------------------------------------------------ the replay ring
@pytest.mark.parametrize("off16", OFF16)
@pytest.mark.parametrize("E,N", BATCHES)
def test_replay_ring_push_sample_and_fetch(batches, E, N, off16):
    import torch

    from collectivecrossing_amd.replay import ReplayBatch, ReplayRing
    b = batches(E, N, "replay")
    L, S, B_ = b.obs_len, 4, 65                        # (65 records: a full wave and one row of the next)
    rng = np.random.default_rng(17)
    b.set_state(episode=np.zeros(E, np.int32))
    b.reset_from_pool()
    b.set_state(step_count=(11 - np.arange(E) % 3).astype(np.int32))    # (max_steps = 12: restarts inside the three steps)
    first = b.rollout(rng.integers(0, 5, size=(1, E, N), dtype=np.uint8), auto_reset=True, want_compact=True, reset_obs="next")
    obs0_c = first.obs_compact[0].clone()
    acts = rng.integers(0, 5, size=(K, E, N), dtype=np.uint8)
    traj = b.alloc_rollout(K, True, True, want_final=True)
    b.rollout(acts, auto_reset=True, out=traj, reset_obs="next")
    assert bool((traj.env_flags & 0x04).any())
    masks_next = rng.integers(0, 256, size=(K, E, N), dtype=np.uint8)
    ring_a, ring_b = ReplayRing(b, steps=S), ReplayRing(b, steps=S)
    ring_a.push(obs0_c, _dev(acts), (traj.reward, traj.agent_flags, traj.env_flags, traj.obs_compact, traj.final_compact),
                _dev(masks_next))
    p = P(f"ReplayRing E={E} N={N}", off16)
    ring_b.push(p.i16("obs0_compact", obs0_c), p.i1("actions", acts),
                (p.i8("reward", traj.reward), p.i1("agent_flags", traj.agent_flags), p.i1("env_flags", traj.env_flags),
                 p.inp("obs_compact", traj.obs_compact, 128 - off16, 16), p.i16("final_compact", traj.final_compact)),
                p.i1("masks_next", masks_next))
    torch.cuda.synchronize()
    for f in ("obs_c", "next_c", "actions", "reward", "done", "valid", "masks_next", "state"):
        assert torch.equal(getattr(ring_a, f).view(torch.uint8), getattr(ring_b, f).view(torch.uint8)), (p.ctx, "ring", f)

    def placed_batch(tag):
        return ReplayBatch(p.o16(f"{tag}.obs", (B_, N, L)), p.out(f"{tag}.next_obs", (B_, N, L), torch.float32, 128 - off16, 16),
                           p.o1(f"{tag}.actions", (B_, N)), p.o8(f"{tag}.reward", (B_, N), torch.float64), p.o1(f"{tag}.done", (B_, N)),
                           p.o1(f"{tag}.valid", (B_, N)), p.o1(f"{tag}.masks_next", (B_, N)), p.o8(f"{tag}.index", (B_,), torch.int64))

    want_s = ring_a.sample(B_)
    ring_b.sample(B_, out=placed_batch("sample"))
    index = torch.from_numpy(rng.integers(-2, ring_a.records + 2, size=B_)).cuda()
    want_f = ring_a.fetch(index)
    ring_b.fetch(p.i8("index", index), out=placed_batch("fetch"))
    expected = {}
    for tag, w in (("sample", want_s), ("fetch", want_f)):
        expected.update({f"{tag}.{f}": getattr(w, f) for f in ("obs", "next_obs", "actions", "reward", "done", "valid", "masks_next", "index")})
    p.check(expected)
    assert torch.equal(ring_a.state, ring_b.state)
    b.rollout(acts, auto_reset=True, reset_obs="terminal")      # (leaves the shared batch in its default mode)
