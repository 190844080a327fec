"""Whole rounds of a categorical double-DQN at A = 51 with ``CategoricalQ.head`` -- ONE wide device head of 255 outputs -- as
the online and the target network, on a live 16 x 8 batch, against the per-op specs composed on the CPU, bit for bit:
``head(obs)`` -> ``q_values`` -> ``q_actions`` under the step's masks -> the step -> ``loss`` on that step's transitions with
``next_online`` / ``next_target`` from the two heads -> ``loss_backward`` -> ``param_grads`` -> one ``DeviceAdam`` over the four
tensors -> a target copy after round 2.  Three rounds, eager with static buffers and through ``loss.backward()`` with
``backward="device"``.  No replay ring: tests/test_gpu_c51_chain.py covers that wiring (with five narrow heads of 8 atoms,
which this head replaces).  The envs' step counters start near the truncation, so every round restarts some envs."""

import numpy as np
import pytest
from _adam_spec import adam_step_spec, new_state, state_bytes
from _c51_spec import c51_loss_backward_spec, c51_loss_spec, q_values_spec
from _learner_chain import AF_LIVE, AF_TERMINATED, EF_RESET, POOL_SEED0, POOL_SIZE, SEED, _copy, _masks, _oracle_batch, chain_config
from _mlp_backward_spec import NAMES, mlp_backward_spec
from _mlp_spec import TANH, bits32c, linear_init, mlp_spec
from _qlearn_spec import q_actions_spec

pytestmark = pytest.mark.gpu

F32 = np.float32
E, N, A, H, ROUNDS = 16, 8, 51, 16, 3
O, L = 5 * A, 6 + 4 * N
EPS = (0.9, 0.5, 0.1)
GAMMA, LR, MAX_GRAD_NORM = 0.99, 1e-3, 0.5
COPY_AFTER = 2                                     # rounds before the target copy
START_STEP_COUNT = 9 + np.arange(E, dtype=np.int32) % 4          # max_steps = 12: truncations in every round
MASKS_ALL = 0x1F
# three steps end no agent's episode one by one, so every fifth (env, agent) is taken out of the loss by hand: rows that do
# not count, +0.0 in their gradient rows
KEEP = ((np.arange(E)[:, None] + np.arange(N)[None, :]) % 5 != 0).astype(np.uint8)
LINKS = ("actions", "explored", "logits", "reward", "done", "valid", "masks_next", "next_target", "next_online", "stats", "row_loss",
         "proj", "grad_logits") + tuple(f"grad.{n}" for n in NAMES) + ("adam_stats",) + tuple(f"param.{n}" for n in NAMES)


def _forward(x, p):
    y, h = mlp_spec(x.reshape(-1, L), *p, TANH)
    return y.reshape(x.shape[:-1] + (5, A)), h.reshape(x.shape[:-1] + (H,))


@pytest.fixture(scope="module")
def reference():
    """The three rounds on the CPU: per round a dict of every array of LINKS; the final m, v and the optimiser's state bytes."""
    oracle, params_c, ob = _oracle_batch(chain_config(), E)
    ob.set_state(step_count=START_STEP_COUNT)
    online = _copy(linear_init(L, H, O, seed=21))
    target = _copy(online)
    ms, vs, state = [np.zeros_like(p) for p in online], [np.zeros_like(p) for p in online], new_state()
    rounds, resets = [], 0
    for u in range(ROUNDS):
        rows, masks = ob.observe(), _masks(oracle, params_c, ob)
        logits, hidden = _forward(rows, online)
        acts, explored = q_actions_spec(q_values_spec(logits), masks, ob.terminated, ob.truncated, ob.step_count.copy(), ob.episode.copy(),
                                        seed=SEED, epsilon=F32(EPS[u]))
        step_obs, reward, af, ef = ob.rollout(acts[None], auto_reset=True)
        reset = (ef[0] & EF_RESET) != 0
        resets += int(reset.sum())
        masks_next = np.where(reset[:, None], np.uint8(MASKS_ALL), _masks(oracle, params_c, ob)).astype(np.uint8)
        done, valid = (af[0] & AF_TERMINATED).astype(np.uint8), ((af[0] & AF_LIVE) * KEEP).astype(np.uint8)
        nt, _ = _forward(step_obs[0], target)
        no, _ = _forward(step_obs[0], online)
        stats, row_loss, proj = c51_loss_spec(logits, acts, reward[0], done, nt, next_online=no, masks_next=masks_next, valid=valid, gamma=GAMMA)
        gl = c51_loss_backward_spec(logits, acts, proj, valid, None, stats).reshape(E, N, 5, A)
        g = mlp_backward_spec(rows.reshape(-1, L), hidden.reshape(-1, H), gl.reshape(-1, O), online[2], TANH)
        grads = [g[n] for n in NAMES]
        adam_stats = adam_step_spec(online, grads, ms, vs, state, LR, max_grad_norm=MAX_GRAD_NORM)
        rnd = dict(actions=acts, explored=explored, logits=logits, reward=reward[0], done=done, valid=valid, masks_next=masks_next,
                   next_target=nt, next_online=no, stats=stats, row_loss=row_loss.reshape(E, N), proj=proj.reshape(E, N, A), grad_logits=gl,
                   adam_stats=adam_stats)
        rnd.update({f"grad.{n}": a for n, a in zip(NAMES, grads)})
        rnd.update({f"param.{n}": a.copy() for n, a in zip(NAMES, online)})
        assert set(rnd) == set(LINKS)
        rounds.append(rnd)
        if u + 1 == COPY_AFTER:
            target = _copy(online)
    # what the run exercised
    assert 0 < resets < ROUNDS * E and all(r["valid"].any() and not r["valid"].all() for r in rounds) and any(r["explored"].any() for r in rounds)
    assert all(r["stats"][6] > 0 and np.isfinite(r["stats"]).all() for r in rounds) and any((r["explored"] == 0).any() for r in rounds)
    assert all(not bits32c(r["grad_logits"])[r["valid"] == 0].any() and r["grad_logits"].any() for r in rounds)
    assert bits32c(rounds[2]["next_target"]).tobytes() == bits32c(rounds[2]["next_online"]).tobytes()        # behind the copy
    assert bits32c(rounds[1]["next_target"]).tobytes() != bits32c(rounds[1]["next_online"]).tobytes()
    return dict(rounds=rounds, m=ms, v=vs, state_bytes=state_bytes(state))


def _same(got, want, what):
    got = got.detach().cpu().numpy() if hasattr(got, "detach") else np.asarray(got)
    want = np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    if got.dtype == np.float32:
        got, want = bits32c(got), bits32c(want)
    np.testing.assert_array_equal(got, want, err_msg=what)


@pytest.mark.parametrize("autograd", (False, True), ids=("eager", "autograd"))
def test_three_rounds_equal_the_composed_specs(reference, autograd):
    import torch

    from collectivecrossing_amd import CategoricalQ, QLearning
    from collectivecrossing_amd.batched import BatchedCollectiveCrossing
    from collectivecrossing_amd.qlearn import QActions

    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    env = BatchedCollectiveCrossing(chain_config(), E)
    try:
        env.make_reset_pool(seed0=POOL_SEED0, size=POOL_SIZE)
        env.reset_from_pool()
        env.synchronize()
        env.set_state(step_count=START_STEP_COUNT)
        env.set_rng_seed(SEED)
        dev, u8 = env.device, torch.uint8
        cq = CategoricalQ(env, atoms=A)
        online, target = cq.head(H, backward="device"), cq.head(H)
        with torch.no_grad():
            for t, a in zip(online.parameters(), linear_init(L, H, O, seed=21)):
                t.copy_(torch.from_numpy(a))
        target.load_state_dict(online.state_dict())
        ql = QLearning(env, epsilon=EPS[0])
        opt = env.adam(online.parameters(), lr=LR, max_grad_norm=MAX_GRAD_NORM)
        traj = env.alloc_rollout(1)
        acts = torch.empty((1, E, N), dtype=u8, device=dev)
        chosen = QActions(acts[0], torch.empty((E, N), dtype=u8, device=dev))
        obs, masks = env.observe(), env.action_masks()
        logits, nt, no = (torch.empty((E, N, 5, A), device=dev) for _ in range(3))
        hidden, q = torch.empty((E, N, H), device=dev), torch.empty((E, N, 5), device=dev)
        loss = cq.alloc_loss((E, N), want_row_loss=True)
        grads = online.alloc_param_grads((E, N))
        keep = torch.from_numpy(KEEP).to(dev)
        for u, want in enumerate(reference["rounds"]):
            ql.epsilon = EPS[u]
            with torch.no_grad():
                env.observe(out=obs)
                env.action_masks(out=masks)
                online(obs, out=logits, hidden_out=hidden)
                cq.q_values(logits, out=q)
                ql.q_actions(q, masks, out=chosen)
                env.rollout(acts, auto_reset=True, out=traj)
                env.action_masks(out=masks)
                reset = (traj.env_flags[0] & EF_RESET) != 0
                masks_next = torch.where(reset[:, None], torch.full_like(masks, MASKS_ALL), masks)
                done, valid = traj.agent_flags[0] & AF_TERMINATED, (traj.agent_flags[0] & AF_LIVE) * keep
                target(traj.obs[0], out=nt)
                online(traj.obs[0], out=no)
            args = (acts[0], traj.reward[0], done, nt)
            kw = dict(next_online=no, masks_next=masks_next, valid=valid, gamma=GAMMA)
            if autograd:
                opt.zero_grad(set_to_none=True)
                y = online(obs)                                           # the same kernel under grad: the same bits
                y.retain_grad()
                r = cq.loss(y, *args, **kw, want_row_loss=True)
                r.loss.backward()                                         # ccx_c51_loss_backward, then ccx_mlp_wide_backward
                seen = dict(logits=y.detach(), stats=r.stats, row_loss=r.row_loss, proj=r.proj, grad_logits=y.grad,
                            **{f"grad.{n}": p.grad for n, p in zip(NAMES, online.parameters())})
                opt.step()
            else:
                cq.loss(logits, *args, **kw, out=loss)
                cq.loss_backward(logits, acts[0], loss.proj, valid, stats=loss.stats, out=loss)
                online.param_grads(obs, hidden, loss.grad_logits, out=grads)                      # [E, N, 5, A], as it is
                seen = dict(logits=logits, stats=loss.stats, row_loss=loss.row_loss, proj=loss.proj, grad_logits=loss.grad_logits,
                            **{f"grad.{n}": getattr(grads, n) for n in NAMES})
                opt.step(grads=[grads.w1t, grads.b1, grads.w2, grads.b2])
            if u + 1 == COPY_AFTER:
                target.load_state_dict(online.state_dict())
            env.synchronize()
            got = dict(seen, actions=acts[0], explored=chosen.explored, reward=traj.reward[0], done=done, valid=valid, masks_next=masks_next,
                       next_target=nt, next_online=no, adam_stats=opt.stats, **{f"param.{n}": p for n, p in zip(NAMES, online.parameters())})
            for k in LINKS:                                               # in chain order: the first link that differs is named
                _same(got[k], want[k], f"round {u}: {k}")
        for k, mine in (("m", opt.m), ("v", opt.v)):
            for n, a, b in zip(NAMES, mine, reference[k]):
                _same(a, b, f"{k}.{n} after the last round")
        _same(opt.state, reference["state_bytes"], "the optimiser's 64 state bytes")
    finally:
        env.close()
