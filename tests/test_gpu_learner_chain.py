"""Whole PPO and DQN iterations on the device against the composed CPU references of tests/_learner_chain.py, bit for bit:
the claim of examples/ppo_device_update.py and examples/dqn_replay_ring.py -- every link from the observation rows to the
NEW PARAMETERS is a written rule -- checked as a whole.  What the per-op tests cannot see is compared here: parameters fed
back from the optimiser into the next forward and the next actor step, Adam's device state over eight steps with a rate
change between graph replays, the draw key with a real network across auto-resets, GAE on the critic's own values of a
``reset_obs="next"`` trajectory, the order of the gradient list, the ring cursor under alternating graphs, the per-round
epsilon, the per-side select of ``grad_q`` and the target copy.

Each test builds its run from library calls only, as the two examples do, on a batch of its own; the heads are made under
``torch.manual_seed(TORCH_SEED)``, their initial parameters are read back and the reference runs from those (once per
module).  Comparisons go in chain order, so a failure names the first link that differs."""

import numpy as np
import pytest
from _learner_chain import (DQN, DQN_START_STEP_COUNT, EF_RESET, GRAD_ORDER, H, N, POOL_SEED0, POOL_SIZE, PPO, SEED, SIDES,
                            START_STEP_COUNT, TORCH_SEED, assert_dqn_coverage, assert_ppo_coverage, chain_config, dqn_epsilon,
                            dqn_reference, ppo_lr, ppo_reference)

pytestmark = pytest.mark.gpu

ADAM_KW = dict(weight_decay=PPO["WEIGHT_DECAY"], max_grad_norm=PPO["MAX_GRAD_NORM"])
MB_KEYS = ("obs", "next_obs", "actions", "reward", "done", "valid", "masks_next", "index")


def _np(t) -> np.ndarray:
    return t.detach().cpu().numpy()


def same(got, want, msg):
    """Equal dtype, shape and bytes (the sign of a zero included)."""
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, (msg, got.dtype, want.dtype, got.shape, want.shape)
    np.testing.assert_array_equal(got.view(np.uint8), want.view(np.uint8), err_msg=msg)


def same_lists(got, want, names, msg):
    assert len(got) == len(want) == len(names)
    for g, w, name in zip(got, want, names):
        same(g, w, f"{msg}: {name}")


# ------------------------------------------------------------------------------------------------- PPO: the device run
class PpoWorld:
    """A batch of its own on a side stream, the two heads and the optimiser; closed by the test."""

    def __init__(self, backward="torch"):
        import torch

        from collectivecrossing_amd.batched import BatchedCollectiveCrossing

        assert torch.cuda.is_available(), "gpu tests need an MI355X"
        self.env = env = BatchedCollectiveCrossing(chain_config(), PPO["E"])
        assert env.num_agents == N
        self.side = torch.cuda.Stream()
        env.use_stream(self.side)
        torch.cuda.synchronize()
        with torch.cuda.stream(self.side), torch.no_grad():
            env.make_reset_pool(seed0=POOL_SEED0, size=POOL_SIZE)
            env.reset_from_pool()
            env.synchronize()
            env.set_state(step_count=START_STEP_COUNT)
            env.set_rng_seed(SEED)
            torch.manual_seed(TORCH_SEED)
            self.actor = env.mlp_head(H, backward=backward)
            self.critic = env.mlp_head(H, O=1, activation="relu", backward=backward)
            self.opt = env.adam([*self.actor.parameters(), *self.critic.parameters()], lr=ppo_lr(0), **ADAM_KW)
        self.start = env.get_state()

    def heads(self):
        self.side.synchronize()
        return [[_np(p) for p in (h.w1t, h.b1, h.w2, h.b2)] for h in (self.actor, self.critic)]

    def final(self):
        self.side.synchronize()
        opt = self.opt
        return dict(params=[_np(p) for p in opt.params], m=[_np(t) for t in opt.m], v=[_np(t) for t in opt.v],
                    state_bytes=_np(opt.state))

    def close(self):
        self.env.use_stream(None)
        self.env.close()


def ppo_buffers(w):
    import torch

    env = w.env
    E, K, L, dev = PPO["E"], PPO["K"], env.obs_len, env.device
    return dict(traj=env.alloc_rollout(K, want_final=True), actions=torch.empty((K, E, N), dtype=torch.uint8, device=dev),
                logp=torch.empty((K, E, N), device=dev), masks=torch.empty((K, E, N), dtype=torch.uint8, device=dev),
                rows=torch.empty((K, E, N, L), device=dev))


def collect_eager(w):
    """The collection of examples/ppo_device_update.py: ``mlp_sample_actions`` + a one-step rollout on [s:s+1] slabs."""
    from collectivecrossing_amd import SampleResult
    from collectivecrossing_amd.batched import RolloutResult

    env, col = w.env, ppo_buffers(w)
    traj = col["traj"]
    obs, masks = env.observe(), env.action_masks()
    for s in range(PPO["K"]):
        col["rows"][s] = obs
        col["masks"][s] = masks
        env.mlp_sample_actions(w.actor, obs, masks, out=SampleResult(col["actions"][s], col["logp"][s], None))
        slab = RolloutResult(**{k: None if t is None else t[s:s + 1] for k, t in vars(traj).items()})
        obs = env.rollout(col["actions"][s:s + 1], auto_reset=True, reset_obs="next", out=slab, masks_out=masks).obs[0]
    return col


def collect_captured(w):
    """The same actor step on static buffers, captured once and replayed K times from ``set_state(**start)``."""
    import torch

    from collectivecrossing_amd import SampleResult

    env, col = w.env, ppo_buffers(w)
    E = PPO["E"]
    obs, masks = env.observe(), env.action_masks()
    actions = torch.empty((1, E, N), dtype=torch.uint8, device=env.device)
    sampled = SampleResult(actions[0], torch.empty((E, N), device=env.device), None)
    one = env.alloc_rollout(1, want_final=True)

    def body():
        env.mlp_sample_actions(w.actor, obs, masks, out=sampled)
        env.rollout(actions, auto_reset=True, reset_obs="next", out=one, masks_out=masks)
        obs.copy_(one.obs[0])

    body()                                                               # (a first eager run, then back to the start)
    w.side.synchronize()
    env.set_state(**w.start)
    env.observe(out=obs)
    env.action_masks(out=masks)
    w.side.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=w.side):
        body()
    traj = col["traj"]
    for s in range(PPO["K"]):
        col["rows"][s].copy_(obs)
        col["masks"][s].copy_(masks)
        graph.replay()
        col["actions"][s].copy_(actions[0])
        col["logp"][s].copy_(sampled.logp)
        for k in ("obs", "reward", "agent_flags", "env_flags", "final_obs"):
            getattr(traj, k)[s].copy_(getattr(one, k)[0])
    return col


def check_collection(col, ref, tag):
    """Links 1 and 2: masks, actions and logp per step; reward and flags; and the rows both sides carry along."""
    got = {k: _np(col[k]) for k in ("masks", "actions", "logp", "rows")}
    traj = col["traj"]
    for s in range(PPO["K"]):
        same(got["rows"][s], ref["rows"][s], f"{tag}: the rows step {s} acts on")
        same(got["masks"][s], ref["masks"][s], f"{tag}: masks of step {s}")
        same(got["actions"][s], ref["actions"][s], f"{tag}: actions of step {s}")
        same(got["logp"][s], ref["logp"][s], f"{tag}: logp of step {s}")
    same(_np(traj.reward), ref["reward"], f"{tag}: reward")
    same(_np(traj.agent_flags), ref["agent_flags"], f"{tag}: agent_flags")
    same(_np(traj.env_flags), ref["env_flags"], f"{tag}: env_flags")
    reset = (ref["env_flags"] & EF_RESET) != 0
    same(_np(traj.final_obs)[reset], ref["final_obs"][reset], f"{tag}: final_obs at EF_RESET")
    same(_np(traj.obs)[-1], ref["last_rows"], f"{tag}: the rows behind the last step")


def values_and_advantages(w, col):
    """Values from ``critic(rows)``, ``final_values`` from ``final_obs`` at EF_RESET rows, ``compute_gae``, ``masked_moments``."""
    import torch

    env, traj, critic = w.env, col["traj"], w.critic
    K, E = PPO["K"], PPO["E"]
    with torch.no_grad():
        values = critic(col["rows"]).squeeze(-1).contiguous()
        last_values = critic(traj.obs[K - 1]).squeeze(-1).contiguous()
        reset = (traj.env_flags & EF_RESET) != 0
        final_values = torch.zeros((K, E, N), device=env.device)
        final_values[reset] = critic(traj.final_obs[reset].contiguous()).squeeze(-1)
        gae = env.compute_gae(traj, values, last_values, final_values, gamma=PPO["GAMMA"], lam=PPO["LAM"])
        norm = env.masked_moments(gae.advantages, gae.valid)
    return dict(values=values, last_values=last_values, final_values=final_values, gae=gae, norm=norm)


def check_advantages(va, ref, tag):
    """Links 3, 4 and 5."""
    for k in ("values", "last_values", "final_values"):
        same(_np(va[k]), ref[k], f"{tag}: {k}")
    same(_np(va["gae"].advantages), ref["advantages"], f"{tag}: advantages")
    same(_np(va["gae"].returns), ref["returns"], f"{tag}: returns")
    same(_np(va["gae"].valid), ref["valid"], f"{tag}: valid")
    same(_np(va["norm"]), ref["norm"], f"{tag}: norm")


def update_buffers(w, col, va):
    """The static buffers and the update body of examples/ppo_device_update.py: (source, mb, loss, grads, update)."""
    import torch

    env, actor, critic, opt, gae, norm = w.env, w.actor, w.critic, w.opt, va["gae"], va["norm"]
    dev = env.device
    lead = (PPO["K"] // PPO["MINIBATCHES"], PPO["E"], N)
    source = dict(obs=col["rows"], acts=col["actions"], logp=col["logp"], adv=gae.advantages, ret=gae.returns, masks=col["masks"],
                  valid=gae.valid)
    mb = {k: torch.empty((lead[0],) + tuple(t.shape[1:]), dtype=t.dtype, device=dev) for k, t in source.items()}
    logits, hid_a = torch.empty(lead + (5,), device=dev), torch.empty(lead + (H,), device=dev)
    vals, hid_c = torch.empty(lead + (1,), device=dev), torch.empty(lead + (H,), device=dev)
    loss = env.alloc_ppo_loss(lead)
    ga, gc = env.alloc_mlp_backward(actor, lead), env.alloc_mlp_backward(critic, lead)
    grads = [ga.w1t, ga.b1, ga.w2, ga.b2, gc.w1t, gc.b1, gc.w2, gc.b2]

    def update():                                                        # library launches only
        actor(mb["obs"], out=logits, hidden_out=hid_a)
        critic(mb["obs"], out=vals, hidden_out=hid_c)
        args = (logits, vals.squeeze(-1), mb["acts"], mb["logp"], mb["adv"], mb["ret"])
        kw = dict(masks=mb["masks"], valid=mb["valid"], norm=norm, **PPO["HYPER"])
        env.ppo_loss(*args, **kw, out=loss)
        gl, gv = env.ppo_loss_backward(*args, **kw, stats=loss.stats, out=loss)
        env.mlp_backward(actor, mb["obs"], hid_a, gl, out=ga)
        env.mlp_backward(critic, mb["obs"], hid_c, gv.unsqueeze(-1), out=gc)
        opt.step(grads=grads)

    return source, mb, loss, grads, update


def gather(source, mb, steps, dev):
    """One minibatch of whole steps into the static buffers, by ``index_select`` with the NumPy permutation."""
    import torch

    index = torch.from_numpy(steps).to(dev)
    for k, t in source.items():
        torch.index_select(t, 0, index, out=mb[k])


def run_updates(w, col, va, ref, captured, check):
    """The eight updates on static buffers, eager or as ONE captured graph replayed eight times; the rate changes after the
    fourth.  ``check``: compare link 6 after every step."""
    import torch

    source, mb, loss, grads, update = update_buffers(w, col, va)
    step = update
    if captured:
        w.side.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=w.side):
            update()
        step = graph.replay
    for i, steps in enumerate(ref["minibatches"]):
        if i == PPO["LR_CHANGE_AFTER"]:
            w.opt.lr = ppo_lr(i)
        gather(source, mb, steps, w.env.device)
        step()
        if check:
            w.side.synchronize()
            same(_np(loss.stats), ref["stats"][i], f"update {i}: the loss stats")
            same_lists([_np(g) for g in grads], ref["grads"][i], GRAD_ORDER, f"update {i}: gradient")
            same(_np(w.opt.stats), ref["adam_stats"][i], f"update {i}: Adam's stats (norm, scale, skipped, rate)")
    return w.final()


def check_final(got, ref, tag):
    """Link 7."""
    for k in ("params", "m", "v"):
        same_lists(got[k], ref[k], GRAD_ORDER, f"{tag}: {k} after the last step")
    same(got["state_bytes"], ref["state_bytes"], f"{tag}: the optimiser's 64 state bytes")


@pytest.fixture(scope="module")
def ppo_ref(oracle):
    """The reference from the initial parameters of the device's freshly made heads; run once."""
    w = PpoWorld()
    try:
        init = w.heads()
    finally:
        w.close()
    ref = ppo_reference(*init)
    ref["init"] = init
    for k, v in ref["facts"].items():
        print(f"ppo {k}: {v}")
    assert_ppo_coverage(ref)
    return ref


def check_init(w, ref):
    for got, want, head in zip(w.heads(), ref["init"], ("actor", "critic")):
        same_lists(got, want, ("w1t", "b1", "w2", "b2"), f"{head}: the heads are made alike in every test")


# ------------------------------------------------------------------------------------------------- PPO: the tests
def test_ppo_iteration_eager(ppo_ref):
    import torch

    w = PpoWorld()
    try:
        check_init(w, ppo_ref)
        with torch.cuda.stream(w.side), torch.no_grad():
            col = collect_eager(w)
            w.side.synchronize()
            check_collection(col, ppo_ref, "eager")
            va = values_and_advantages(w, col)
            w.side.synchronize()
            check_advantages(va, ppo_ref, "eager")
            got = run_updates(w, col, va, ppo_ref, captured=False, check=True)
        check_final(got, ppo_ref, "eager")
        assert w.opt.counts() == (8, 0)
    finally:
        w.close()


def test_ppo_iteration_captured(ppo_ref):
    """The actor step captured and replayed K times from the start state, then the update captured once and replayed eight
    times with ``opt.lr`` set between the fourth and the fifth replay: the reference's history and final state, and the
    eager run's."""
    import torch

    w, e = PpoWorld(), PpoWorld()
    try:
        check_init(w, ppo_ref)
        with torch.cuda.stream(w.side), torch.no_grad():
            col = collect_captured(w)
            w.side.synchronize()
            check_collection(col, ppo_ref, "captured actor step")
            va = values_and_advantages(w, col)
            captured = run_updates(w, col, va, ppo_ref, captured=True, check=False)
        check_final(captured, ppo_ref, "captured")
        with torch.cuda.stream(e.side), torch.no_grad():
            col = collect_eager(e)
            eager = run_updates(e, col, values_and_advantages(e, col), ppo_ref, captured=False, check=False)
        check_final(captured, eager, "captured against eager")
    finally:
        w.close()
        e.close()


def test_ppo_iteration_through_autograd(ppo_ref):
    """The same eight updates with ``backward="device"`` heads, ``r.loss.backward()`` and ``opt.step()`` on the ``.grad``:
    the autograd path and the static-buffer path are the same rule."""
    import torch

    w = PpoWorld(backward="device")
    try:
        check_init(w, ppo_ref)
        env, opt = w.env, w.opt
        with torch.cuda.stream(w.side):
            with torch.no_grad():
                col = collect_eager(w)
            va = values_and_advantages(w, col)
            gae = va["gae"]
            source = dict(obs=col["rows"], acts=col["actions"], logp=col["logp"], adv=gae.advantages, ret=gae.returns,
                          masks=col["masks"], valid=gae.valid)
            for i, steps in enumerate(ppo_ref["minibatches"]):
                if i == PPO["LR_CHANGE_AFTER"]:
                    opt.lr = ppo_lr(i)
                index = torch.from_numpy(steps).to(env.device)
                mb = {k: torch.index_select(t, 0, index) for k, t in source.items()}
                opt.zero_grad(set_to_none=True)                          # (a fresh .grad: nothing is added onto old bits)
                r = env.ppo_loss(w.actor(mb["obs"]), w.critic(mb["obs"]).squeeze(-1), mb["acts"], mb["logp"], mb["adv"], mb["ret"],
                                 masks=mb["masks"], valid=mb["valid"], norm=va["norm"], **PPO["HYPER"])
                r.loss.backward()
                opt.step()
                w.side.synchronize()
                same(_np(r.stats), ppo_ref["stats"][i], f"update {i}: the loss stats")
                same_lists([_np(p.grad) for p in opt.params], ppo_ref["grads"][i], GRAD_ORDER, f"update {i}: .grad")
        check_final(w.final(), ppo_ref, "through autograd")
    finally:
        w.close()


# ------------------------------------------------------------------------------------------------- DQN
def compact_of_rows(rows):
    import torch

    return torch.stack([rows[:, 1, 6:10]] + [rows[:, 0, 6 + 4 * j:10 + 4 * j] for j in range(1, rows.shape[-2])], dim=1).contiguous()


def test_dqn_loop_captured_against_the_reference(oracle):
    """The loop of examples/dqn_replay_ring.py: an actor graph and an update graph replayed alternately, ``ql.epsilon`` set
    per round, the target synchronised every TARGET_EVERY updates."""
    import torch

    from collectivecrossing_amd import QLearning, ReplayRing, SideHeads
    from collectivecrossing_amd.batched import BatchedCollectiveCrossing
    from collectivecrossing_amd.qlearn import QActions

    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    E, B = DQN["E"], DQN["BATCH"]
    td_kw = dict(gamma=DQN["GAMMA"], huber_delta=DQN["HUBER_DELTA"])
    env = BatchedCollectiveCrossing(chain_config(), E)
    stream = torch.cuda.Stream()
    env.use_stream(stream)
    torch.cuda.synchronize()
    try:
        with torch.cuda.stream(stream), torch.no_grad():
            env.make_reset_pool(seed0=POOL_SEED0, size=POOL_SIZE)
            env.reset_from_pool()
            env.synchronize()
            env.set_state(step_count=DQN_START_STEP_COUNT)
            env.set_rng_seed(SEED)
            dev = env.device
            torch.manual_seed(TORCH_SEED)
            online = SideHeads(env, {s: env.mlp_head(H) for s in SIDES})
            target = SideHeads(env, {s: env.mlp_head(H) for s in SIDES})
            target.load_state_dict(online.state_dict())
            ql = QLearning(env, epsilon=DQN["EPS"][0])
            opt = env.adam(online.parameters(), lr=DQN["LR"], max_grad_norm=DQN["MAX_GRAD_NORM"])
            side_of = [online.slot_mask(i) for i in range(len(SIDES))]
            first_side = side_of[0].bool()
            ring = ReplayRing(env, steps=DQN["RING_STEPS"])
            stream.synchronize()
            init = [[_np(p) for p in (h.w1t, h.b1, h.w2, h.b2)] for h in online.heads]
            ref = dqn_reference(init)
            for k, v in ref["facts"].items():
                print(f"dqn {k}: {v}")
            assert_dqn_coverage(ref)

            # ---- the actor's static buffers
            u8, f32 = torch.uint8, torch.float32
            traj = env.alloc_rollout(1, want_obs=False, want_compact=True, want_final=True)
            acts = torch.empty((1, E, N), dtype=u8, device=dev)
            chosen = QActions(acts[0], torch.empty((E, N), dtype=u8, device=dev))
            q_act = torch.empty((E, N, 5), device=dev)
            obs, masks = env.observe(), env.action_masks()
            masks_next = masks.view(1, E, N)
            obs_c = compact_of_rows(obs)

            def actor_step():
                env.observe(out=obs)
                online(obs, out=q_act)
                ql.q_actions(q_act, masks, out=chosen)
                env.rollout(acts, auto_reset=True, reset_obs="next", out=traj, want_obs=False, want_compact=True, masks_out=masks)
                ring.push(obs_c, acts, traj, masks_next=masks_next)
                obs_c.copy_(traj.obs_compact[0])

            # ---- the update's static buffers
            lead = (B, N)
            mb = ring.alloc_batch(B)
            valid_of = [torch.empty(lead, dtype=u8, device=dev) for _ in SIDES]
            q, hid = torch.empty(lead + (5,), device=dev), torch.empty(lead + (H,), device=dev)
            q_next_target, q_next_online = torch.empty(lead + (5,), device=dev), torch.empty(lead + (5,), device=dev)
            losses = [ql.alloc_td_loss(lead, want_td_error=False) for _ in SIDES]
            gq = torch.empty(lead + (5,), dtype=f32, device=dev)
            grads = online.alloc_backward(lead)
            flat = [t for o in grads for t in (o.w1t, o.b1, o.w2, o.b2)]

            def update():
                ring.sample(B, out=mb)
                online(mb.obs, out=q, hidden_out=hid)
                target(mb.next_obs, out=q_next_target)
                online(mb.next_obs, out=q_next_online)
                args = (q, mb.actions, mb.reward, mb.done, q_next_target, q_next_online, mb.masks_next)
                for side, valid, loss in zip(side_of, valid_of, losses):
                    torch.mul(mb.valid, side, out=valid)
                    ql.td_loss(*args, valid=valid, **td_kw, out=loss)
                    ql.td_loss_backward(*args, valid=valid, **td_kw, stats=loss.stats, out=loss)
                torch.where(first_side[:, None], losses[0].grad_q, losses[1].grad_q, out=gq)
                online.backward_into(mb.obs, hid, gq, out=grads)
                opt.step(grads=flat)

            names = tuple(f"{s}.{n}" for s in SIDES for n in ("w1t", "b1", "w2", "b2"))
            for s in range(DQN["WARMUP"]):
                actor_step()
                stream.synchronize()
                same(_np(acts[0]), ref["actions"][s], f"warm-up step {s}: actions")
            actor_graph, update_graph = torch.cuda.CUDAGraph(), torch.cuda.CUDAGraph()
            with torch.cuda.graph(actor_graph, stream=stream):
                actor_step()
            with torch.cuda.graph(update_graph, stream=stream):
                update()
            stream.synchronize()

            for u in range(DQN["ROUNDS"]):
                ql.epsilon = dqn_epsilon(u)
                actor_graph.replay()
                update_graph.replay()
                stream.synchronize()
                tag = f"round {u}"
                assert ql.epsilon == ref["epsilon"][u]
                same(_np(acts[0]), ref["actions"][DQN["WARMUP"] + u], f"{tag}: actions")
                same(_np(chosen.explored), ref["explored"][DQN["WARMUP"] + u], f"{tag}: explored")
                same(_np(mb.index), ref["index"][u], f"{tag}: the drawn record indices")
                for k in MB_KEYS:
                    same(_np(getattr(mb, k)), ref["mb"][u][k], f"{tag}: minibatch {k}")
                for i, side in enumerate(SIDES):
                    same(_np(losses[i].stats), ref["td_stats"][u][i], f"{tag}: td stats of {side}")
                same_lists([_np(t) for t in flat], ref["grads"][u], names, f"{tag}: gradient")
                same(_np(opt.stats), ref["adam_stats"][u], f"{tag}: Adam's stats")
                if (u + 1) % DQN["TARGET_EVERY"] == 0:
                    torch._foreach_copy_(list(target.parameters()), list(online.parameters()))
            stream.synchronize()
            same_lists([_np(p) for p in opt.params], ref["params"], names, "the online parameters")
            same_lists([_np(p) for p in target.parameters()], ref["target"], names, "the target parameters")
            same_lists([_np(t) for t in opt.m], ref["m"], names, "m")
            same_lists([_np(t) for t in opt.v], ref["v"], names, "v")
            same(_np(opt.state), ref["state_bytes"], "the optimiser's 64 state bytes")
            assert ring.state[:2].tolist() == ref["ring_state"][:2].tolist() == [DQN["WARMUP"] + DQN["ROUNDS"], DQN["ROUNDS"]]
    finally:
        env.use_stream(None)
        env.close()
