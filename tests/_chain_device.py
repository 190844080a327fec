"""The device side of the three bigger loops, built from library calls only as the examples build them.  TEST INFRASTRUCTURE
ONLY: what tests/test_gpu_rainbow_chain.py, tests/test_gpu_c51_chain.py, tests/test_gpu_ppo_minibatch_chain.py and
tests/test_gpu_resume.py run and hold to the composed CPU references of tests/_rainbow_chain.py and tests/_c51_chain.py, bit for
bit.

``RainbowLoop``: the loop of examples/dqn_dueling.py with the reference's shapes on a batch and stream of its own -- the env
with its reset pool, terminated table and seed, the two ``SideHeads``, ring / ``NStepReplay`` / ``PrioritizedReplay``, the
optimiser, the static buffers of ``actor_step`` and ``update``, eager or as two graphs replayed alternately.  ``start`` puts
it at the reference's beginning; a resumed run restores a checkpoint instead (tests/test_gpu_resume.py).
``CategoricalLoop``: the categorical double-DQN of tests/_c51_chain.py over the same env and replay, five heads per network.
``World`` / ``collect`` / ``values_and_advantages`` / ``MinibatchUpdates``: the iteration of examples/ppo_minibatches.py.
Everything here runs inside ``with loop.scope():`` (the handle's stream current, no autograd)."""

import contextlib

import numpy as np
from _c51_chain import C51, C51_GRAD_ORDER, C51_LINKS, C51_START_STEP_COUNT
from _c51_chain import HEADS as C51_HEADS
from _learner_chain import (EF_RESET, GRAD_ORDER, H, N, POOL_SEED0, POOL_SIZE, PPO, SEED, SIDES, START_STEP_COUNT, chain_config,
                            ppo_lr)
from _rainbow_chain import (LINKS, MB_KEYS, PPO_MB, PPO_MB_KEYS, RAINBOW, RAINBOW_GRAD_ORDER, RAINBOW_START_STEP_COUNT,
                            hand_truncation, rainbow_beta, rainbow_epsilon, same, same_lists, terminated_tables)

L = 6 + 4 * N


def _np(t) -> np.ndarray:
    return t.detach().cpu().numpy()


def compact_of_rows(rows):
    import torch

    return torch.stack([rows[:, 1, 6:10]] + [rows[:, 0, 6 + 4 * j:10 + 4 * j] for j in range(1, rows.shape[-2])], dim=1).contiguous()


# ---------------------------------------------------------------------------------------------------------------------
# Rainbow
# ---------------------------------------------------------------------------------------------------------------------
class RainbowLoop:
    """Everything a run of the loop has to construct.  ``track``: ``track_episodes(log_capacity=track)`` before anything
    else.  ``start(init)`` begins the reference's run; the constructor alone leaves a fresh batch behind
    ``reset_from_pool()`` with fresh heads, replay objects and optimiser, which is what a resumed run loads into."""

    CONST, LINKS = RAINBOW, LINKS                    # the loop's constants and the links a checked round compares, in chain order

    def __init__(self, track: int = 0):
        import torch

        from collectivecrossing_amd import NStepReplay, PrioritizedReplay, QLearning, ReplayRing, SideHeads
        from collectivecrossing_amd.batched import BatchedCollectiveCrossing
        from collectivecrossing_amd.qlearn import QActions

        assert torch.cuda.is_available(), "gpu tests need an MI355X"
        R = RAINBOW
        E, B = R["E"], R["BATCH"]
        config = chain_config()
        self.env = env = BatchedCollectiveCrossing(config, E)
        self.stream = stream = torch.cuda.Stream()
        env.use_stream(stream)
        torch.cuda.synchronize()
        self.graphs = None
        with self.scope():
            if track:
                env.track_episodes(log_capacity=track)
            env.make_reset_pool(seed0=POOL_SEED0, size=POOL_SIZE)
            env.reset_from_pool()
            env.synchronize()
            env.set_terminated_table(*terminated_tables(config))
            env.set_rng_seed(SEED)
            dev = env.device
            self.online = online = SideHeads(env, {s: env.mlp_head(H, O=R["O"]) for s in SIDES})
            self.target = target = SideHeads(env, {s: env.mlp_head(H, O=R["O"]) for s in SIDES})
            self.ql = ql = QLearning(env, epsilon=R["EPS"][0])
            self.opt = opt = env.adam(online.parameters(), lr=R["LR"], max_grad_norm=R["MAX_GRAD_NORM"])
            side_of = [online.slot_mask(i) for i in range(len(SIDES))]
            first_side = side_of[0].bool()
            self.ring = ring = ReplayRing(env, steps=R["RING_STEPS"])
            self.ns = ns = NStepReplay(ring, n=R["N_STEP"], gamma=R["GAMMA"])
            self.pr = pr = PrioritizedReplay(ns, alpha=R["ALPHA"], beta=R["BETA"][0], eps=R["PRIO_EPS"])

            # ---- the actor's static buffers
            u8, f32 = torch.uint8, torch.float32
            self.traj = traj = env.alloc_rollout(1, want_obs=False, want_compact=True, want_final=True)
            self.acts = acts = torch.empty((1, E, N), dtype=u8, device=dev)
            self.chosen = chosen = QActions(acts[0], torch.empty((E, N), dtype=u8, device=dev))
            self.obs, self.masks = obs, masks = env.observe(), env.action_masks()
            masks_next = masks.view(1, E, N)
            self.obs_c = obs_c = compact_of_rows(obs)

            def actor_step():
                env.observe(out=obs)
                ql.sides_q_actions(online, obs, masks, out=chosen)
                env.rollout(acts, auto_reset=True, reset_obs="next", out=traj, want_obs=False, want_compact=True, masks_out=masks)
                pr.push(obs_c, acts, traj, masks_next=masks_next)
                obs_c.copy_(traj.obs_compact[0])

            # ---- the update's static buffers
            lead = (B, N)
            self.pmb = pmb = pr.alloc_batch(B)
            mb, discount = pmb.batch.batch, pmb.batch.discount
            valid_of = [torch.empty(lead, dtype=u8, device=dev) for _ in SIDES]
            hid = torch.empty(lead + (H,), device=dev)
            va = tuple(torch.empty(lead + (6,), device=dev) for _ in range(3))
            qs = tuple(torch.empty(lead + (5,), device=dev) for _ in range(3))
            q, q_next_target, q_next_online = qs
            losses = [ql.alloc_td_loss(lead, want_td_error=True) for _ in SIDES]
            gq = torch.empty(lead + (5,), dtype=f32, device=dev)
            gva = torch.empty(lead + (6,), dtype=f32, device=dev)
            grads = online.alloc_backward(lead)
            flat = [t for o in grads for t in (o.w1t, o.b1, o.w2, o.b2)]

            def update():
                pr.sample(B, out=pmb)
                online(mb.obs, out=va[0], hidden_out=hid)
                target(mb.next_obs, out=va[1])
                online(mb.next_obs, out=va[2])
                ql.dueling_into(va, qs)
                args = (q, mb.actions, mb.reward, mb.done, q_next_target, q_next_online, mb.masks_next)
                for side, valid, loss in zip(side_of, valid_of, losses):
                    torch.mul(mb.valid, side, out=valid)
                    kw = dict(valid=valid, weights=pmb.weights, discount=discount, huber_delta=R["HUBER_DELTA"])
                    ql.td_loss(*args, **kw, want_td_error=True, out=loss)
                    ql.td_loss_backward(*args, **kw, stats=loss.stats, out=loss)
                torch.where(first_side[:, None], losses[0].grad_q, losses[1].grad_q, out=gq)
                ql.dueling_backward(gq, out=gva)
                online.backward_into(mb.obs, hid, gva, out=grads)
                opt.step(grads=flat)
                pr.update_priorities(mb.index, tuple(l.td_error for l in losses))

            def got_of_round() -> dict:
                got = dict(actions=acts[0], explored=chosen.explored, index=pmb.batch.index, weights=pmb.weights,
                           leaf_drawn=pmb.leaf_drawn, grad_q=gq, gva=gva, adam_stats=opt.stats, leaf=pr.leaf, pstate=pr.pstate, cut=ns.cut)
                got.update({f"mb.{k}": getattr(mb, k) for k in MB_KEYS[:8]})
                got.update({"mb.discount": discount, "mb.span": pmb.batch.span})
                for i, s in enumerate(SIDES):
                    got[f"td_stats.{s}"], got[f"td_error.{s}"] = losses[i].stats, losses[i].td_error
                got.update({f"grad.{g}": t for g, t in zip(RAINBOW_GRAD_ORDER, flat)})
                return got

            self.actor_step, self.update, self.got_of_round = actor_step, update, got_of_round
            self.step_actor, self.step_update = actor_step, update

    @contextlib.contextmanager
    def scope(self):
        import torch

        with torch.cuda.stream(self.stream), torch.no_grad():
            yield

    def start(self, init) -> None:
        """The reference's beginning: staggered step counters, the committed parameters, target := online."""
        import torch

        self.env.set_state(step_count=RAINBOW_START_STEP_COUNT)
        for head, par in zip(self.online.heads, init):
            for t, a in zip((head.w1t, head.b1, head.w2, head.b2), par):
                t.copy_(torch.from_numpy(a))
        self.target.load_state_dict(self.online.state_dict())

    def online_parameters(self) -> list:
        return list(self.online.parameters())

    def target_parameters(self) -> list:
        return list(self.target.parameters())

    def refresh_actor_inputs(self) -> None:
        """After the env state was put somewhere else by hand: ``obs_c`` and the masks the next actor step reads."""
        self.env.observe(out=self.obs)
        self.obs_c.copy_(compact_of_rows(self.obs))
        self.env.action_masks(out=self.masks)

    def warm_up(self, ref) -> None:
        for s in range(self.CONST["WARMUP"]):
            self.actor_step()
            self.stream.synchronize()
            same(_np(self.acts[0]), ref["actions"][s], f"warm-up step {s}: actions")

    def capture(self) -> None:
        """The actor step and the update as two graphs, from here on replayed alternately."""
        import torch

        actor_graph, update_graph = torch.cuda.CUDAGraph(), torch.cuda.CUDAGraph()
        with torch.cuda.graph(actor_graph, stream=self.stream):
            self.actor_step()
        with torch.cuda.graph(update_graph, stream=self.stream):
            self.update()
        self.stream.synchronize()
        self.graphs = (actor_graph, update_graph)
        self.step_actor, self.step_update = actor_graph.replay, update_graph.replay

    def run_rounds(self, ref, first: int, last: int, check: bool) -> None:
        """Rounds ``first .. last - 1`` with the hand truncation, the event and the rates of the reference; ``check``: every
        link of every round against ``ref["rounds"][u]``, in chain order."""
        import torch

        R, env, stream, ql, pr = self.CONST, self.env, self.stream, self.ql, self.pr
        for u in range(first, last):
            if u == R["TRUNC_ROUND"]:                                # out of band, eagerly: a user truncation by hand
                stream.synchronize()
                env.set_state(truncated=hand_truncation(env.get_state()["truncated"]))
                env.action_masks(out=self.masks)
            if u == R["EVENT_ROUND"]:                                # out of band, eagerly: the envs put back
                env.reset_from_pool()
                self.ns.mark_cut()
                self.refresh_actor_inputs()
            ql.epsilon = rainbow_epsilon(u)
            pr.beta = rainbow_beta(u)
            self.step_actor()
            self.step_update()
            if check:
                stream.synchronize()
                assert ql.epsilon == ref["epsilon"][u] and pr.beta == ref["beta"][u]
                got = self.got_of_round()
                for k in self.LINKS:
                    same(_np(got[k]), ref["rounds"][u][k], f"round {u}: {k}")
            if (u + 1) % R["TARGET_EVERY"] == 0:
                torch._foreach_copy_(self.target_parameters(), self.online_parameters())
        stream.synchronize()

    def final(self) -> dict:
        """The final state as NumPy arrays."""
        self.stream.synchronize()
        opt, pr = self.opt, self.pr
        return dict(params=[_np(p) for p in opt.params], target=[_np(p) for p in self.target_parameters()], m=[_np(t) for t in opt.m],
                    v=[_np(t) for t in opt.v], state_bytes=_np(opt.state), ring_state=_np(self.ring.state), leaf=_np(pr.leaf),
                    pstate=_np(pr.pstate), cut=_np(self.ns.cut))

    def close(self) -> None:
        self.graphs = None
        self.env.use_stream(None)
        self.env.close()


def check_rainbow_final(got, ref, tag):
    for k in ("params", "target", "m", "v"):
        same_lists(got[k], ref[k], RAINBOW_GRAD_ORDER, f"{tag}: {k} after the last round")
    for k in ("state_bytes", "ring_state", "leaf", "pstate", "cut"):
        same(got[k], ref[k], f"{tag}: {k} after the last round")
    assert got["ring_state"][:2].tolist() == [RAINBOW["WARMUP"] + RAINBOW["ROUNDS"], 0] and int(got["pstate"][1]) == RAINBOW["ROUNDS"]


# ---------------------------------------------------------------------------------------------------------------------
# Categorical (C51) double-DQN over the same replay
# ---------------------------------------------------------------------------------------------------------------------
class CategoricalLoop(RainbowLoop):
    """The loop of tests/_c51_chain.py from library calls only: the Rainbow loop's env, ring / ``NStepReplay`` /
    ``PrioritizedReplay`` and out-of-band acts (``scope``, ``warm_up``, ``capture``, ``run_rounds`` and ``close`` are
    inherited), with FIVE heads ``env.mlp_head(H, O=A)`` per network -- head k gives the atom logits of action k; A = 8 is
    the device head's limit, not a choice about C51 -- copied into one contiguous ``[..., 5, A]`` buffer, ``CategoricalQ``
    for the expected values, the loss and its backward, ``grad_logits[..., k, :]`` copied out for ``mlp_backward`` of head k,
    and one Adam over the 20 parameter tensors.  Static buffers throughout: the actor step and the update capture as two
    graphs.  ``autograd=True``: the update calls ``loss`` on a leaf logits tensor that requires a gradient (filled from the
    heads) and reads ``logits.grad`` behind ``r.loss.backward()`` in the place of ``loss_backward(out=)``; eager only."""

    CONST, LINKS = C51, C51_LINKS

    def __init__(self, autograd: bool = False):
        import torch

        from collectivecrossing_amd import CategoricalQ, NStepReplay, PrioritizedReplay, QLearning, ReplayRing
        from collectivecrossing_amd.batched import BatchedCollectiveCrossing
        from collectivecrossing_amd.qlearn import QActions

        assert torch.cuda.is_available(), "gpu tests need an MI355X"
        C = C51
        E, B, A = C["E"], C["BATCH"], C["ATOMS"]
        config = chain_config()
        self.env = env = BatchedCollectiveCrossing(config, E)
        self.stream = stream = torch.cuda.Stream()
        env.use_stream(stream)
        torch.cuda.synchronize()
        self.graphs = None
        with self.scope():
            env.make_reset_pool(seed0=POOL_SEED0, size=POOL_SIZE)
            env.reset_from_pool()
            env.synchronize()
            env.set_terminated_table(*terminated_tables(config))
            env.set_rng_seed(SEED)
            dev = env.device
            self.online = online = [env.mlp_head(H, O=A) for _ in range(C51_HEADS)]
            self.target = target = [env.mlp_head(H, O=A) for _ in range(C51_HEADS)]
            self.cq = cq = CategoricalQ(env, atoms=A, vmin=C["VMIN"], vmax=C["VMAX"])
            self.ql = ql = QLearning(env, epsilon=C["EPS"][0])
            self.opt = opt = env.adam(self.online_parameters(), lr=C["LR"], max_grad_norm=C["MAX_GRAD_NORM"])
            self.ring = ring = ReplayRing(env, steps=C["RING_STEPS"])
            self.ns = ns = NStepReplay(ring, n=C["N_STEP"], gamma=C["GAMMA"])
            self.pr = pr = PrioritizedReplay(ns, alpha=C["ALPHA"], beta=C["BETA"][0], eps=C["PRIO_EPS"])

            def forward(net, x, logits, scratch, hidden=None):
                """The five heads on rows x into the contiguous [..., 5, A] buffer: exact copies of their outputs."""
                for k, head in enumerate(net):
                    head(x, out=scratch[k], hidden_out=None if hidden is None else hidden[k])
                    logits[..., k, :].copy_(scratch[k])

            # ---- the actor's static buffers
            u8, f32 = torch.uint8, torch.float32
            self.traj = traj = env.alloc_rollout(1, want_obs=False, want_compact=True, want_final=True)
            self.acts = acts = torch.empty((1, E, N), dtype=u8, device=dev)
            self.chosen = chosen = QActions(acts[0], torch.empty((E, N), dtype=u8, device=dev))
            self.obs, self.masks = obs, masks = env.observe(), env.action_masks()
            masks_next = masks.view(1, E, N)
            self.obs_c = obs_c = compact_of_rows(obs)
            act_scratch = [torch.empty((E, N, A), device=dev) for _ in range(C51_HEADS)]
            act_logits = torch.empty((E, N, C51_HEADS, A), device=dev)
            q_act = torch.empty((E, N, 5), device=dev)

            def actor_step():
                env.observe(out=obs)
                forward(online, obs, act_logits, act_scratch)
                cq.q_values(act_logits, out=q_act)
                ql.q_actions(q_act, masks, out=chosen)
                env.rollout(acts, auto_reset=True, reset_obs="next", out=traj, want_obs=False, want_compact=True, masks_out=masks)
                pr.push(obs_c, acts, traj, masks_next=masks_next)
                obs_c.copy_(traj.obs_compact[0])

            # ---- the update's static buffers
            lead = (B, N)
            self.pmb = pmb = pr.alloc_batch(B)
            mb, discount = pmb.batch.batch, pmb.batch.discount
            scratch = [torch.empty(lead + (A,), device=dev) for _ in range(C51_HEADS)]
            hid = [torch.empty(lead + (H,), device=dev) for _ in range(C51_HEADS)]
            logits, next_target, next_online = (torch.empty(lead + (C51_HEADS, A), dtype=f32, device=dev) for _ in range(3))
            loss = cq.alloc_loss(lead, want_row_loss=True)
            seen = dict(stats=loss.stats, row_loss=loss.row_loss, proj=loss.proj, grad_logits=loss.grad_logits)
            grads = [env.alloc_mlp_backward(head, lead) for head in online]
            flat = [t for o in grads for t in (o.w1t, o.b1, o.w2, o.b2)]
            if autograd:
                logits.requires_grad_()                              # a leaf; the heads fill it under no_grad

            def update():
                pr.sample(B, out=pmb)
                forward(online, mb.obs, logits, scratch, hid)
                forward(target, mb.next_obs, next_target, scratch)
                forward(online, mb.next_obs, next_online, scratch)
                args = (logits, mb.actions, mb.reward, mb.done, next_target)
                kw = dict(next_online=next_online, masks_next=mb.masks_next, valid=mb.valid, weights=pmb.weights, discount=discount)
                if autograd:
                    logits.grad = None
                    with torch.enable_grad():
                        r = cq.loss(*args, **kw, want_row_loss=True)
                        r.loss.backward()
                    seen.update(stats=r.stats, row_loss=r.row_loss, proj=r.proj, grad_logits=logits.grad)
                else:
                    cq.loss(*args, **kw, out=loss)
                    cq.loss_backward(logits, mb.actions, loss.proj, mb.valid, pmb.weights, stats=loss.stats, out=loss)
                for k, head in enumerate(online):
                    scratch[k].copy_(seen["grad_logits"][..., k, :])
                    env.mlp_backward(head, mb.obs, hid[k], scratch[k], out=grads[k])
                opt.step(grads=flat)
                pr.update_priorities(mb.index, seen["row_loss"])

            def got_of_round() -> dict:
                got = dict(actions=acts[0], explored=chosen.explored, index=pmb.batch.index, weights=pmb.weights,
                           leaf_drawn=pmb.leaf_drawn, logits=logits, next_target=next_target, next_online=next_online, **seen,
                           adam_stats=opt.stats, leaf=pr.leaf, pstate=pr.pstate, cut=ns.cut)
                got.update({f"mb.{k}": getattr(mb, k) for k in MB_KEYS[:8]})
                got.update({"mb.discount": discount, "mb.span": pmb.batch.span})
                got.update({f"grad.{g}": t for g, t in zip(C51_GRAD_ORDER, flat)})
                return got

            self.actor_step, self.update, self.got_of_round = actor_step, update, got_of_round
            self.step_actor, self.step_update = actor_step, update

    def online_parameters(self) -> list:
        return [t for h in self.online for t in (h.w1t, h.b1, h.w2, h.b2)]

    def target_parameters(self) -> list:
        return [t for h in self.target for t in (h.w1t, h.b1, h.w2, h.b2)]

    def start(self, init) -> None:
        """The reference's beginning: staggered step counters, the committed parameters, target := online."""
        import torch

        self.env.set_state(step_count=C51_START_STEP_COUNT)
        for t, a in zip(self.online_parameters(), (a for par in init for a in par)):
            t.copy_(torch.from_numpy(a))
        torch._foreach_copy_(self.target_parameters(), self.online_parameters())


def check_c51_final(got, ref, tag):
    for k in ("params", "target", "m", "v"):
        same_lists(got[k], ref[k], C51_GRAD_ORDER, f"{tag}: {k} after the last round")
    for k in ("state_bytes", "ring_state", "leaf", "pstate", "cut"):
        same(got[k], ref[k], f"{tag}: {k} after the last round")
    assert got["ring_state"][:2].tolist() == [C51["WARMUP"] + C51["ROUNDS"], 0] and int(got["pstate"][1]) == C51["ROUNDS"]


# ---------------------------------------------------------------------------------------------------------------------
# PPO with device-drawn minibatches
# ---------------------------------------------------------------------------------------------------------------------
class World:
    """A batch of its own on a side stream, the two heads and the optimiser; ``init``: the committed parameters, or None
    (whatever ``mlp_head`` made: a resumed run loads its own)."""

    def __init__(self, init=None):
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
            self.actor = env.mlp_head(H)
            self.critic = env.mlp_head(H, O=1, activation="relu")
            if init is not None:
                for head, par in zip((self.actor, self.critic), init):
                    for t, a in zip((head.w1t, head.b1, head.w2, head.b2), par):
                        t.copy_(torch.from_numpy(a))
            self.opt = env.adam([*self.actor.parameters(), *self.critic.parameters()], lr=ppo_lr(0), weight_decay=PPO["WEIGHT_DECAY"],
                                max_grad_norm=PPO_MB["MAX_GRAD_NORM"])

    @contextlib.contextmanager
    def scope(self):
        import torch

        with torch.cuda.stream(self.side), torch.no_grad():
            yield

    def final(self, mb):
        self.side.synchronize()
        opt = self.opt
        return dict(params=[_np(p) for p in opt.params], m=[_np(t) for t in opt.m], v=[_np(t) for t in opt.v],
                    state_bytes=_np(opt.state), mb_state=_np(mb.state))

    def close(self):
        self.env.use_stream(None)
        self.env.close()


def collect(w, compact: bool):
    """The collection of examples/ppo_minibatches.py: ``traj.obs[s]`` is the row BEHIND step s, ``obs0`` the one step 0 acted on."""
    import torch

    from collectivecrossing_amd import SampleResult
    from collectivecrossing_amd.batched import RolloutResult

    env = w.env
    E, K, dev = PPO["E"], PPO["K"], env.device
    traj = env.alloc_rollout(K, want_obs=True, want_compact=compact, want_final=True)
    col = dict(traj=traj, actions=torch.empty((K, E, N), dtype=torch.uint8, device=dev), logp=torch.empty((K, E, N), device=dev),
               masks=torch.empty((K, E, N), dtype=torch.uint8, device=dev))
    col["obs0"], masks = env.observe().clone(), env.action_masks()
    obs = col["obs0"]
    for s in range(K):
        col["masks"][s] = masks
        env.mlp_sample_actions(w.actor, obs, masks, out=SampleResult(col["actions"][s], col["logp"][s], None))
        slab = RolloutResult(**{k: None if t is None else t[s:s + 1] for k, t in vars(traj).items()})
        obs = env.rollout(col["actions"][s:s + 1], auto_reset=True, reset_obs="next", out=slab, want_compact=compact, masks_out=masks).obs[0]
    return col


def values_and_advantages(w, col):
    import torch

    env, traj, critic = w.env, col["traj"], w.critic
    K, E = PPO["K"], PPO["E"]
    values = torch.empty((K, E, N), device=env.device)
    values[0] = critic(col["obs0"]).squeeze(-1)
    values[1:] = critic(traj.obs[:K - 1]).squeeze(-1)
    last_values = critic(traj.obs[K - 1]).squeeze(-1).contiguous()
    reset = (traj.env_flags & EF_RESET) != 0
    final_values = torch.zeros((K, E, N), device=env.device)
    final_values[reset] = critic(traj.final_obs[reset].contiguous()).squeeze(-1)
    gae = env.compute_gae(traj, values, last_values, final_values, gamma=PPO["GAMMA"], lam=PPO["LAM"])
    return dict(values=values, last_values=last_values, final_values=final_values, gae=gae, norm=env.masked_moments(gae.advantages, gae.valid))


def minibatch_source(col, va, form) -> dict:
    """What ``set_source`` is given, by keyword, and the ``norm`` of the loss: everything of the collection an update reads."""
    traj, gae = col["traj"], va["gae"]
    obs, obs0 = (traj.obs_compact, compact_of_rows(col["obs0"])) if form == "compact" else (traj.obs, col["obs0"])
    return dict(obs=obs, actions=col["actions"], logp=col["logp"], advantages=gae.advantages, returns=gae.returns, masks=col["masks"],
                valid=gae.valid, obs0=obs0)


class MinibatchUpdates:
    """The updates of examples/ppo_minibatches.py on static buffers, ``mb.next`` inside: a new ``RolloutMinibatches`` over
    ``source`` (:func:`minibatch_source`, or the same tensors from a checkpoint), eager, or ONE captured graph replayed."""

    def __init__(self, w, source: dict, norm):
        import torch

        from collectivecrossing_amd import RolloutMinibatches

        self.w = w
        env, actor, critic, opt = w.env, w.actor, w.critic, w.opt
        dev = env.device
        self.mb = mb = RolloutMinibatches(env, num_steps=PPO["K"], batch_size=PPO_MB["B"])
        mb.set_source(**source)
        self.batch = batch = mb.alloc()
        lead = (mb.batch_size, N)
        logits, hid_a = torch.empty(lead + (5,), device=dev), torch.empty(lead + (H,), device=dev)
        vals, hid_c = torch.empty(lead + (1,), device=dev), torch.empty(lead + (H,), device=dev)
        self.loss = loss = env.alloc_ppo_loss(lead)
        ga, gc = env.alloc_mlp_backward(actor, lead), env.alloc_mlp_backward(critic, lead)
        self.grads = grads = [ga.w1t, ga.b1, ga.w2, ga.b2, gc.w1t, gc.b1, gc.w2, gc.b2]

        def update():                                                        # library launches only, the gather included
            mb.next(out=batch)
            actor(batch.obs, out=logits, hidden_out=hid_a)
            critic(batch.obs, out=vals, hidden_out=hid_c)
            args = (logits, vals.squeeze(-1), batch.actions, batch.logp, batch.advantages, batch.returns)
            kw = dict(masks=batch.masks, valid=batch.valid, norm=norm, **PPO["HYPER"])
            env.ppo_loss(*args, **kw, out=loss)
            gl, gv = env.ppo_loss_backward(*args, **kw, stats=loss.stats, out=loss)
            env.mlp_backward(actor, batch.obs, hid_a, gl, out=ga)
            env.mlp_backward(critic, batch.obs, hid_c, gv.unsqueeze(-1), out=gc)
            opt.step(grads=grads)

        self.update = self.step = update
        self.graph = None

    def capture(self) -> None:
        import torch

        self.w.side.synchronize()
        self.graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self.graph, stream=self.w.side):
            self.update()
        self.step = self.graph.replay

    def run(self, ref, first: int, last: int, check: bool) -> None:
        """Updates ``first .. last - 1``; the rate changes before update LR_CHANGE_AFTER.  ``check``: every link after every step."""
        w, opt, batch = self.w, self.w.opt, self.batch
        for i in range(first, last):
            if i == PPO["LR_CHANGE_AFTER"]:
                opt.lr = ppo_lr(i)
            self.step()
            if check:
                w.side.synchronize()
                same(_np(batch.index), ref["index"][i], f"update {i}: batch.index")
                for k in PPO_MB_KEYS:
                    same(_np(getattr(batch, k)), ref["mb"][i][k], f"update {i}: minibatch {k}")
                same(_np(self.loss.stats), ref["stats"][i], f"update {i}: the loss stats")
                same_lists([_np(g) for g in self.grads], ref["grads"][i], GRAD_ORDER, f"update {i}: gradient")
                same(_np(opt.stats), ref["adam_stats"][i], f"update {i}: Adam's stats (norm, scale, skipped, rate)")


def check_ppo_final(got, ref, tag):
    for k in ("params", "m", "v"):
        same_lists(got[k], ref[k], GRAD_ORDER, f"{tag}: {k} after the last step")
    same(got["state_bytes"], ref["state_bytes"], f"{tag}: the optimiser's 64 state bytes")
    same(got["mb_state"], ref["mb_state"], f"{tag}: the minibatch state")
    assert got["mb_state"].tolist() == [PPO_MB["EPOCHS"], 0, 0, 0]
