"""The whole loop of examples/dqn_dueling.py on the device against the composed CPU reference of tests/_rainbow_chain.py, bit
for bit: prioritised replay over an n-step ring, per-side dueling heads, the fused actor launch, both sides' ``td_error`` into
``update_priorities``.  What no per-op test and no run-against-run comparison can see is compared here: the leaves made from
the loss's own ``td_error`` and what they do to the next draw and its weights, max-leaf on records pushed after it rose, the
window's end on real cut bytes under a prioritised draw when the ring wraps, ``next_obs`` / ``masks_next`` from the window's
last slot, the per-row discount in the loss, ``dueling_backward`` between ``grad_q`` and ``backward_into``, the fused actor on
a real state across auto-resets, ``beta`` and ``epsilon`` written between graph replays, and two out-of-band acts between two
replays: a hand truncation (``set_state(truncated=)``: dropped rows) and the envs put back (``reset_from_pool`` + ``mark_cut``).

The loop is built from library calls only, as the example does, on a batch and stream of its own; the heads are made with
``env.mlp_head(H, O=6)`` and the ``linear_init`` parameters of tests/test_rainbow_chain_reference.py are copied into them, so the
reference the device is held to is the one whose coverage the CPU test asserts (asserted again here, once per module).
Comparisons go in chain order (``LINKS``), so a failure names the first link that differs."""

import numpy as np
import pytest
from _learner_chain import H, N, POOL_SEED0, POOL_SIZE, SEED, SIDES, chain_config
from _mlp_spec import linear_init
from _rainbow_chain import (LINKS, MB_KEYS, RAINBOW, RAINBOW_GRAD_ORDER, RAINBOW_INIT_SEEDS, RAINBOW_START_STEP_COUNT,
                            assert_rainbow_coverage, hand_truncation, rainbow_beta, rainbow_epsilon, rainbow_reference, same,
                            same_lists, terminated_tables)

pytestmark = pytest.mark.gpu

L = 6 + 4 * N


def _np(t) -> np.ndarray:
    return t.detach().cpu().numpy()


@pytest.fixture(scope="module")
def rainbow_ref(oracle):
    """The reference from the committed ``linear_init`` parameters; run once."""
    init = [linear_init(L, H, RAINBOW["O"], seed=s) for s in RAINBOW_INIT_SEEDS]
    ref = rainbow_reference(init)
    ref["init"] = init
    for k, v in ref["facts"].items():
        print(f"rainbow {k}: {v}")
    assert_rainbow_coverage(ref)
    return ref


def compact_of_rows(rows):
    import torch

    return torch.stack([rows[:, 1, 6:10]] + [rows[:, 0, 6 + 4 * j:10 + 4 * j] for j in range(1, rows.shape[-2])], dim=1).contiguous()


def run_loop(ref, captured: bool, check: bool) -> dict:
    """The loop of examples/dqn_dueling.py with the reference's shapes, eager or as two graphs replayed alternately;
    ``check``: every link of every round against the reference.  Returns the final state as NumPy arrays."""
    import torch

    from collectivecrossing_amd import NStepReplay, PrioritizedReplay, QLearning, ReplayRing, SideHeads
    from collectivecrossing_amd.batched import BatchedCollectiveCrossing
    from collectivecrossing_amd.qlearn import QActions

    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    R = RAINBOW
    E, B, W = R["E"], R["BATCH"], R["WARMUP"]
    config = chain_config()
    env = BatchedCollectiveCrossing(config, E)
    stream = torch.cuda.Stream()
    env.use_stream(stream)
    torch.cuda.synchronize()
    try:
        with torch.cuda.stream(stream), torch.no_grad():
            env.make_reset_pool(seed0=POOL_SEED0, size=POOL_SIZE)
            env.reset_from_pool()
            env.synchronize()
            env.set_state(step_count=RAINBOW_START_STEP_COUNT)
            env.set_terminated_table(*terminated_tables(config))
            env.set_rng_seed(SEED)
            dev = env.device
            online = SideHeads(env, {s: env.mlp_head(H, O=R["O"]) for s in SIDES})
            target = SideHeads(env, {s: env.mlp_head(H, O=R["O"]) for s in SIDES})
            for head, init in zip(online.heads, ref["init"]):
                for t, a in zip((head.w1t, head.b1, head.w2, head.b2), init):
                    t.copy_(torch.from_numpy(a))
            target.load_state_dict(online.state_dict())
            ql = QLearning(env, epsilon=R["EPS"][0])
            opt = env.adam(online.parameters(), lr=R["LR"], max_grad_norm=R["MAX_GRAD_NORM"])
            side_of = [online.slot_mask(i) for i in range(len(SIDES))]
            first_side = side_of[0].bool()
            ring = ReplayRing(env, steps=R["RING_STEPS"])
            ns = NStepReplay(ring, n=R["N_STEP"], gamma=R["GAMMA"])
            pr = PrioritizedReplay(ns, alpha=R["ALPHA"], beta=R["BETA"][0], eps=R["PRIO_EPS"])

            # ---- the actor's static buffers
            u8, f32 = torch.uint8, torch.float32
            traj = env.alloc_rollout(1, want_obs=False, want_compact=True, want_final=True)
            acts = torch.empty((1, E, N), dtype=u8, device=dev)
            chosen = QActions(acts[0], torch.empty((E, N), dtype=u8, device=dev))
            obs, masks = env.observe(), env.action_masks()
            masks_next = masks.view(1, E, N)
            obs_c = compact_of_rows(obs)

            def actor_step():
                env.observe(out=obs)
                ql.sides_q_actions(online, obs, masks, out=chosen)
                env.rollout(acts, auto_reset=True, reset_obs="next", out=traj, want_obs=False, want_compact=True, masks_out=masks)
                pr.push(obs_c, acts, traj, masks_next=masks_next)
                obs_c.copy_(traj.obs_compact[0])

            # ---- the update's static buffers
            lead = (B, N)
            pmb = pr.alloc_batch(B)
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

            for s in range(W):
                actor_step()
                stream.synchronize()
                same(_np(acts[0]), ref["actions"][s], f"warm-up step {s}: actions")
            step_actor, step_update = actor_step, update
            if captured:
                actor_graph, update_graph = torch.cuda.CUDAGraph(), torch.cuda.CUDAGraph()
                with torch.cuda.graph(actor_graph, stream=stream):
                    actor_step()
                with torch.cuda.graph(update_graph, stream=stream):
                    update()
                stream.synchronize()
                step_actor, step_update = actor_graph.replay, update_graph.replay

            for u in range(R["ROUNDS"]):
                if u == R["TRUNC_ROUND"]:                                # out of band, eagerly: a user truncation by hand
                    stream.synchronize()
                    env.set_state(truncated=hand_truncation(env.get_state()["truncated"]))
                    env.action_masks(out=masks)
                if u == R["EVENT_ROUND"]:                                # out of band, eagerly: the envs put back
                    env.reset_from_pool()
                    ns.mark_cut()
                    env.observe(out=obs)
                    obs_c.copy_(compact_of_rows(obs))
                    env.action_masks(out=masks)
                ql.epsilon = rainbow_epsilon(u)
                pr.beta = rainbow_beta(u)
                step_actor()
                step_update()
                if check:
                    stream.synchronize()
                    assert ql.epsilon == ref["epsilon"][u] and pr.beta == ref["beta"][u]
                    got = got_of_round()
                    for k in LINKS:
                        same(_np(got[k]), ref["rounds"][u][k], f"round {u}: {k}")
                if (u + 1) % R["TARGET_EVERY"] == 0:
                    torch._foreach_copy_(list(target.parameters()), list(online.parameters()))
            stream.synchronize()
            assert opt.counts() == (R["ROUNDS"], 0)
            return dict(params=[_np(p) for p in opt.params], target=[_np(p) for p in target.parameters()], m=[_np(t) for t in opt.m],
                        v=[_np(t) for t in opt.v], state_bytes=_np(opt.state), ring_state=_np(ring.state), leaf=_np(pr.leaf),
                        pstate=_np(pr.pstate), cut=_np(ns.cut))
    finally:
        env.use_stream(None)
        env.close()


def check_final(got, ref, tag):
    for k in ("params", "target", "m", "v"):
        same_lists(got[k], ref[k], RAINBOW_GRAD_ORDER, f"{tag}: {k} after the last round")
    for k in ("state_bytes", "ring_state", "leaf", "pstate", "cut"):
        same(got[k], ref[k], f"{tag}: {k} after the last round")
    assert got["ring_state"][:2].tolist() == [RAINBOW["WARMUP"] + RAINBOW["ROUNDS"], 0] and int(got["pstate"][1]) == RAINBOW["ROUNDS"]


def test_rainbow_loop_captured_against_the_reference(rainbow_ref):
    """An actor graph and an update graph replayed alternately, ``ql.epsilon`` and ``pr.beta`` set between replays, the hand
    truncation and the event eagerly between two replays: every link of every round, then the final state."""
    check_final(run_loop(rainbow_ref, captured=True, check=True), rainbow_ref, "captured")


def test_rainbow_loop_eager_ends_in_the_references_state(rainbow_ref):
    """The same loop without graphs; only the final state is compared."""
    check_final(run_loop(rainbow_ref, captured=False, check=False), rainbow_ref, "eager")
