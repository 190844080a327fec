#!/usr/bin/env python3
"""The loop of examples/dqn_prioritized.py -- double DQN with two policies, proportional prioritised replay on the device --
with N-STEP TARGETS (include/ccx.h: CCX_NSTEP): `NStepReplay(ring, n=3)` sits under the priorities.  `pr.push` marks the
priorities AND the env-level cuts; `pr.sample(out=)` draws as before and fetches through the n-step ring: ONE kernel walks
each record forward through up to two successors in the ring and hands back the discounted 3-step reward, the state the
window ends on and, per row, the discount gamma^m its bootstrap takes -- `td_loss(discount=mb.discount)` reads it where it
read `gamma`.  With a reward of -1 per step, information now travels three steps per update.  No `index_select` chain, no
`where` over successors, nothing that knows `head` outside the library.  The whole run happens twice from the same seeds: the
parameters AND the leaves end equal bit for bit.  That every link of this loop (with dueling heads on top) is the written
rule, not only that two runs agree, is what tests/test_gpu_rainbow_chain.py checks against the composed CPU specs."""

import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

import torch  # noqa: E402

from collectivecrossing_amd import BatchedCollectiveCrossing, CollectiveCrossingConfig, NStepReplay, PrioritizedReplay, QLearning, ReplayRing, SideHeads  # noqa: E402
from collectivecrossing_amd.qlearn import QActions  # noqa: E402
from collectivecrossing_amd.truncated_configs import MaxStepsTruncatedConfig  # noqa: E402

config = CollectiveCrossingConfig(
    width=12, height=8, division_y=4, tram_door_left=5, tram_door_right=7, tram_length=9,
    num_boarding_agents=5, num_exiting_agents=3, exiting_destination_area_y=0,
    boarding_destination_area_y=8, truncated_config=MaxStepsTruncatedConfig(max_steps=40))
SIDES = ("boarding", "exiting")
GAMMA, N_STEP, HUBER_DELTA, LR = 0.99, 3, 1.0, 1e-3
EPS_START, EPS_END = 1.0, 0.05
ALPHA, BETA_START = 0.6, 0.4


def compact_of_rows(rows):
    """Compact records [E, N, 4] of DefaultObservation rows [E, N, L] (N >= 2): slot j >= 1 as row 0 sees it, slot 0 as row 1
    does.  Used once, for the state the first step acts on; from then on the rollout's own `obs_compact` is the record."""
    N = rows.shape[-2]
    return torch.stack([rows[:, 1, 6:10]] + [rows[:, 0, 6 + 4 * j:10 + 4 * j] for j in range(1, N)], dim=1).contiguous()


def train(num_envs=1024, updates=300, ring_steps=64, batch=4096, warmup_steps=16, target_every=25, anneal_updates=200, hidden=64,
          seed=0, log_every=50, log=print):
    """`updates` minibatch updates (one actor step of `num_envs` envs before each) from fixed seeds; returns the online
    network's parameters, the optimiser's (taken, skipped) counts, the last TD statistics per side, the leaves and
    ``pstate``."""
    env = BatchedCollectiveCrossing(config, num_envs)
    stream = torch.cuda.Stream()
    env.use_stream(stream)                                           # a capture needs a stream of its own
    torch.cuda.synchronize()
    with torch.cuda.stream(stream), torch.no_grad():
        env.make_reset_pool(seed0=seed, size=4096)
        env.reset_from_pool()
        env.set_rng_seed(2024 + seed)                                # the epsilon-greedy draws AND the prioritised draws
        E, N, dev = num_envs, env.num_agents, env.device
        nb = config.num_boarding_agents
        torch.manual_seed(seed)                                      # (the networks' initial parameters: the only use of torch's generator)
        online = SideHeads(env, {s: env.mlp_head(hidden) for s in SIDES})
        target = SideHeads(env, {s: env.mlp_head(hidden) for s in SIDES})
        target.load_state_dict(online.state_dict())
        ql = QLearning(env, epsilon=EPS_START)
        opt = env.adam(online.parameters(), lr=LR, max_grad_norm=10.0)
        side_of = [online.slot_mask(i) for i in range(len(SIDES))]    # u8 [N] each
        first_side = side_of[0].bool()
        ring = ReplayRing(env, steps=ring_steps)
        ns = NStepReplay(ring, n=N_STEP, gamma=GAMMA)
        pr = PrioritizedReplay(ns, alpha=ALPHA, beta=BETA_START)

        # ---- the actor's static buffers
        u8, f32 = torch.uint8, torch.float32
        traj = env.alloc_rollout(1, want_obs=False, want_compact=True, want_final=True)
        acts = torch.empty((1, E, N), dtype=u8, device=dev)
        chosen = QActions(acts[0], None)
        q_act = torch.empty((E, N, 5), device=dev)
        obs, masks = env.observe(), env.action_masks()
        masks_next = masks.view(1, E, N)                             # behind the rollout: the legal set of the NEXT state
        obs_c = compact_of_rows(obs)                                 # the compact record the next step acts on

        def actor_step():
            env.observe(out=obs)
            online(obs, out=q_act)
            ql.q_actions(q_act, masks, out=chosen)
            env.rollout(acts, auto_reset=True, reset_obs="next", out=traj, want_obs=False, want_compact=True, masks_out=masks)
            pr.push(obs_c, acts, traj, masks_next=masks_next)     # the ring's push, the cuts, and leaf = max_leaf at its slots
            obs_c.copy_(traj.obs_compact[0])

        # ---- the update's static buffers: a minibatch of `batch` env-steps, [batch, N, ...]
        lead = (batch, N)
        pmb = pr.alloc_batch(batch)
        mb, discount = pmb.batch.batch, pmb.batch.discount            # the n-step minibatch: records, and gamma^m per row
        valid_of = [torch.empty(lead, dtype=u8, device=dev) for _ in SIDES]
        q, hid = torch.empty(lead + (5,), device=dev), torch.empty(lead + (hidden,), device=dev)
        q_next_target, q_next_online = torch.empty(lead + (5,), device=dev), torch.empty(lead + (5,), device=dev)
        losses = [ql.alloc_td_loss(lead, want_td_error=True) for _ in SIDES]
        gq = torch.empty(lead + (5,), dtype=f32, device=dev)
        grads = online.alloc_backward(lead)
        flat = [t for o in grads for t in (o.w1t, o.b1, o.w2, o.b2)]

        def update():
            pr.sample(batch, out=pmb)                                # refresh the sums, draw, weights; then the n-step fetch
            online(mb.obs, out=q, hidden_out=hid)
            target(mb.next_obs, out=q_next_target)
            online(mb.next_obs, out=q_next_online)
            args = (q, mb.actions, mb.reward, mb.done, q_next_target, q_next_online, mb.masks_next)
            for side, valid, loss in zip(side_of, valid_of, losses):  # per side: its rows, its mean
                torch.mul(mb.valid, side, out=valid)                  # valid & side (0 / 4 times 0 / 1)
                ql.td_loss(*args, valid=valid, weights=pmb.weights, discount=discount, huber_delta=HUBER_DELTA, want_td_error=True, out=loss)
                ql.td_loss_backward(*args, valid=valid, weights=pmb.weights, discount=discount, huber_delta=HUBER_DELTA, stats=loss.stats,
                                    out=loss)
            torch.where(first_side[:, None], losses[0].grad_q, losses[1].grad_q, out=gq)   # a select: each side keeps its own bits
            online.backward_into(mb.obs, hid, gq, out=grads)
            opt.step(grads=flat)
            pr.update_priorities(mb.index, tuple(l.td_error for l in losses))   # +0.0 where a row is the other side's

        for _ in range(warmup_steps):
            actor_step()
        stream.synchronize()
        actor_graph, update_graph = torch.cuda.CUDAGraph(), torch.cuda.CUDAGraph()
        with torch.cuda.graph(actor_graph, stream=stream):
            actor_step()
        with torch.cuda.graph(update_graph, stream=stream):
            update()
        stream.synchronize()

        for u in range(updates):
            ql.epsilon = max(EPS_END, EPS_START - (EPS_START - EPS_END) * u / max(1, anneal_updates))
            pr.beta = min(1.0, BETA_START + (1.0 - BETA_START) * u / max(1, anneal_updates))
            actor_graph.replay()                                     # head is on the device: the push lands one step further
            update_graph.replay()                                    # draws is on the device: a fresh minibatch
            if (u + 1) % target_every == 0:
                torch._foreach_copy_(list(target.parameters()), list(online.parameters()))
            if log_every and (u + 1) % log_every == 0:
                stream.synchronize()
                head, (max_leaf, draws, total, min_leaf) = ring.state[0].item(), pr.pstate.tolist()
                log(f"update {u + 1:4d}: epsilon {ql.epsilon:.3f}, " + ", ".join(
                    f"{s}: loss {float(l.loss):.4f} |td| {float(l.mean_abs_td):.4f}" for s, l in zip(SIDES, losses))
                    + f", beta {pr.beta:.2f}, ring head {head}, draws {draws}, priorities {min_leaf / 65536:.4f} .. {max_leaf / 65536:.2f}")
        stream.synchronize()
        assert ring.state[:2].tolist() == [warmup_steps + updates, 0] and pr.pstate[1].item() == updates
        params = [p.detach().clone() for p in opt.params]
        last_stats, counts = [l.stats.tolist() for l in losses], opt.counts()
        leaves = (pr.leaf.clone(), pr.pstate.clone())
        spans = torch.bincount(pmb.batch.span[mb.valid != 0].flatten().long(), minlength=N_STEP + 1).tolist()
    env.use_stream(None)
    env.close()
    return params, counts, last_stats, leaves, spans


def same_bits(a, b) -> bool:
    return all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(a, b))


if __name__ == "__main__":
    first, counts, stats, (leaf, pstate), spans = train()
    second, counts2, _, (leaf2, pstate2), spans2 = train(log=lambda *_: None)
    for side, st in zip(SIDES, stats):
        print(f"{side}, last minibatch: loss {st[0]:.4f}, mean |td| {st[1]:.4f}, mean Q taken {st[2]:.3f}, mean target {st[3]:.3f}, "
              f"{int(st[6])} agent-steps, {int(st[7])} bad actions")
    print(f"optimiser steps on the device: {counts[0]} taken, {counts[1]} skipped")
    print(f"the priorities: {int((leaf > 0).sum())} of {leaf.numel()} records drawable, {leaf.unique().numel()} distinct leaves, "
          f"max_leaf {pstate[0].item() / 65536:.3f}")
    print(f"the last minibatch's live rows by span: " + ", ".join(f"{m} step{'s' * (m > 1)}: {c}" for m, c in enumerate(spans) if m))
    assert spans == spans2 and spans[N_STEP] > 0 and counts == counts2 and all(torch.isfinite(p).all() for p in first)
    same = same_bits(first, second) and torch.equal(leaf, leaf2) and torch.equal(pstate, pstate2)
    print(f"two runs from the same seeds: the {sum(p.numel() for p in first)} parameters and the {leaf.numel()} leaves are {'equal bit for bit' if same else 'DIFFERENT'}")
    assert same, "the run is pinned by its seeds: the draws, the windows, the weights, the loss, the optimiser step and the priorities"
