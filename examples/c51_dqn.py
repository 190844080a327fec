#!/usr/bin/env python3
"""A short categorical (C51) double-DQN loop on one batch (include/ccx.h: CCX_C51).  The network is torch's --
`Linear(L, 64) -> Tanh -> Linear(64, 5 * A)`, online and target -- and everything around it runs on the device through the
library: `CategoricalQ.q_values` turns the actor's atom logits into expected values, `QLearning.q_actions` chooses from them,
the replay memory is a `ReplayRing`, and the update is `CategoricalQ.loss`, whose `loss.backward()` reaches the logits through
`ccx_c51_loss_backward`.  `stats` is printed per logged update.

At the end, on one fixed minibatch: two calls of `loss` + `loss_backward` give equal bits, while the textbook composition in
torch -- floor / ceil and two `index_add_`, floating-point atomics in no fixed order -- need not (whether it did is printed,
not asserted)."""

import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

import torch  # noqa: E402

from collectivecrossing_amd import (BatchedCollectiveCrossing, CategoricalQ, CollectiveCrossingConfig, QLearning,  # noqa: E402
                                    ReplayRing)
from collectivecrossing_amd.qlearn import QActions  # noqa: E402
from collectivecrossing_amd.truncated_configs import MaxStepsTruncatedConfig  # noqa: E402

config = CollectiveCrossingConfig(
    width=12, height=8, division_y=4, tram_door_left=5, tram_door_right=7, tram_length=9,
    num_boarding_agents=5, num_exiting_agents=3, exiting_destination_area_y=0,
    boarding_destination_area_y=8, truncated_config=MaxStepsTruncatedConfig(max_steps=40))
GAMMA, LR = 0.99, 1e-3
VMIN, VMAX = -10.0, 10.0
EPS_START, EPS_END = 1.0, 0.05


def compact_of_rows(rows):
    """Compact records [E, N, 4] of DefaultObservation rows [E, N, L] (N >= 2), as examples/dqn_replay_ring.py makes them."""
    N = rows.shape[-2]
    return torch.stack([rows[:, 1, 6:10]] + [rows[:, 0, 6 + 4 * j:10 + 4 * j] for j in range(1, N)], dim=1).contiguous()


def torch_c51_loss(logits, actions, reward, done, next_target, next_online, masks_next, valid, support, gamma, vmin=VMIN, vmax=VMAX):
    """The textbook in torch on the same arrays: softmax, expected values, masked argmax, gather, floor / ceil with
    `index_add_`, log_softmax, a mean over `valid`.  Returns (loss, proj).  (Nothing here waits for the device: the
    composition captures into a graph, which profiles/c51_timing.py does.)"""
    A = support.numel()
    dz = (vmax - vmin) / (A - 1)
    lead = actions.shape
    rows = actions.numel()
    each = torch.arange(rows, device=logits.device)
    legal = ((masks_next.reshape(rows, 1).int() | 0x10) >> torch.arange(5, device=logits.device)) & 1
    q_sel = (torch.softmax(next_online.reshape(rows, 5, A), -1) * support).sum(-1).masked_fill(legal == 0, float("-inf"))
    kstar = q_sel.argmax(-1)
    p = torch.softmax(next_target.reshape(rows, 5, A)[each, kstar], -1)
    live = (done.reshape(rows, 1) == 0).float()
    t = (reward.reshape(rows, 1).float() + live * gamma * support).clamp(vmin, vmax)
    b = ((t - vmin) / dz).clamp(0, A - 1)
    lo, hi = b.floor().long(), b.ceil().long()
    offset = (each * A).unsqueeze(1)
    proj = torch.zeros(rows * A, device=logits.device)
    proj.index_add_(0, (lo + offset).reshape(-1), (p * (hi.float() - b + (lo == hi).float())).reshape(-1))
    proj.index_add_(0, (hi + offset).reshape(-1), (p * (b - lo.float())).reshape(-1))
    proj = proj.view(rows, A)
    a = actions.reshape(rows).long().clamp(max=4)
    logp = torch.log_softmax(logits.reshape(rows, 5, A)[each, a], -1)
    counts = (valid.reshape(rows) != 0) & (actions.reshape(rows) <= 4)
    ce = -(proj * logp).sum(-1)
    loss = torch.where(counts, ce, torch.zeros_like(ce)).sum() / counts.sum()
    proj = torch.where(counts[:, None], proj, torch.zeros_like(proj))    # (the library writes +0.0 where a row does not count)
    return loss, proj.view(lead + (A,))


def train(num_envs=256, updates=100, ring_steps=32, batch=512, warmup_steps=8, target_every=20, anneal_updates=60, atoms=51,
          hidden=64, seed=0, log_every=10, log=print):
    """`updates` minibatch updates (one actor step of `num_envs` envs before each) from fixed seeds; returns the `stats` of
    every update and (ours equal, torch's equal): whether two evaluations of the loss and its gradient on one fixed minibatch
    gave equal bits, through the library and through the torch composition."""
    env = BatchedCollectiveCrossing(config, num_envs)
    stream = torch.cuda.Stream()
    env.use_stream(stream)
    torch.cuda.synchronize()
    all_stats = []
    with torch.cuda.stream(stream):
        env.make_reset_pool(seed0=seed, size=4096)
        env.reset_from_pool()
        env.set_rng_seed(2024 + seed)                                # the epsilon-greedy draws AND the replay draws
        E, N, A, dev = num_envs, env.num_agents, atoms, env.device
        torch.manual_seed(seed)

        def net():
            return torch.nn.Sequential(torch.nn.Linear(env.obs_len, hidden), torch.nn.Tanh(), torch.nn.Linear(hidden, 5 * A)).to(dev)
        online, target = net(), net()
        target.load_state_dict(online.state_dict())
        cq = CategoricalQ(env, atoms=A, vmin=VMIN, vmax=VMAX)
        ql = QLearning(env, epsilon=EPS_START)
        opt = torch.optim.Adam(online.parameters(), lr=LR)
        ring = ReplayRing(env, steps=ring_steps)

        traj = env.alloc_rollout(1, want_obs=False, want_compact=True, want_final=True)
        acts = torch.empty((1, E, N), dtype=torch.uint8, device=dev)
        chosen = QActions(acts[0], None)
        q_act = torch.empty((E, N, 5), device=dev)
        obs, masks = env.observe(), env.action_masks()
        masks_next = masks.view(1, E, N)                             # behind the rollout: the legal set of the NEXT state
        obs_c = compact_of_rows(obs)
        mb = ring.alloc_batch(batch)

        def actor_step():
            with torch.no_grad():
                env.observe(out=obs)
                cq.q_values(online(obs).view(E, N, 5, A), out=q_act)  # atom logits -> expected values
                ql.q_actions(q_act, masks, out=chosen)               # ... -> epsilon-greedy actions over the legal set
                env.rollout(acts, auto_reset=True, reset_obs="next", out=traj, want_obs=False, want_compact=True, masks_out=masks)
                ring.push(obs_c, acts, traj, masks_next=masks_next)
                obs_c.copy_(traj.obs_compact[0])

        def next_logits():
            with torch.no_grad():
                return target(mb.next_obs).view(batch, N, 5, A), online(mb.next_obs).view(batch, N, 5, A)

        for _ in range(warmup_steps):
            actor_step()
        for u in range(updates):
            ql.epsilon = max(EPS_END, EPS_START - (EPS_START - EPS_END) * u / max(1, anneal_updates))
            actor_step()
            ring.sample(batch, out=mb)
            nt, no = next_logits()
            logits = online(mb.obs).view(batch, N, 5, A)
            r = cq.loss(logits, mb.actions, mb.reward, mb.done, nt, no, mb.masks_next, valid=mb.valid, gamma=GAMMA)
            opt.zero_grad(set_to_none=True)
            r.loss.backward()                                        # ccx_c51_loss_backward, then torch's own backward of the net
            opt.step()
            if (u + 1) % target_every == 0:
                target.load_state_dict(online.state_dict())
            stream.synchronize()
            all_stats.append(r.stats.tolist())
            if log_every and (u + 1) % log_every == 0:
                st = all_stats[-1]
                log(f"update {u + 1:4d}: epsilon {ql.epsilon:.3f}, loss {st[0]:.4f}, mean ce {st[1]:.4f}, mean Q taken {st[2]:.3f}, "
                    f"mean target {st[3]:.3f}, {int(st[6])} agent-steps, {int(st[7])} bad actions")

        # ---- one fixed minibatch, evaluated twice each way
        nt, no = next_logits()
        with torch.no_grad():
            logits = online(mb.obs).view(batch, N, 5, A).contiguous()
        ours = []
        for _ in range(2):
            out = cq.alloc_loss((batch, N))
            cq.loss(logits, mb.actions, mb.reward, mb.done, nt, no, mb.masks_next, valid=mb.valid, gamma=GAMMA, out=out)
            cq.loss_backward(logits, mb.actions, out.proj, valid=mb.valid, stats=out.stats, out=out)
            ours.append((out.stats, out.row_loss, out.proj, out.grad_logits))
        theirs = []
        for _ in range(2):
            x = logits.clone().requires_grad_()
            loss, proj = torch_c51_loss(x, mb.actions, mb.reward, mb.done, nt, no, mb.masks_next, mb.valid, cq.support, GAMMA)
            (g,) = torch.autograd.grad(loss, x)
            theirs.append((loss.detach().reshape(1), proj.detach(), g))
        stream.synchronize()
        ours_equal, theirs_equal = same_bits(*ours), same_bits(*theirs)
        close = float((ours[0][2] - theirs[0][1]).abs().max())
    env.use_stream(None)
    env.close()
    return all_stats, (ours_equal, theirs_equal, close)


def same_bits(a, b) -> bool:
    return all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(a, b))


if __name__ == "__main__":
    stats, (ours_equal, theirs_equal, close) = train()
    print(f"one fixed minibatch, loss + loss_backward twice: stats, row_loss, proj and grad_logits are "
          f"{'equal bit for bit' if ours_equal else 'DIFFERENT'}")
    print(f"the torch composition with index_add_, twice: loss, proj and gradient are "
          f"{'equal bit for bit this time' if theirs_equal else 'different in some bits'} (nothing fixes the order of its atomic additions); "
          f"its projection lies within {close:.2e} of the library's")
    assert ours_equal and all(all(map(lambda v: v == v, s)) for s in stats)
