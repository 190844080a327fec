#!/usr/bin/env python3
"""The loop of examples/c51_dqn.py with the network on the device too (include/ccx.h: CCX_MLP_WIDE).  Online and target are
`CategoricalQ.head(64)`: a `WideMlpHead` with 5 * A outputs shaped [5, A], forward in one launch, `backward="device"` so that
`loss.backward()` reaches the four parameter tensors through `ccx_c51_loss_backward` and `ccx_mlp_wide_backward`, and the step
is `DeviceAdam`.  With that every link from the observation rows to the new parameters follows a written rule.

At the end, on one fixed minibatch and one fixed set of parameters: two evaluations of one whole update -- heads, loss, both
backward passes, the Adam step on a copy of the parameters -- give equal bits, the network included."""

import copy
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

import torch  # noqa: E402

from collectivecrossing_amd import BatchedCollectiveCrossing, CategoricalQ, DeviceAdam, QLearning, ReplayRing  # noqa: E402
from collectivecrossing_amd.qlearn import QActions  # noqa: E402

sys.path.insert(0, str(Path(__file__).resolve().parent))
from c51_dqn import EPS_END, EPS_START, GAMMA, LR, VMAX, VMIN, compact_of_rows, config, same_bits  # noqa: E402


def train(num_envs=256, updates=100, ring_steps=32, batch=512, warmup_steps=8, target_every=20, anneal_updates=60, atoms=51,
          hidden=64, seed=0, log_every=10, log=print):
    """`updates` minibatch updates (one actor step of `num_envs` envs before each) from fixed seeds; returns the `stats` of
    every update and whether two evaluations of one whole update from the same parameters gave equal bits."""
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
        cq = CategoricalQ(env, atoms=A, vmin=VMIN, vmax=VMAX)
        online, target = cq.head(hidden, backward="device"), cq.head(hidden)
        target.load_state_dict(online.state_dict())
        ql = QLearning(env, epsilon=EPS_START)
        opt = DeviceAdam(env, online.parameters(), lr=LR)
        ring = ReplayRing(env, steps=ring_steps)

        traj = env.alloc_rollout(1, want_obs=False, want_compact=True, want_final=True)
        acts = torch.empty((1, E, N), dtype=torch.uint8, device=dev)
        chosen = QActions(acts[0], None)
        q_act = torch.empty((E, N, 5), device=dev)
        logits_act = torch.empty((E, N, 5, A), device=dev)
        obs, masks = env.observe(), env.action_masks()
        masks_next = masks.view(1, E, N)                             # behind the rollout: the legal set of the NEXT state
        obs_c = compact_of_rows(obs)
        mb = ring.alloc_batch(batch)

        def actor_step():
            with torch.no_grad():
                env.observe(out=obs)
                cq.q_values(online(obs, out=logits_act), out=q_act)  # rows -> atom logits -> expected values
                ql.q_actions(q_act, masks, out=chosen)               # ... -> epsilon-greedy actions over the legal set
                env.rollout(acts, auto_reset=True, reset_obs="next", out=traj, want_obs=False, want_compact=True, masks_out=masks)
                ring.push(obs_c, acts, traj, masks_next=masks_next)
                obs_c.copy_(traj.obs_compact[0])

        def update(net, optimiser):
            """One whole update of `net` on the minibatch in `mb`; returns the loss result."""
            with torch.no_grad():
                nt, no = target(mb.next_obs), net(mb.next_obs)
            r = cq.loss(net(mb.obs), mb.actions, mb.reward, mb.done, nt, no, mb.masks_next, valid=mb.valid, gamma=GAMMA)
            optimiser.zero_grad(set_to_none=True)
            r.loss.backward()                                        # ccx_c51_loss_backward, then ccx_mlp_wide_backward
            optimiser.step()
            return r

        for _ in range(warmup_steps):
            actor_step()
        for u in range(updates):
            ql.epsilon = max(EPS_END, EPS_START - (EPS_START - EPS_END) * u / max(1, anneal_updates))
            actor_step()
            ring.sample(batch, out=mb)
            r = update(online, opt)
            if (u + 1) % target_every == 0:
                target.load_state_dict(online.state_dict())
            stream.synchronize()
            all_stats.append(r.stats.tolist())
            if log_every and (u + 1) % log_every == 0:
                st = all_stats[-1]
                log(f"update {u + 1:4d}: epsilon {ql.epsilon:.3f}, loss {st[0]:.4f}, mean ce {st[1]:.4f}, mean Q taken {st[2]:.3f}, "
                    f"mean target {st[3]:.3f}, {int(st[6])} agent-steps, {int(st[7])} bad actions")

        # ---- one fixed minibatch, one whole update from the same parameters, twice
        twice = []
        for _ in range(2):
            net = cq.head(hidden, backward="device")
            net.load_state_dict(copy.deepcopy(online.state_dict()))
            r = update(net, DeviceAdam(env, net.parameters(), lr=LR))
            twice.append([r.stats, r.proj] + [p.grad for p in net.parameters()] + [p.detach() for p in net.parameters()])
        stream.synchronize()
        equal = same_bits(*twice)
    env.use_stream(None)
    env.close()
    return all_stats, equal


if __name__ == "__main__":
    stats, equal = train()
    print(f"one fixed minibatch, one whole update twice (heads, loss, both backward passes, Adam): stats, proj, the four "
          f"gradients and the four new parameter tensors are {'equal bit for bit' if equal else 'DIFFERENT'}")
    assert equal and all(all(map(lambda v: v == v, s)) for s in stats)
