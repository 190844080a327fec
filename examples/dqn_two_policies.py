#!/usr/bin/env python3
"""The set-up of the reference's training script -- double DQN with two policies, "boarding" and "exiting" -- on this stack
(include/ccx.h: CCX_QLEARN, CCX_SIDES, CCX_ADAM).  The online and the target Q-networks are two `SideHeads`; the actor loop
is `online(obs)` -> `q_actions` with an annealed epsilon (a device scalar) -> `rollout(reset_obs="next", masks_out=)`.  A torch
ring holds env-steps ([R, N, L] rows, so `SideHeads` runs on what is drawn); the next state of a step that ended an episode
is its `final_obs` row, and its legal set is taken as "everything" (the masks the rollout wrote belong to the new episode).
The update is per side: `td_loss` -> `td_loss_backward` with `valid & side`, the two gradient arrays joined by a select,
`backward_into`, ONE `DeviceAdam`.  A minibatch update -- the index gather and every library launch -- is ONE captured graph;
the indices come from a seeded torch generator on the device; the target network is synchronised every TARGET_EVERY updates
with `torch._foreach_copy_`.  The whole run happens twice from the same seeds: the parameters end equal bit for bit."""

import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

import torch  # noqa: E402

from collectivecrossing_amd import BatchedCollectiveCrossing, CollectiveCrossingConfig, QLearning, SideHeads  # noqa: E402
from collectivecrossing_amd._abi import AF_LIVE, AF_TERMINATED, EF_RESET  # noqa: E402
from collectivecrossing_amd.qlearn import QActions  # noqa: E402
from collectivecrossing_amd.truncated_configs import MaxStepsTruncatedConfig  # noqa: E402

config = CollectiveCrossingConfig(
    width=12, height=8, division_y=4, tram_door_left=5, tram_door_right=7, tram_length=9,
    num_boarding_agents=5, num_exiting_agents=3, exiting_destination_area_y=0,
    boarding_destination_area_y=8, truncated_config=MaxStepsTruncatedConfig(max_steps=40))
SIDES = ("boarding", "exiting")
GAMMA, HUBER_DELTA, LR = 0.99, 1.0, 1e-3
EPS_START, EPS_END = 1.0, 0.05


def train(num_envs=1024, updates=300, ring_steps=64, batch=4096, warmup_steps=16, target_every=25, anneal_updates=200, hidden=64,
          seed=0, log_every=50, log=print):
    """`updates` minibatch updates (one actor step of `num_envs` envs before each) from fixed seeds; returns the online
    network's parameters, the optimiser's (taken, skipped) counts and the last TD statistics per side."""
    env = BatchedCollectiveCrossing(config, num_envs)
    stream = torch.cuda.Stream()
    env.use_stream(stream)                                           # a capture needs a stream of its own
    torch.cuda.synchronize()
    with torch.cuda.stream(stream), torch.no_grad():
        env.make_reset_pool(seed0=seed, size=4096)
        env.reset_from_pool()
        env.set_rng_seed(2024 + seed)
        env.track_episodes()
        E, N, L, dev = num_envs, env.num_agents, env.obs_len, env.device
        nb = config.num_boarding_agents
        torch.manual_seed(seed)
        online = SideHeads(env, {s: env.mlp_head(hidden) for s in SIDES})
        target = SideHeads(env, {s: env.mlp_head(hidden) for s in SIDES})
        target.load_state_dict(online.state_dict())
        ql = QLearning(env, epsilon=EPS_START)
        opt = env.adam(online.parameters(), lr=LR, max_grad_norm=10.0)
        side_of = [online.slot_mask(i) for i in range(len(SIDES))]    # u8 [N] each
        first_side = side_of[0].bool()
        gen = torch.Generator(device=dev)
        gen.manual_seed(seed)

        # ---- the replay ring: R env-steps of static shape
        R = ring_steps * E
        u8, f32 = torch.uint8, torch.float32
        ring = dict(obs=torch.zeros((R, N, L), device=dev), next_obs=torch.zeros((R, N, L), device=dev),
                    acts=torch.full((R, N), 255, dtype=u8, device=dev), reward=torch.zeros((R, N), dtype=torch.float64, device=dev),
                    done=torch.zeros((R, N), dtype=u8, device=dev), valid=torch.zeros((R, N), dtype=u8, device=dev),
                    masks_next=torch.full((R, N), 0x1F, dtype=u8, device=dev))

        # ---- the actor's static buffers
        traj = env.alloc_rollout(1, want_final=True)
        acts = torch.empty((1, E, N), dtype=u8, device=dev)
        chosen = QActions(acts[0], None)
        q_act = torch.empty((E, N, 5), device=dev)
        obs, masks = env.observe(), env.action_masks()
        everything = torch.tensor(0x1F, dtype=u8, device=dev)

        def actor_step(t):
            nonlocal obs
            at = (t % ring_steps) * E
            ring["obs"][at:at + E] = obs
            online(obs, out=q_act)
            ql.q_actions(q_act, masks, out=chosen)
            env.rollout(acts, auto_reset=True, reset_obs="next", out=traj, masks_out=masks)
            af = traj.agent_flags[0]
            reset = (traj.env_flags[0] & EF_RESET) != 0
            ring["acts"][at:at + E] = acts[0]
            ring["reward"][at:at + E] = traj.reward[0]
            ring["done"][at:at + E] = af & AF_TERMINATED
            ring["valid"][at:at + E] = af & AF_LIVE
            ring["next_obs"][at:at + E] = torch.where(reset[:, None, None], traj.final_obs[0], traj.obs[0])
            ring["masks_next"][at:at + E] = torch.where(reset[:, None], everything, masks)
            obs = traj.obs[0]

        # ---- the update's static buffers: a minibatch of `batch` env-steps, [batch, N, ...]
        lead = (batch, N)
        idx = torch.zeros((batch,), dtype=torch.int64, device=dev)
        mb = {k: torch.empty((batch,) + tuple(t.shape[1:]), dtype=t.dtype, device=dev) for k, t in ring.items()}
        valid_of = [torch.empty(lead, dtype=u8, device=dev) for _ in SIDES]
        q, hid = torch.empty(lead + (5,), device=dev), torch.empty(lead + (hidden,), device=dev)
        q_next_target, q_next_online = torch.empty(lead + (5,), device=dev), torch.empty(lead + (5,), device=dev)
        losses = [ql.alloc_td_loss(lead, want_td_error=False) for _ in SIDES]
        gq = torch.empty(lead + (5,), dtype=f32, device=dev)
        grads = online.alloc_backward(lead)
        flat = [t for o in grads for t in (o.w1t, o.b1, o.w2, o.b2)]

        def update():
            for k, t in ring.items():
                torch.index_select(t, 0, idx, out=mb[k])
            online(mb["obs"], out=q, hidden_out=hid)
            target(mb["next_obs"], out=q_next_target)
            online(mb["next_obs"], out=q_next_online)
            args = (q, mb["acts"], mb["reward"], mb["done"], q_next_target, q_next_online, mb["masks_next"])
            for side, valid, loss in zip(side_of, valid_of, losses):  # per side: its rows, its mean
                torch.mul(mb["valid"], side, out=valid)               # valid & side (0 / 4 times 0 / 1)
                ql.td_loss(*args, valid=valid, gamma=GAMMA, huber_delta=HUBER_DELTA, out=loss)
                ql.td_loss_backward(*args, valid=valid, gamma=GAMMA, huber_delta=HUBER_DELTA, stats=loss.stats, out=loss)
            torch.where(first_side[:, None], losses[0].grad_q, losses[1].grad_q, out=gq)   # a select: each side keeps its own bits
            online.backward_into(mb["obs"], hid, gq, out=grads)
            opt.step(grads=flat)

        for t in range(warmup_steps):
            actor_step(t)
        stream.synchronize()
        graph = torch.cuda.CUDAGraph()
        torch.randint(0, min(warmup_steps, ring_steps) * E, (batch,), generator=gen, out=idx)
        with torch.cuda.graph(graph, stream=stream):
            update()
        stream.synchronize()

        stats = env.episode_stats()
        for u in range(updates):
            t = warmup_steps + u
            ql.epsilon = max(EPS_END, EPS_START - (EPS_START - EPS_END) * u / max(1, anneal_updates))
            actor_step(t)
            filled = min(t + 1, ring_steps) * E
            torch.randint(0, filled, (batch,), generator=gen, out=idx)
            graph.replay()
            if (u + 1) % target_every == 0:
                torch._foreach_copy_(list(target.parameters()), list(online.parameters()))
            if log_every and (u + 1) % log_every == 0:
                stream.synchronize()
                done_envs = stats.finished > 0
                last = stats.last_ret[done_envs]
                per_side = [float(last[:, :nb].sum(1).mean()), float(last[:, nb:].sum(1).mean())] if bool(done_envs.any()) else [0.0, 0.0]
                log(f"update {u + 1:4d}: epsilon {ql.epsilon:.3f}, " + ", ".join(
                    f"{s}: return {r:8.3f} loss {float(l.loss):.4f} |td| {float(l.mean_abs_td):.4f}" for s, r, l in zip(SIDES, per_side, losses))
                    + f", {int(stats.finished.sum())} episodes")
        stream.synchronize()
        params = [p.detach().clone() for p in opt.params]
        last_stats, counts = [l.stats.tolist() for l in losses], opt.counts()
    env.use_stream(None)
    env.close()
    return params, counts, last_stats


def same_bits(a, b) -> bool:
    return all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(a, b))


if __name__ == "__main__":
    first, counts, stats = train()
    second, counts2, _ = train(log=lambda *_: None)
    for side, st in zip(SIDES, stats):
        print(f"{side}, last minibatch: loss {st[0]:.4f}, mean |td| {st[1]:.4f}, mean Q taken {st[2]:.3f}, mean target {st[3]:.3f}, "
              f"{int(st[6])} agent-steps, {int(st[7])} bad actions")
    print(f"optimiser steps on the device: {counts[0]} taken, {counts[1]} skipped")
    assert counts == counts2 and all(torch.isfinite(p).all() for p in first)
    same = same_bits(first, second)
    print(f"two runs from the same seeds: the {sum(p.numel() for p in first)} parameters are {'equal bit for bit' if same else 'DIFFERENT'}")
    assert same, "the run is pinned by its seeds: the draws, the gather, the loss, the backward pass and the optimiser step"
