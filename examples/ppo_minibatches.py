#!/usr/bin/env python3
"""The iteration of ppo_device_update.py with the minibatches drawn on the device too (include/ccx.h: CCX_MINIBATCH): the
gather sits INSIDE the captured update, so a minibatch update is ONE graph -- `RolloutMinibatches.next`, both heads' forward,
`ppo_loss`, `ppo_loss_backward`, two `mlp_backward(out=)` and `opt.step(grads=)` -- and replaying it EPOCHS x
minibatches_per_epoch times walks through the shuffled env-steps of every epoch by itself: no `randperm`, no `index_select`,
no host work between replays.  The shuffle is over the K * E env-steps, not over whole steps, and it comes from
`set_rng_seed`: nothing in the iteration is left to torch's generator but the initial weights.  `obs0=` makes the gather
pick the row each step ACTED ON out of the rollout's own `obs`, so the collect loop keeps no second copy of every row.
The whole iteration runs twice from the same seeds; the parameters and the optimiser's m and v are equal bit for bit.  That
every link of it is the written rule, not only that two runs agree, is what tests/test_gpu_ppo_minibatch_chain.py checks: the
same calls at small shapes, with a last minibatch that is partly empty, against the per-op specs composed on the CPU."""

import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

import torch  # noqa: E402

from collectivecrossing_amd import (BatchedCollectiveCrossing, CollectiveCrossingConfig, RolloutMinibatches,  # noqa: E402
                                    SampleResult)
from collectivecrossing_amd._abi import EF_RESET  # noqa: E402
from collectivecrossing_amd.batched import RolloutResult  # noqa: E402
from collectivecrossing_amd.truncated_configs import MaxStepsTruncatedConfig  # noqa: E402

config = CollectiveCrossingConfig(
    width=12, height=8, division_y=4, tram_door_left=5, tram_door_right=7, tram_length=9,
    num_boarding_agents=5, num_exiting_agents=3, exiting_destination_area_y=0,
    boarding_destination_area_y=8, truncated_config=MaxStepsTruncatedConfig(max_steps=40))
E, K, EPOCHS, MINIBATCHES = 1024, 64, 3, 4
HYPER = dict(clip=0.2, vf_coef=0.5, ent_coef=0.01)


def iteration():
    """One PPO iteration from fixed seeds; returns (parameters, m, v) of actor and critic, the last stats, the optimiser's
    counts, the number of clipped steps and the minibatch state."""
    env = BatchedCollectiveCrossing(config, E)
    side = torch.cuda.Stream()
    env.use_stream(side)                                             # a capture needs a stream of its own
    torch.cuda.synchronize()
    with torch.cuda.stream(side), torch.no_grad():
        env.make_reset_pool(seed0=0, size=4096)
        env.reset_from_pool()
        env.set_rng_seed(2024)
        N = env.num_agents
        torch.manual_seed(0)
        actor = env.mlp_head(64)
        critic = env.mlp_head(64, O=1)
        opt = env.adam([*actor.parameters(), *critic.parameters()], lr=3e-4, max_grad_norm=0.5)

        # ---- collect: traj.obs[s] is the row BEHIND step s; the one step 0 acted on is kept once
        traj = env.alloc_rollout(K, want_final=True)
        acts = torch.empty((K, E, N), dtype=torch.uint8, device=env.device)
        logp_old = torch.empty((K, E, N), device=env.device)
        masks_old = torch.empty((K, E, N), dtype=torch.uint8, device=env.device)
        obs0, masks = env.observe().clone(), env.action_masks()
        obs = obs0
        for s in range(K):
            masks_old[s] = masks
            env.mlp_sample_actions(actor, obs, masks, out=SampleResult(acts[s], logp_old[s], None))
            slab = RolloutResult(**{k: None if t is None else t[s:s + 1] for k, t in vars(traj).items()})
            obs = env.rollout(acts[s:s + 1], auto_reset=True, reset_obs="next", out=slab, masks_out=masks).obs[0]

        # ---- values and advantages
        values = torch.empty((K, E, N), device=env.device)
        values[0] = critic(obs0).squeeze(-1)
        values[1:] = critic(traj.obs[:K - 1]).squeeze(-1)
        last_values = critic(traj.obs[K - 1]).squeeze(-1).contiguous()
        reset = (traj.env_flags & EF_RESET) != 0
        final_values = torch.zeros((K, E, N), device=env.device)
        final_values[reset] = critic(traj.final_obs[reset].contiguous()).squeeze(-1)
        gae = env.compute_gae(traj, values, last_values, final_values, gamma=0.99, lam=0.95)
        norm = env.masked_moments(gae.advantages, gae.valid)

        # ---- the update's static buffers: a minibatch of K * E / MINIBATCHES env-steps, [B, N, ...]
        mb = RolloutMinibatches(env, num_steps=K, batch_size=K * E // MINIBATCHES)
        mb.set_source(traj.obs, acts, logp_old, gae.advantages, gae.returns, masks=masks_old, valid=gae.valid, obs0=obs0)
        batch = mb.alloc()
        lead = (mb.batch_size, N)
        logits, hid_a = torch.empty(lead + (5,), device=env.device), torch.empty(lead + (64,), device=env.device)
        vals, hid_c = torch.empty(lead + (1,), device=env.device), torch.empty(lead + (64,), device=env.device)
        loss = env.alloc_ppo_loss(lead)
        ga, gc = env.alloc_mlp_backward(actor, lead), env.alloc_mlp_backward(critic, lead)
        grads = [ga.w1t, ga.b1, ga.w2, ga.b2, gc.w1t, gc.b1, gc.w2, gc.b2]

        def update():                                                # library launches only, the gather included
            mb.next(out=batch)
            actor(batch.obs, out=logits, hidden_out=hid_a)
            critic(batch.obs, out=vals, hidden_out=hid_c)
            args = (logits, vals.squeeze(-1), batch.actions, batch.logp, batch.advantages, batch.returns)
            kw = dict(masks=batch.masks, valid=batch.valid, norm=norm, **HYPER)
            env.ppo_loss(*args, **kw, out=loss)
            gl, gv = env.ppo_loss_backward(*args, **kw, stats=loss.stats, out=loss)
            env.mlp_backward(actor, batch.obs, hid_a, gl, out=ga)
            env.mlp_backward(critic, batch.obs, hid_c, gv.unsqueeze(-1), out=gc)
            opt.step(grads=grads)

        side.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            update()

        # ---- the update: ONE replay per minibatch; the state on the device walks through minibatches and epochs
        clipped = torch.zeros((), dtype=torch.int64, device=env.device)
        for _ in range(EPOCHS * mb.minibatches_per_epoch):
            graph.replay()
            clipped += opt.scale < 1.0
        side.synchronize()
        out = ([p.detach().clone() for p in opt.params], [t.clone() for t in opt.m], [t.clone() for t in opt.v])
        stats, counts, clipped, state = loss.stats.tolist(), opt.counts(), int(clipped), mb.state.tolist()
    env.use_stream(None)
    env.close()
    return out, stats, counts, clipped, state


first, stats, counts, clipped, state = iteration()
second, _, _, clipped2, state2 = iteration()
loss, policy, value, entropy, kl, cf, n, _ = stats
print(f"after {EPOCHS} epochs x {MINIBATCHES} minibatches of {K * E // MINIBATCHES} shuffled env-steps, each ONE replayed graph: loss {loss:.4f} "
      f"(policy {policy:.4f}, value {value:.4f}, entropy {entropy:.4f}, approx_kl {kl:.5f}, clip_frac {cf:.3f}, {int(n)} agent-steps in "
      f"the last minibatch)")
print(f"optimiser steps on the device: {counts[0]} taken, {counts[1]} skipped, {clipped} clipped at max_grad_norm = 0.5; "
      f"minibatch state on the device: epoch {state[0]}, cursor {state[1]}")
assert counts == (EPOCHS * MINIBATCHES, 0) and clipped == clipped2
assert state == state2 == [EPOCHS, 0, 0, 0]
assert all(torch.isfinite(t).all() for group in first for t in group)
for name, a, b in zip(("parameters", "m", "v"), first, second):
    same = all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(a, b))
    print(f"two runs from the same seeds: the {sum(t.numel() for t in a)} values of {name} are {'equal bit for bit' if same else 'DIFFERENT'}")
    assert same, "the update is pinned by its seeds, the minibatch draw and the optimiser step included"
