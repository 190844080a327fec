#!/usr/bin/env python3
"""The update of mlp_policy.py with `backward="device"`: every link from the observation rows to the parameter gradients is
a written rule (include/ccx.h: CCX_MLP forward and backward, CCX_PPO_LOSS, CCX_GAE, CCX_SAMPLE), so a run is pinned by
its seeds.  The whole iteration -- collect, advantages, EPOCHS x MINIBATCHES optimiser steps -- runs twice from the same seeds,
and the parameters after all epochs are equal bit for bit."""

import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

import torch  # noqa: E402

from collectivecrossing_amd import BatchedCollectiveCrossing, CollectiveCrossingConfig, SampleResult  # noqa: E402
from collectivecrossing_amd._abi import EF_RESET  # noqa: E402
from collectivecrossing_amd.batched import RolloutResult  # noqa: E402
from collectivecrossing_amd.truncated_configs import MaxStepsTruncatedConfig  # noqa: E402

config = CollectiveCrossingConfig(
    width=12, height=8, division_y=4, tram_door_left=5, tram_door_right=7, tram_length=9,
    num_boarding_agents=5, num_exiting_agents=3, exiting_destination_area_y=0,
    boarding_destination_area_y=8, truncated_config=MaxStepsTruncatedConfig(max_steps=40))
E, K, EPOCHS, MINIBATCHES = 1024, 64, 3, 4


def iteration():
    """One PPO iteration from fixed seeds; returns the parameters of actor and critic and the last epoch's stats."""
    env = BatchedCollectiveCrossing(config, E)
    env.make_reset_pool(seed0=0, size=4096)
    env.reset_from_pool()
    env.set_rng_seed(2024)
    N, L = env.num_agents, env.obs_len
    torch.manual_seed(0)
    actor = env.mlp_head(64, backward="device")                  # the parameter gradients come from ccx_mlp_backward
    critic = env.mlp_head(64, O=1, backward="device")
    opt = torch.optim.Adam([*actor.parameters(), *critic.parameters()], lr=3e-4)

    # ---- collect
    traj = env.alloc_rollout(K, want_final=True)
    acts = torch.empty((K, E, N), dtype=torch.uint8, device=env.device)
    logp_old = torch.empty((K, E, N), device=env.device)
    masks_old = torch.empty((K, E, N), dtype=torch.uint8, device=env.device)
    rows = torch.empty((K, E, N, L), device=env.device)
    obs, masks = env.observe(), env.action_masks()
    for s in range(K):
        rows[s] = obs
        masks_old[s] = masks
        env.mlp_sample_actions(actor, obs, masks, out=SampleResult(acts[s], logp_old[s], None))
        slab = RolloutResult(**{k: None if t is None else t[s:s + 1] for k, t in vars(traj).items()})
        obs = env.rollout(acts[s:s + 1], auto_reset=True, reset_obs="next", out=slab, masks_out=masks).obs[0]

    # ---- values and advantages
    with torch.no_grad():
        values = critic(rows).squeeze(-1).contiguous()
        last_values = critic(traj.obs[K - 1]).squeeze(-1).contiguous()
        reset = (traj.env_flags & EF_RESET) != 0
        final_values = torch.zeros((K, E, N), device=env.device)
        final_values[reset] = critic(traj.final_obs[reset].contiguous()).squeeze(-1)
    gae = env.compute_gae(traj, values, last_values, final_values, gamma=0.99, lam=0.95)
    norm = env.masked_moments(gae.advantages, gae.valid)

    # ---- the update: minibatches of whole steps, [K / MINIBATCHES, E, N, L] each
    for epoch in range(EPOCHS):
        for steps in torch.randperm(K, device=env.device).chunk(MINIBATCHES):
            pick = lambda t: t.index_select(0, steps)            # noqa: E731
            obs_mb = pick(rows)
            r = env.ppo_loss(actor(obs_mb), critic(obs_mb).squeeze(-1), pick(acts), pick(logp_old), pick(gae.advantages),
                             pick(gae.returns), masks=pick(masks_old), valid=pick(gae.valid), norm=norm,
                             clip=0.2, vf_coef=0.5, ent_coef=0.01)
            opt.zero_grad()
            r.loss.backward()                                    # ppo_loss' kernel to the logits and values, then ccx_mlp_backward
            opt.step()
    env.synchronize()
    torch.cuda.synchronize()
    params = [p.detach().clone() for p in (*actor.parameters(), *critic.parameters())]
    stats = r.stats.tolist()
    env.close()
    return params, stats


first, stats = iteration()
second, _ = iteration()
loss, policy, value, entropy, kl, cf, n, _ = stats
print(f"after {EPOCHS} epochs x {MINIBATCHES} minibatches: loss {loss:.4f} (policy {policy:.4f}, value {value:.4f}, entropy {entropy:.4f}, "
      f"approx_kl {kl:.5f}, clip_frac {cf:.3f}, {int(n)} agent-steps in the last minibatch)")
assert all(torch.isfinite(p).all() for p in first)
same = all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(first, second))
print(f"two runs from the same seeds: the {sum(p.numel() for p in first)} parameters are "
      f"{'equal bit for bit' if same else 'DIFFERENT'}")
assert same, "with backward=\"device\" an update is pinned by its seeds"
