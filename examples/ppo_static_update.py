#!/usr/bin/env python3
"""The iteration of ppo_update.py with an update loop of static shapes: no boolean indexing, no `nonzero`, no host
synchronisation between `zero_grad()` and `opt.step()`.  `masked_moments` gives the advantages' mean and std over the valid
agent-steps once; every minibatch (whole steps, picked by `index_select` with a device index) goes through `ppo_loss`
(include/ccx.h: CCX_PPO_LOSS), which treats `valid` as a selection inside its kernels, reduces over the rows that count in a
fixed f64 tree, and is an autograd Function to both the logits and the values.  Every number of the loss is bit-defined.

Before the first optimiser step, on the same weights and the same logits, the ratio is exactly 1 on every row that counts:
the script prints `approx_kl` and `clip_frac` of the whole batch, and both are 0.  (That check evaluates the actor step by
step, on `[E, N, L]` inputs as the actor loop did: a matrix product of another shape may round its sums in another order.)"""

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
env = BatchedCollectiveCrossing(config, E)
env.make_reset_pool(seed0=0, size=4096)
env.reset_from_pool()
env.set_rng_seed(2024)
N, L = env.num_agents, env.obs_len
torch.manual_seed(0)
actor = torch.nn.Sequential(torch.nn.Linear(L, 64), torch.nn.Tanh(), torch.nn.Linear(64, 5)).to(env.device)
critic = torch.nn.Sequential(torch.nn.Linear(L, 64), torch.nn.Tanh(), torch.nn.Linear(64, 1)).to(env.device)
opt = torch.optim.Adam([*actor.parameters(), *critic.parameters()], lr=3e-4)

# ---- collect: as in ppo_update.py
traj = env.alloc_rollout(K, want_final=True)
acts = torch.empty((K, E, N), dtype=torch.uint8, device=env.device)
logp_old = torch.empty((K, E, N), device=env.device)
masks_old = torch.empty((K, E, N), dtype=torch.uint8, device=env.device)
rows = torch.empty((K, E, N, L), device=env.device)             # what each step acted on


def slab(s):
    """Step s of the trajectory buffers as a one-step result."""
    return RolloutResult(**{k: None if t is None else t[s:s + 1] for k, t in vars(traj).items()})


with torch.no_grad():
    obs = env.observe()
    masks = env.action_masks()
    for s in range(K):
        rows[s] = obs
        masks_old[s] = masks
        env.sample_actions(actor(obs), masks, out=SampleResult(acts[s], logp_old[s], None))
        obs = env.rollout(acts[s:s + 1], auto_reset=True, reset_obs="next", out=slab(s), masks_out=masks).obs[0]
    values = critic(rows).squeeze(-1).contiguous()
    last_values = critic(traj.obs[K - 1]).squeeze(-1).contiguous()
    reset = (traj.env_flags & EF_RESET) != 0
    final_values = torch.zeros((K, E, N), device=env.device)
    final_values[reset] = critic(traj.final_obs[reset]).squeeze(-1)
gae = env.compute_gae(traj, values, last_values, final_values, gamma=0.99, lam=0.95)

# ---- once per iteration: mean and std of the advantages over the valid agent-steps, on the device ([n, mean, std, 0])
norm = env.masked_moments(gae.advantages, gae.valid)

# ---- before the first optimiser step: the same weights, the same logits, the same distribution -> ratio exactly 1
with torch.no_grad():
    logits = torch.stack([actor(rows[s]) for s in range(K)])     # step by step, as the actor loop computed them
    first = env.ppo_loss(logits, values, acts, logp_old, gae.advantages, gae.returns, masks=masks_old, valid=gae.valid, norm=norm)
print(f"before the first update, over {int(first.count)} agent-steps that count: approx_kl {float(first.approx_kl):g}, "
      f"clip_frac {float(first.clip_frac):g}")
assert float(first.approx_kl) == 0.0 and float(first.clip_frac) == 0.0, "ppo_loss applies the distribution sample_actions drew from"

# ---- a few epochs of minibatches of whole steps: every shape is static, nothing below reads a value back to the host
history = []
for epoch in range(EPOCHS):
    for steps in torch.randperm(K, device=env.device).chunk(MINIBATCHES):
        pick = lambda t: t.index_select(0, steps)                # noqa: E731  [K / MINIBATCHES, E, N, ...], whatever `valid` holds
        obs_mb = pick(rows)
        r = env.ppo_loss(actor(obs_mb), critic(obs_mb).squeeze(-1), pick(acts), pick(logp_old), pick(gae.advantages),
                         pick(gae.returns), masks=pick(masks_old), valid=pick(gae.valid), norm=norm,
                         clip=0.2, vf_coef=0.5, ent_coef=0.01)
        opt.zero_grad()
        r.loss.backward()                                        # one kernel to the logits and the values, then torch's own
        opt.step()
    history.append(r.stats)                                      # a device tensor: printed after the loop
for epoch, stats in enumerate(history):
    loss, policy, value, entropy, kl, cf, n, _ = stats.tolist()
    print(f"epoch {epoch}: loss {loss:.4f} (policy {policy:.4f}, value {value:.4f}, entropy {entropy:.4f}, approx_kl {kl:.5f}, "
          f"clip_frac {cf:.3f}, {int(n)} agent-steps)")
assert all(torch.isfinite(p).all() for p in actor.parameters())
n_valid = int(norm[0])
print(f"{E} envs x {K} steps: {n_valid} of {gae.valid.numel()} agent-steps valid, {int(reset.sum())} restarts; "
      f"advantage mean {float(norm[1]):.4f}, std {float(norm[2]):.4f}")
env.close()
