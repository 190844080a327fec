#!/usr/bin/env python3
"""From a rollout to one policy-gradient step without leaving the GPU: a small torch actor and critic, a rollout with
same-step auto-reset observations (`reset_obs="next"` + `final_obs`), advantages and value targets from `compute_gae`
(include/ccx.h: CCX_GAE), and one masked PPO-style loss step.

Which value goes where: `values[s]` is the critic on the rows step s ACTED ON -- `observe()` before the rollout for step 0,
`obs[s - 1]` afterwards (in "next" mode those are already the new episode's rows where an env restarted); `last_values` is
the critic on `obs[K - 1]`; `final_values` is the critic on `final_obs`, the rows a finished episode ENDED ON, and only
the steps with `EF_RESET` have such rows.  Termination never bootstraps; truncation bootstraps from `final_values`."""

import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

import torch  # noqa: E402

from collectivecrossing_amd import BatchedCollectiveCrossing, CollectiveCrossingConfig  # noqa: E402
from collectivecrossing_amd._abi import EF_RESET  # noqa: E402
from collectivecrossing_amd.batched import RolloutResult  # noqa: E402
from collectivecrossing_amd.truncated_configs import MaxStepsTruncatedConfig  # noqa: E402

config = CollectiveCrossingConfig(
    width=12, height=8, division_y=4, tram_door_left=5, tram_door_right=7, tram_length=9,
    num_boarding_agents=5, num_exiting_agents=3, exiting_destination_area_y=0,
    boarding_destination_area_y=8, truncated_config=MaxStepsTruncatedConfig(max_steps=40))
E, K = 1024, 64
env = BatchedCollectiveCrossing(config, E)
env.make_reset_pool(seed0=0, size=4096)
env.reset_from_pool()
N, L = env.num_agents, env.obs_len
torch.manual_seed(0)
actor = torch.nn.Sequential(torch.nn.Linear(L, 64), torch.nn.Tanh(), torch.nn.Linear(64, 5)).to(env.device)
critic = torch.nn.Sequential(torch.nn.Linear(L, 64), torch.nn.Tanh(), torch.nn.Linear(64, 1)).to(env.device)
opt = torch.optim.Adam([*actor.parameters(), *critic.parameters()], lr=3e-4)

# ---- collect: the actor picks every step's actions from the rows the step before left (policy in the loop)
traj = env.alloc_rollout(K, want_final=True)
acts = torch.empty((K, E, N), dtype=torch.uint8, device=env.device)
logp_old = torch.empty((K, E, N), device=env.device)
rows = torch.empty((K, E, N, L), device=env.device)             # what each step acted on


def slab(s):
    """Step s of the trajectory buffers as a one-step result."""
    return RolloutResult(**{k: None if t is None else t[s:s + 1] for k, t in vars(traj).items()})


with torch.no_grad():
    obs = env.observe()
    for s in range(K):
        rows[s] = obs
        dist = torch.distributions.Categorical(logits=actor(obs))
        a = dist.sample()
        acts[s], logp_old[s] = a.to(torch.uint8), dist.log_prob(a)
        obs = env.rollout(acts[s:s + 1], auto_reset=True, reset_obs="next", out=slab(s)).obs[0]
    # ---- the critic's three inputs to compute_gae
    values = critic(rows).squeeze(-1).contiguous()               # values[0] from observe(), values[s] from obs[s - 1]
    last_values = critic(traj.obs[K - 1]).squeeze(-1).contiguous()
    reset = (traj.env_flags & EF_RESET) != 0                     # [K, E]: the only (s, e) whose final_obs rows were written
    final_values = torch.zeros((K, E, N), device=env.device)
    final_values[reset] = critic(traj.final_obs[reset]).squeeze(-1)
gae = env.compute_gae(traj, values, last_values, final_values, gamma=0.99, lam=0.95)
env.synchronize()

# ---- one masked PPO-style step: everything is averaged over the agent-steps that exist (valid = 1)
valid = gae.valid.bool()
adv = gae.advantages[valid]
adv_n = (adv - adv.mean()) / (adv.std() + 1e-8)
dist = torch.distributions.Categorical(logits=actor(rows[valid]))
ratio = torch.exp(dist.log_prob(acts[valid].long()) - logp_old[valid])
policy_loss = -torch.min(ratio * adv_n, ratio.clamp(0.8, 1.2) * adv_n).mean()
value_loss = (critic(rows[valid]).squeeze(-1) - gae.returns[valid]).pow(2).mean()
loss = policy_loss + 0.5 * value_loss - 0.01 * dist.entropy().mean()
opt.zero_grad()
loss.backward()
opt.step()
print(f"{E} envs x {K} steps: {int(valid.sum())} of {valid.numel()} agent-steps valid, {int(reset.sum())} restarts; "
      f"mean advantage {adv.mean():.4f}, mean return {gae.returns[valid].mean():.4f}; "
      f"loss {loss.item():.4f} (policy {policy_loss.item():.4f}, value {value_loss.item():.4f})")
env.close()
