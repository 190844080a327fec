#!/usr/bin/env python3
"""The iteration of ppo_static_update.py with the library's own network between the observation rows and the logits:
`MlpHead` (include/ccx.h: CCX_MLP) as actor and critic.  The actor loop is two launches per step -- `mlp_sample_actions`
(rows -> actions, logp: one kernel) and `rollout` -- run eagerly, then once more from the same start as ONE captured graph
that repeats the eager run's actions.  The update runs on `[K / MINIBATCHES, E, N, L]` minibatches.

The logits of a row are a fixed sequence of f32 operations on that row, whatever batch it sits in.  So the check before the
first optimiser step needs no care about shapes: the whole batch goes through the actor in ONE `[K, E, N, L]` call, and
`approx_kl` and `clip_frac` are both 0 -- the ratio is exactly 1 on every row that counts."""

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
actor = env.mlp_head(64)                                         # Linear(L, 64) -> Tanh -> Linear(64, 5), parameters in the kernel's layout
critic = env.mlp_head(64, O=1)
opt = torch.optim.Adam([*actor.parameters(), *critic.parameters()], lr=3e-4)

# ---- collect: observation rows -> actions in one launch, then the step
traj = env.alloc_rollout(K, want_final=True)
acts = torch.empty((K, E, N), dtype=torch.uint8, device=env.device)
logp_old = torch.empty((K, E, N), device=env.device)
masks_old = torch.empty((K, E, N), dtype=torch.uint8, device=env.device)
rows = torch.empty((K, E, N, L), device=env.device)             # what each step acted on


def slab(s):
    """Step s of the trajectory buffers as a one-step result."""
    return RolloutResult(**{k: None if t is None else t[s:s + 1] for k, t in vars(traj).items()})


start = env.get_state()
obs = env.observe()
masks = env.action_masks()
for s in range(K):
    rows[s] = obs
    masks_old[s] = masks
    env.mlp_sample_actions(actor, obs, masks, out=SampleResult(acts[s], logp_old[s], None))
    obs = env.rollout(acts[s:s + 1], auto_reset=True, reset_obs="next", out=slab(s), masks_out=masks).obs[0]

# ---- the same actor loop as ONE captured graph of static buffers, replayed K times from the same start: the same actions
side = torch.cuda.Stream()
env.use_stream(side)
torch.cuda.synchronize()
with torch.cuda.stream(side):
    g_obs, g_masks = env.observe(), env.action_masks()
    g_acts = torch.empty((1, E, N), dtype=torch.uint8, device=env.device)
    g_out = env.alloc_rollout(1)
    g_sample = SampleResult(g_acts[0], torch.empty((E, N), device=env.device), None)
    replayed = torch.empty_like(acts)

    def actor_step():
        env.mlp_sample_actions(actor, g_obs, g_masks, out=g_sample)
        env.rollout(g_acts, auto_reset=True, reset_obs="next", out=g_out, masks_out=g_masks)
        g_obs.copy_(g_out.obs[0])

    side.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        actor_step()
    env.set_state(**start)                                       # (the capture itself ran nothing; start where the eager run started)
    env.observe(out=g_obs)
    env.action_masks(out=g_masks)
    for s in range(K):
        graph.replay()
        replayed[s].copy_(g_acts[0])
    side.synchronize()
env.use_stream(None)
same = bool((replayed == acts).all())
print(f"actor loop: {K} steps eager, then {K} replays of one captured graph (mlp_sample_actions -> rollout): "
      f"{'the same' if same else 'DIFFERENT'} actions")
assert same, "the captured actor loop repeats the eager run"

# ---- values and advantages
with torch.no_grad():
    values = critic(rows).squeeze(-1).contiguous()
    last_values = critic(traj.obs[K - 1]).squeeze(-1).contiguous()
    reset = (traj.env_flags & EF_RESET) != 0
    final_values = torch.zeros((K, E, N), device=env.device)
    final_values[reset] = critic(traj.final_obs[reset].contiguous()).squeeze(-1)
gae = env.compute_gae(traj, values, last_values, final_values, gamma=0.99, lam=0.95)
norm = env.masked_moments(gae.advantages, gae.valid)

# ---- before the first optimiser step: the whole batch in ONE [K, E, N, L] call -> ratio exactly 1
with torch.no_grad():
    first = env.ppo_loss(actor(rows), values, acts, logp_old, gae.advantages, gae.returns, masks=masks_old, valid=gae.valid, norm=norm)
print(f"before the first update, over {int(first.count)} agent-steps that count, one [K, E, N, L] call: "
      f"approx_kl {float(first.approx_kl):g}, clip_frac {float(first.clip_frac):g}")
assert float(first.approx_kl) == 0.0 and float(first.clip_frac) == 0.0, "MlpHead's logits do not depend on the batch a row sits in"

# ---- a few epochs of minibatches of whole steps, [K / MINIBATCHES, E, N, L] each
history = []
for epoch in range(EPOCHS):
    for steps in torch.randperm(K, device=env.device).chunk(MINIBATCHES):
        pick = lambda t: t.index_select(0, steps)                # noqa: E731
        obs_mb = pick(rows)
        r = env.ppo_loss(actor(obs_mb), critic(obs_mb).squeeze(-1), pick(acts), pick(logp_old), pick(gae.advantages),
                         pick(gae.returns), masks=pick(masks_old), valid=pick(gae.valid), norm=norm,
                         clip=0.2, vf_coef=0.5, ent_coef=0.01)
        opt.zero_grad()
        r.loss.backward()                                        # ppo_loss' kernel to the logits and values, then the heads' f32 backward
        opt.step()
    history.append(r.stats)
for epoch, stats in enumerate(history):
    loss, policy, value, entropy, kl, cf, n, _ = stats.tolist()
    print(f"epoch {epoch}: loss {loss:.4f} (policy {policy:.4f}, value {value:.4f}, entropy {entropy:.4f}, approx_kl {kl:.5f}, "
          f"clip_frac {cf:.3f}, {int(n)} agent-steps)")
assert all(torch.isfinite(p).all() for p in actor.parameters())
print(f"{E} envs x {K} steps: {int(norm[0])} of {gae.valid.numel()} agent-steps valid, {int(reset.sum())} restarts")
env.close()
