#!/usr/bin/env python3
"""How the episodes went, without leaving the GPU: a greedy auto-reset rollout with episode tracking on, then mean return
and episode length per side -- what the reference's demos print from `total_reward += reward` in their Python loop
(examples/waiting_policy_demo.py) and its training script logs as episode_return_min / mean / max.  The sums are the
reference's bit for bit: one f64 add per agent and step, in step order."""

import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

import numpy as np  # noqa: E402

from collectivecrossing_amd import BatchedCollectiveCrossing, CollectiveCrossingConfig  # noqa: E402
from collectivecrossing_amd.truncated_configs import MaxStepsTruncatedConfig  # noqa: E402

config = CollectiveCrossingConfig(
    width=12, height=8, division_y=4, tram_door_left=5, tram_door_right=7, tram_length=9,
    num_boarding_agents=5, num_exiting_agents=3, exiting_destination_area_y=0,
    boarding_destination_area_y=8, truncated_config=MaxStepsTruncatedConfig(max_steps=100))
E, K = 4096, 200
env = BatchedCollectiveCrossing(config, E)
env.make_reset_pool(seed0=0, size=8192)
env.reset_from_pool()
env.track_episodes(log_capacity=1 << 16)          # from here on every rollout / step feeds the statistics

env.rollout_greedy(K, auto_reset=True, want_obs=False)

stats = env.episode_stats()                        # zero-copy device views
env.synchronize()
nb = config.num_boarding_agents
print(f"{E} envs x {K} greedy steps: {int(stats.finished.sum())} finished episodes, "
      f"{int((stats.closed == 0).sum())} envs in the middle of one")
last = stats.last_ret[stats.finished > 0]          # [.., N]: the most recent finished episode of every env that has one
print(f"last finished episode per env: mean return boarding {last[:, :nb].mean():.3f}, exiting {last[:, nb:].mean():.3f}, "
      f"mean length {stats.last_steps[stats.finished > 0].float().mean():.1f} steps")

log = env.finished_episodes()                      # every stored record as NumPy arrays; clears the log
ended = {1: "terminated", 2: "truncated", 3: "terminated + truncated"}
print(f"log: {len(log)} records ({log.dropped} dropped)")
for name, cols in (("boarding", slice(0, nb)), ("exiting", slice(nb, None))):
    per_episode = log.ret[:, cols].sum(1)
    print(f"  {name:<9} return per episode (sum over the side): min {per_episode.min():.3f} mean {per_episode.mean():.3f} "
          f"max {per_episode.max():.3f}; live steps per agent {log.live_steps[:, cols].mean():.1f}")
print(f"  episode length: mean {log.steps.mean():.1f}, max {log.steps.max()}; "
      + ", ".join(f"{ended[k]} {int(v)}" for k, v in zip(*np.unique(log.end, return_counts=True))))
env.close()
