#!/usr/bin/env python3
"""An actor in the loop without torch glue between the network and the step: `sample_actions` turns the policy's logits
and the step's own legal-action masks into the action tensor `rollout` reads and the `log pi(a|s)` a PPO update needs later
(`logp_old`), in one kernel -- eagerly, and with the whole loop body captured once into a HIP graph and replayed per step.
The draw is keyed by (global env, episode, step of the episode, agent slot) and `set_rng_seed`: eager and captured runs from
the same state take the same actions, and so would any sharding of the batch."""

import sys
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

import torch  # noqa: E402

from collectivecrossing_amd import BatchedCollectiveCrossing, CollectiveCrossingConfig, SampleResult  # noqa: E402
from collectivecrossing_amd.truncated_configs import MaxStepsTruncatedConfig  # noqa: E402

config = CollectiveCrossingConfig(
    width=12, height=8, division_y=4, tram_door_left=5, tram_door_right=7, tram_length=9,
    num_boarding_agents=5, num_exiting_agents=3, exiting_destination_area_y=0,
    boarding_destination_area_y=8, truncated_config=MaxStepsTruncatedConfig(max_steps=100))
E, STEPS = 4096, 300
env = BatchedCollectiveCrossing(config, E)
dev = env.device
N, L = env.num_agents, env.obs_len
env.make_reset_pool(seed0=0, size=8192)
env.reset_from_pool()
env.set_rng_seed(2024)

torch.manual_seed(0)
policy = torch.nn.Sequential(torch.nn.Linear(L, 64), torch.nn.Tanh(), torch.nn.Linear(64, 5)).to(dev)
side = torch.cuda.Stream(device=dev)
env.use_stream(side)                             # bind the env to the stream BEFORE capturing on it

with torch.cuda.stream(side), torch.no_grad():
    obs = env.observe()                                               # f32 [E, N, L]
    masks = env.action_masks()                                        # u8 [E, N]: the legal actions of the reset state
    actions = torch.empty((1, E, N), dtype=torch.uint8, device=dev)   # what rollout reads ...
    logp_old = torch.empty((E, N), dtype=torch.float32, device=dev)
    sampled = SampleResult(actions[0], logp_old, None)                # ... is what sample_actions writes
    out = env.alloc_rollout(1)
    wasted = torch.zeros((), dtype=torch.int64, device=dev)           # moves asked for that the mask calls no-ops

    def body():
        env.sample_actions(policy(obs), masks, out=sampled)           # one kernel: actions (255 for finished agents) + logp_old
        live = actions[0] != 255
        bit = (masks >> actions[0].clamp(max=4)) & 1
        wasted.add_((live & (bit == 0)).sum())
        # reset_obs="next": the rows of a restarted env are those of its NEW episode, the state the masks describe
        env.rollout(actions, auto_reset=True, out=out, masks_out=masks, reset_obs="next")
        obs.copy_(out.obs[0])

    start = env.get_state()
    body()                                                            # warm-up (allocations)
    side.synchronize()
    first_eager = actions.clone()
    t0 = time.perf_counter()
    for _ in range(STEPS):
        body()
    side.synchronize()
    eager = (time.perf_counter() - t0) / STEPS

    env.set_state(**start)                                            # back to the start: the captured loop repeats the eager one
    env.observe(out=obs)
    env.action_masks(out=masks)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        body()
    side.synchronize()
    graph.replay()
    side.synchronize()
    same = bool((actions == first_eager).all())
    env.zero_counters()
    t0 = time.perf_counter()
    for _ in range(STEPS):
        graph.replay()
    side.synchronize()
    replay = (time.perf_counter() - t0) / STEPS
    c = env.counters()
    mean_logp = float(logp_old.sum() / (actions[0] != 255).sum().clamp(min=1))

assert int(wasted) == 0, "a masked policy never asks for a move the mask rules out"
assert same, "the captured loop takes the eager loop's actions"
moving = c["moves"] / max(1, c["live_agent_steps"])
print(f"{E} envs, sampled network policy in the loop: eager {eager * 1e6:.1f} us/step, HIP graph {replay * 1e6:.1f} us/step "
      f"({E / replay:.3e} env-steps/s); {c['episodes']} episodes restarted; {moving:.0%} of the live agent-steps moved; "
      f"mean log pi(a|s) of the last step {mean_logp:.3f}; first captured step = first eager step: {same}")
env.close()
