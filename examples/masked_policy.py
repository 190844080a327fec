#!/usr/bin/env python3
"""Invalid-action masking with a network in the loop: the step that advances 4096 envs also leaves, on the device, which
of its five actions would actually move each agent (`masks_out`: walls, the door row, the grid's edge and other active
agents turn the rest into silent no-ops).  The network's logits are masked with `logits.masked_fill(~mask, -inf)` before
sampling -- eagerly, and with the whole loop body captured once into a HIP graph and replayed per step.  A one-step
launch without a move order writes the masks itself (`masks_fused`): no second kernel."""

import sys
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

import torch  # noqa: E402

from collectivecrossing_amd import BatchedCollectiveCrossing, CollectiveCrossingConfig, unpack_action_masks  # noqa: E402
from collectivecrossing_amd.truncated_configs import MaxStepsTruncatedConfig  # noqa: E402

config = CollectiveCrossingConfig(
    width=12, height=8, division_y=4, tram_door_left=5, tram_door_right=7, tram_length=9,
    num_boarding_agents=5, num_exiting_agents=3, exiting_destination_area_y=0,
    boarding_destination_area_y=8, truncated_config=MaxStepsTruncatedConfig(max_steps=100))
E = 4096
env = BatchedCollectiveCrossing(config, E)
dev = env.device
N, L = env.num_agents, env.obs_len
env.make_reset_pool(seed0=0, size=8192)
env.reset_from_pool()

torch.manual_seed(0)
policy = torch.nn.Sequential(torch.nn.Linear(L, 64), torch.nn.Tanh(), torch.nn.Linear(64, 5)).to(dev)
side = torch.cuda.Stream(device=dev)
env.use_stream(side)                             # bind the env to the stream BEFORE capturing on it

with torch.cuda.stream(side), torch.no_grad():
    obs = env.observe()                                               # f32 [E, N, L]
    masks = env.action_masks()                                        # u8 [E, N]: the legal actions of the reset state
    actions = torch.empty((1, E, N), dtype=torch.uint8, device=dev)
    noise = torch.empty((E, N, 5), device=dev)
    out = env.alloc_rollout(1)
    wasted = torch.zeros((), dtype=torch.int64, device=dev)           # moves asked for that the mask calls no-ops

    def body():
        legal = unpack_action_masks(masks)                            # bool [E, N, 5], index = action id
        logits = policy(obs).masked_fill(~legal, float("-inf"))
        noise.exponential_()                                          # Gumbel-max sampling: graph-capturable
        actions[0].copy_((logits - noise.log()).argmax(-1).to(torch.uint8))
        wasted.add_((~legal.gather(-1, actions[0].long().unsqueeze(-1))).sum())
        # reset_obs="next": the rows of a restarted env are those of its NEW episode, the state the masks describe
        env.rollout(actions, auto_reset=True, out=out, masks_out=masks, reset_obs="next")   # masks of the NEW state, after restarts
        obs.copy_(out.obs[0])

    body()                                                            # warm-up (allocations)
    side.synchronize()
    t0 = time.perf_counter()
    for _ in range(300):
        body()
    side.synchronize()
    eager = (time.perf_counter() - t0) / 300

    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        body()
    side.synchronize()
    env.zero_counters()
    t0 = time.perf_counter()
    for _ in range(300):
        graph.replay()
    side.synchronize()
    replay = (time.perf_counter() - t0) / 300
    c = env.counters()

assert int(wasted) == 0, "a masked policy never asks for a move the mask rules out"
moving = c["moves"] / max(1, c["live_agent_steps"])
print(f"{E} envs, masked network in the loop (masks written by the step's own launch: {env.masks_fused(1)}): "
      f"eager {eager * 1e6:.1f} us/step, HIP graph {replay * 1e6:.1f} us/step ({E / replay:.3e} env-steps/s); "
      f"{c['episodes']} episodes restarted; {moving:.0%} of the live agent-steps moved (the rest chose to wait or lost a "
      f"same-step race for a cell)")
env.close()
