#!/usr/bin/env python3
"""Training one side against a scripted other side: a torch network drives the boarding agents, the reference's
GreedyPolicy drives the exiting agents, and both meet in ONE launch per step (`rollout_mixed` / `step_mixed`) -- eagerly,
and with the loop body captured once into a HIP graph.  The network's action tensor carries whatever it likes in the
exiting slots: scripted slots are never read.  Episodes that end restart from a pool of seeded placements."""

import sys
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

import torch  # noqa: E402

from collectivecrossing_amd import BatchedCollectiveCrossing, CollectiveCrossingConfig  # noqa: E402
from collectivecrossing_amd.batched import scripted_slot_mask  # noqa: E402
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
scripted = scripted_slot_mask(config, "exiting")                      # 0b11100000: slots 5..7

torch.manual_seed(0)
policy = torch.nn.Sequential(torch.nn.Linear(L, 64), torch.nn.Tanh(), torch.nn.Linear(64, 5)).to(dev)
side = torch.cuda.Stream(device=dev)
env.use_stream(side)                                                  # bind the env to the stream BEFORE capturing on it

with torch.cuda.stream(side), torch.no_grad():
    obs = env.observe()                                               # f32 [E, N, L] on the device
    actions = torch.empty((1, E, N), dtype=torch.uint8, device=dev)
    taken = torch.empty((1, E, N), dtype=torch.uint8, device=dev)     # what every agent really did (255 = not asked)
    out = env.alloc_rollout(1)                                        # static one-step output buffers

    def body():
        actions[0].copy_(policy(obs).argmax(-1).to(torch.uint8))      # the network answers for every slot ...
        env.rollout_mixed(actions, scripted, "greedy", auto_reset=True, out=out, actions_out=taken, reset_obs="next")   # ... the exiting ones are scripted
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
    scripted_moves = int((taken[0, :, 5:] < 4).sum())

print(f"{E} envs, network on the boarding slots, greedy exiting agents: eager {eager * 1e6:.1f} us/step "
      f"({E / eager:.3e} env-steps/s), HIP graph {replay * 1e6:.1f} us/step ({E / replay:.3e} env-steps/s); "
      f"{c['episodes']} episodes finished and restarted, {c['arrivals']} arrivals in {c['env_steps']} env-steps; "
      f"{scripted_moves} scripted agents moved in the last step")
env.close()
