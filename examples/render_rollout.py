#!/usr/bin/env python3
"""Video of a greedy rollout: K fused steps of the on-device greedy policy with the compact observation output, drawn as
frames for 4 envs in one ccx_render_compact launch and saved as PNG (first and last step) and an animated GIF (when PIL
imports; otherwise the frames are only rendered)."""

import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

import numpy as np  # noqa: E402

from collectivecrossing_amd import BatchedCollectiveCrossing, CollectiveCrossingConfig  # noqa: E402
from collectivecrossing_amd.truncated_configs import MaxStepsTruncatedConfig  # noqa: E402

K, E, SHOW, CELL_PX = 40, 256, 4, 16
config = CollectiveCrossingConfig(
    width=12, height=8, division_y=4, tram_door_left=5, tram_door_right=7, tram_length=9,
    num_boarding_agents=5, num_exiting_agents=3, exiting_destination_area_y=0,
    boarding_destination_area_y=8, truncated_config=MaxStepsTruncatedConfig(max_steps=100))

batch = BatchedCollectiveCrossing(config, E)
batch.make_reset_pool(seed0=0, size=1024)
batch.reset_from_pool()
traj, _ = batch.rollout_greedy(K, auto_reset=True, out=batch.alloc_rollout(K, want_obs=False, want_compact=True))
video = batch.render_compact(traj.obs_compact[:, :SHOW], cell_px=CELL_PX)       # [K, 4, H*cp, W*cp, 3] uint8
frames = video.cpu().numpy()
# the 4 envs side by side, one image per step
strip = np.concatenate(list(frames.transpose(1, 0, 2, 3, 4)), axis=2)              # [K, H*cp, 4*W*cp, 3]
print(f"rendered {K} steps x {SHOW} envs: {tuple(video.shape)}")

out = Path(__file__).resolve().parent / "render_out"
try:
    from PIL import Image
except ImportError:
    print("PIL is not installed: frames rendered, nothing saved")
else:
    out.mkdir(exist_ok=True)
    images = [Image.fromarray(f) for f in strip]
    images[0].save(out / "step_000.png")
    images[-1].save(out / f"step_{K - 1:03d}.png")
    images[0].save(out / "rollout.gif", save_all=True, append_images=images[1:], duration=120, loop=0)
    print(f"saved {out / 'rollout.gif'} and two PNGs")
batch.close()
