"""Record the reference's rendered frames at points the CCX_RENDER spec must reproduce (tests/golden/render/*.npz).

Runs the reference (``import_reference`` of gen_golden.py) in the build container, never on the GPU machine:

    python tests/golden/gen_render_golden.py

For each config the reference env is reset (and stepped with its GreedyPolicy where asked), ``env.render()`` draws the
Agg frame, and the axes its ``_draw_matplotlib`` drew into map grid coordinates to figure pixels (``ax.transData``).
Stored per config:
  - ``config_json``: the config's keyword arguments; ``geometry``: the ccx_params fields of the frame (width .. exiting_dest_y), ``x`` / ``y`` / ``types`` of every slot;
  - ``cell_rgb`` [H, W, 3] / ``cell_ok`` [H, W]: the frame at every cell centre (i + 1/2, j + 1/2), row j from y = 0;
  - ``agent_rgb`` [N, 3] / ``agent_ok`` [N]: the frame at (x + AGENT_DX, y + AGENT_DX), inside each agent's innermost disc;
  - ``origin`` / ``extent``: (row, col) of the axes' top-left corner and its size in the 800 x 1200 figure;
a point is ok only where the reference's 7 x 7 pixel neighbourhood is uniform, which drops text and grid lines.
"""

from __future__ import annotations

import json
import sys
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE))
from gen_golden import build_ref_config, import_reference  # noqa: E402

OUT = HERE / "render"
AGENT_DX = 0.08    # the agent point (x + d, y + d): clear of the label, inside the innermost disc (radius 0.2) and its edge

BASE = dict(truncated_config={"truncated_function": "max_steps", "max_steps": 100})
CONFIGS = {
    # the reference's own test_rendering (door interior width 0: door_right = door_left + 1)
    "ref_test_10x6": (dict(width=10, height=6, division_y=3, tram_door_left=3, tram_door_right=4, tram_length=8,
                           num_boarding_agents=2, num_exiting_agents=1, exiting_destination_area_y=0,
                           boarding_destination_area_y=4), 42, 0),
    # C2 (bench.py) after a few greedy steps; boarding_destination_area_y == H: the seats row sits at H - 1
    "c2_greedy": (dict(width=12, height=8, division_y=4, tram_door_left=5, tram_door_right=7, tram_length=9,
                       num_boarding_agents=5, num_exiting_agents=3, exiting_destination_area_y=0,
                       boarding_destination_area_y=8), 7, 4),
    # seats row inside the tram, wide door
    "seats_inside_16x10": (dict(width=16, height=10, division_y=5, tram_door_left=3, tram_door_right=8, tram_length=12,
                                num_boarding_agents=4, num_exiting_agents=4, exiting_destination_area_y=1,
                                boarding_destination_area_y=8), 3, 2),
    # no exit row (exiting_destination_area_y == division_y: outside the reference's validation, built unvalidated)
    "no_exit_row_9x7": (dict(width=9, height=7, division_y=3, tram_door_left=2, tram_door_right=4, tram_length=7,
                             num_boarding_agents=2, num_exiting_agents=2, exiting_destination_area_y=3,
                             boarding_destination_area_y=6, _relaxed=True), 11, 0),
    # door interior width 0 on an odd grid
    "narrow_door_13x9": (dict(width=13, height=9, division_y=4, tram_door_left=4, tram_door_right=5, tram_length=9,
                              num_boarding_agents=3, num_exiting_agents=2, exiting_destination_area_y=2,
                              boarding_destination_area_y=9), 5, 3),
}


def _uniform(img: np.ndarray, r: int, c: int, half: int = 3) -> bool:
    if r - half < 0 or c - half < 0 or r + half >= img.shape[0] or c + half >= img.shape[1]:
        return False
    win = img[r - half:r + half + 1, c - half:c + half + 1].reshape(-1, 3)
    return bool((win == win[0]).all())


def record(name: str, cfg: dict, seed: int, greedy_steps: int) -> dict:
    from collectivecrossing import CollectiveCrossingEnv

    env = CollectiveCrossingEnv(config=build_ref_config({**BASE, **cfg}))
    env.reset(seed=seed)
    if greedy_steps:
        from baseline_policies import GreedyPolicy
        pol = GreedyPolicy(randomness_factor=0.0, seed=42)
        for _ in range(greedy_steps):
            env.step({aid: int(pol.get_action(aid, None, env)) for aid in env.agents})
    axes = []
    draw = env._draw_matplotlib

    def capture(ax):
        axes.append(ax)
        return draw(ax)

    env._draw_matplotlib = capture
    img = np.asarray(env.render()).copy()
    ax = axes[-1]
    fig_h = img.shape[0]

    def pixel(X: float, Y: float) -> tuple[int, int]:
        dx, dy = ax.transData.transform((X, Y))
        return int(np.floor(fig_h - dy)), int(np.floor(dx))

    W, H = cfg["width"], cfg["height"]
    cell_rgb = np.zeros((H, W, 3), np.uint8)
    cell_ok = np.zeros((H, W), bool)
    for j in range(H):
        for i in range(W):
            r, c = pixel(i + 0.5, j + 0.5)
            cell_rgb[j, i] = img[r, c]
            cell_ok[j, i] = _uniform(img, r, c)
    agents = list(env._agents.values())
    xs = np.array([a.x for a in agents], np.int32)
    ys = np.array([a.y for a in agents], np.int32)
    types = np.array([0 if a.is_boarding else 1 for a in agents], np.int8)
    agent_rgb = np.zeros((len(agents), 3), np.uint8)
    agent_ok = np.zeros(len(agents), bool)
    for k, a in enumerate(agents):
        r, c = pixel(a.x + AGENT_DX, a.y + AGENT_DX)
        if 0 <= r < img.shape[0] and 0 <= c < img.shape[1]:
            agent_rgb[k] = img[r, c]
            agent_ok[k] = _uniform(img, r, c)
    # an agent's point also lies under every disc of an agent on the same grid point drawn later: fine, the spec blends
    # them in slot order too
    o_r, o_c = pixel(0.0, float(H))
    e_r, e_c = pixel(float(W), 0.0)
    geometry = np.array([W, H, cfg["division_y"], env.tram_left, env.tram_right, env.tram_door_left, env.tram_door_right,
                         cfg["boarding_destination_area_y"], cfg["exiting_destination_area_y"]], np.int32)
    return dict(geometry=geometry, x=xs, y=ys, types=types, cell_rgb=cell_rgb, cell_ok=cell_ok,
                agent_rgb=agent_rgb, agent_ok=agent_ok, origin=np.array([o_r, o_c], np.int32),
                extent=np.array([e_r - o_r, e_c - o_c], np.int32), seed=np.int64(seed),
                greedy_steps=np.int32(greedy_steps), relaxed=np.bool_(bool(cfg.get("_relaxed"))),
                config_json=np.array(json.dumps({k: v for k, v in cfg.items() if not k.startswith("_")})))


def main() -> None:
    import_reference()
    OUT.mkdir(exist_ok=True)
    for name, (cfg, seed, steps) in CONFIGS.items():
        rec = record(name, cfg, seed, steps)
        np.savez_compressed(OUT / f"{name}.npz", **rec)
        print(f"{name}: {int(rec['cell_ok'].sum())}/{rec['cell_ok'].size} cell centres, "
              f"{int(rec['agent_ok'].sum())}/{rec['agent_ok'].size} agent points uniform")


if __name__ == "__main__":
    main()
