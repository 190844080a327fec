#!/usr/bin/env python3
"""Generate tests/golden/g15_array_strategies.json.gz by RUNNING THE REFERENCE with the g15 plugins of
array_strategies.py (per-agent form) registered in ITS registries; every dict it returns is recorded as data.

The reference is imported the way gen_golden.py imports it (``CCX_REFERENCE``, the stand-ins of ``_refshim/``); only the
data file is committed.  Per episode: ``geometry`` ("C1" / "BIG": array_strategies.C1 / BIG), ``max_steps``, ``seed``,
``forced`` (positions poked into env._agents after reset), ``initial`` positions, and per step the ordered action dict,
the post-step ``positions`` [N][2] and ``flags`` [N][3] (active, terminated, truncated), ``step_count``, the ``rewards`` /
``terminateds`` / ``truncateds`` dicts as returned (absent keys stay absent) and the keys of ``observations``.

Usage: python tests/golden/gen_array_golden.py
"""

from __future__ import annotations

import gzip
import json
import sys
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE))

# (geometry, max_steps, seed, steps, agents placed next to their destination row and walked onto it in the first steps)
EPISODES = [
    ("C1", 14, 1500, 24, {"exiting_0": [3, 2], "boarding_0": [8, 6]}),
    ("C1", 14, 1501, 24, {"exiting_0": [3, 1], "boarding_0": [8, 7]}),
    # four of eight agents arrive within two steps: the half-arrived rule ends the episode for everybody
    ("C1", 14, 1502, 24, {"exiting_0": [3, 1], "exiting_1": [5, 2], "boarding_0": [8, 7], "boarding_1": [6, 6]}),
    # a grid whose occupancy tables do not fit in LDS: four early arrivals, two neighbours inside the tram, the crowd
    # budget runs out near step 22
    ("BIG", 30, 1503, 36, {"exiting_0": [30, 2], "exiting_1": [40, 1], "boarding_0": [45, 98], "boarding_1": [55, 99],
                           "boarding_2": [50, 52], "boarding_3": [50, 51]}),
]


def main() -> None:
    import array_strategies as ast
    from gen_golden import import_reference
    import_reference()
    from collectivecrossing import CollectiveCrossingEnv, configs, reward_configs, rewards
    from collectivecrossing import terminated_configs, terminateds, truncated_configs, truncateds

    plugins = ast.make_g15(rewards.RewardFunction, terminateds.TerminatedFunction, truncateds.TruncatedFunction)
    rewards.REWARD_FUNCTIONS[ast.G15_NAMES["reward"]] = plugins["reward"]
    terminateds.TERMINATED_FUNCTIONS[ast.G15_NAMES["terminated"]] = plugins["terminated"]
    truncateds.TRUNCATED_FUNCTIONS[ast.G15_NAMES["truncated"]] = plugins["truncated"]
    episodes = []
    for geometry, max_steps, seed, num_steps, forced in EPISODES:
        env = CollectiveCrossingEnv(config=ast.g15_config(configs, reward_configs, terminated_configs, truncated_configs,
                                                          getattr(ast, geometry), max_steps))
        env.reset(seed=seed)
        ids = list(env._agents)
        for a, pos in forced.items():
            env._agents[a].position = np.array(pos)
        initial = [[int(v) for v in env._agents[a].position] for a in ids]
        rng = np.random.default_rng(seed)
        steps = []
        for k in range(num_steps):
            acting = [a for a in ids if rng.random() > 0.1]
            rng.shuffle(acting)
            acts = {a: int(rng.integers(0, 5)) for a in acting}
            if k < 4:       # the forced agents walk straight to their destination row
                acts.update({a: (3 if a.startswith("exiting") else 1) for a in list(forced)[:4] if a in acts})
            o, r, te, tr, _ = env.step(dict(acts))
            steps.append(dict(
                actions=acts, positions=[[int(v) for v in env._agents[a].position] for a in ids],
                flags=[[bool(env._agents[a].active), bool(env._agents[a].terminated), bool(env._agents[a].truncated)] for a in ids],
                step_count=int(env._step_count), rewards={k_: float(v) for k_, v in r.items()},
                terminateds={k_: bool(v) for k_, v in te.items()}, truncateds={k_: bool(v) for k_, v in tr.items()},
                obs_keys=sorted(o)))
        episodes.append(dict(geometry=geometry, max_steps=max_steps, seed=seed, forced=forced, ids=ids, initial=initial, steps=steps))
    f = HERE / "g15_array_strategies.json.gz"
    with gzip.GzipFile(f, "wb", mtime=0) as z:
        z.write(json.dumps(dict(episodes=episodes), separators=(",", ":")).encode())
    print(f"wrote {f.name}: {len(episodes)} episodes, {sum(len(e['steps']) for e in episodes)} steps, {f.stat().st_size} bytes")


if __name__ == "__main__":
    main()
