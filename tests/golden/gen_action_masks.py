#!/usr/bin/env python3
"""Legal-action fixtures ``g15_action_masks_*``: episodes of the REFERENCE in which, on every state an episode passes
through (the reset state and the state behind every step), the reference's own ``GreedyPolicy._is_valid_action(id, a,
env)`` (baseline_policies/greedy_policy.py:238-264 -> ``env._is_move_valid``, collectivecrossing.py:345-369) is asked for
every agent of ``env.agents`` and every action.

Built on the helpers of ``gen_golden.py`` (the reference import behind ``_refshim``, the ``cfg_*`` builders).  Per file,
with S = recorded states over all its episodes and N = agent slots (boarding first):

  config_json                           the config dict (tests/_fixtures.py: config_from_dict)
  x, y            i32 [S, N]            positions
  active, terminated, truncated  u8 [S, N]
  listed          u8 [S, N]             1 = the agent is in env.agents on that state
  masks           u8 [S, N]             bit a = _is_valid_action(id, a, env) for listed agents (bit 4 = wait, always);
                                        0x10 for the others (ccx.h: done agents may only wait)
  episode         i32 [S]               which episode of the file the state belongs to

The files live in a directory of their own (tests/golden/action_masks/): the step tests glob tests/golden/*.npz and
expect trajectories there.

Every cleared direction bit of a listed agent has one cause -- the target is outside the grid (bounds), inside it but
refused by ``_is_valid_position`` / ``_would_hit_tram_wall`` (wall / door row), or held by another active agent
(occupancy) -- and the generator prints the counts per file, cause and direction and insists that every cause occurs
for every direction somewhere in the set.

Usage: python tests/golden/gen_action_masks.py      (no-op when the reference is absent)
"""

from __future__ import annotations

import json
import sys
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent
OUT = HERE / "action_masks"
sys.path.insert(0, str(HERE))

import gen_golden as gg  # noqa: E402

DIRS = ((1, 0), (0, 1), (-1, 0), (0, -1))      # actions 0..3: right, up, left, down (actions.py:8-24)
CAUSES = ("bounds", "wall/door", "occupancy")


class MaskRecorder:
    def __init__(self, name: str, cfg: dict):
        from baseline_policies import create_greedy_policy
        from collectivecrossing import CollectiveCrossingEnv
        self.name, self.cfg = name, cfg
        self.ids = gg.ids_of(cfg)
        self.env = CollectiveCrossingEnv(config=gg.build_ref_config(cfg))
        self.policy = create_greedy_policy(epsilon=0.0)
        self.rows = {k: [] for k in ("x", "y", "active", "terminated", "truncated", "listed", "masks", "episode")}
        self.causes = np.zeros((3, 4), np.int64)
        self.episode = -1

    def reset(self, seed: int):
        self.episode += 1
        obs, _ = self.env.reset(seed=int(seed))
        self.snapshot()
        return obs

    def step(self, acts: dict) -> tuple[bool, bool]:
        _, _, term, trunc, _ = self.env.step(dict(acts))
        self.snapshot()
        return bool(term["__all__"]), bool(trunc["__all__"])

    def snapshot(self) -> None:
        env, c = self.env, self.cfg
        listed = set(env.agents)
        row = {k: [] for k in self.rows if k != "episode"}
        for aid in self.ids:
            ag = env._agents[aid]
            x, y = int(ag.position[0]), int(ag.position[1])
            m = 0x10
            if aid in listed:
                assert self.policy._is_valid_action(aid, 4, env)
                for a, (dx, dy) in enumerate(DIRS):
                    if self.policy._is_valid_action(aid, a, env):
                        m |= 1 << a
                        continue
                    tx, ty = x + dx, y + dy
                    cur, new = np.array([x, y]), np.array([tx, ty])
                    if not (0 <= tx <= c["width"] and 0 <= ty <= c["height"]):
                        cause = 0
                    elif not env._is_valid_position(new) or env._would_hit_tram_wall(cur, new):
                        cause = 1
                    else:
                        assert env._is_position_occupied(new, exclude_agent=aid)
                        cause = 2
                    self.causes[cause, a] += 1
            for k, v in (("x", x), ("y", y), ("active", ag.active), ("terminated", ag.terminated),
                         ("truncated", ag.truncated), ("listed", aid in listed), ("masks", m)):
                row[k].append(int(v))
        for k, v in row.items():
            self.rows[k].append(v)
        self.rows["episode"].append(self.episode)

    def save(self) -> np.ndarray:
        OUT.mkdir(exist_ok=True)
        dt = dict(x=np.int32, y=np.int32, episode=np.int32)
        arrays = {k: np.asarray(v, dt.get(k, np.uint8)) for k, v in self.rows.items()}
        out = OUT / f"{self.name}.npz"
        np.savez_compressed(out, config_json=np.array(json.dumps(self.cfg)), **arrays)
        print(f"wrote action_masks/{out.name}: S={len(arrays['episode'])} N={len(self.ids)} {out.stat().st_size / 1024:.0f} KiB")
        for ci, cname in enumerate(CAUSES):
            print(f"    cleared by {cname:10s} right/up/left/down = {self.causes[ci].tolist()}")
        return self.causes


def random_episodes(name, cfg, seeds, max_states, p_wait=0.0):
    """reset(seed), then uniform actions for env.agents until the episode ends (or max_states are recorded)."""
    rec = MaskRecorder(name, cfg)
    for seed in seeds:
        rec.reset(seed)
        rng = np.random.default_rng(15100 + int(seed))
        for _ in range(max_states):
            acts = {aid: (4 if rng.random() < p_wait else int(rng.integers(0, 4))) for aid in rec.env.agents}
            at, au = rec.step(acts)
            if at or au:
                break
    return rec.save()


def greedy_episodes(name, cfg, seeds, max_states):
    """The reference's greedy policy drives everybody: agents arrive (and, with all_at_destination, stay listed while
    inactive -- arrived agents may then share a cell)."""
    rec = MaskRecorder(name, cfg)
    for seed in seeds:
        obs = rec.reset(seed)
        for _ in range(max_states):
            env = rec.env
            acts = {aid: int(rec.policy.get_action(aid, obs.get(aid), env)) for aid in env.agents}
            at, au = rec.step(acts)
            obs = {aid: env._get_agent_observation(aid) for aid in env.agents}
            if at or au:
                break
    return rec.save()


def edge_walk(name, cfg, seed):
    """One boarding agent walks the waiting area to x == width, x == 0 and y == 0; one exiting agent walks the tram to
    its side walls and to y == height.  The others wait where reset() put them."""
    rec = MaskRecorder(name, cfg)
    rec.reset(seed)
    env, W, H = rec.env, cfg["width"], cfg["height"]

    def walk(aid, action, until):
        side = (1, 3) if action in (0, 2) else (0, 2)               # blocked by somebody: step aside and go on
        for _ in range(2 * (W + H)):
            if until(env._agents[aid].position):
                return
            ok = rec.policy._is_valid_action(aid, action, env)
            rec.step({aid: action if ok else next(a for a in side if rec.policy._is_valid_action(aid, a, env))})

    b, e = "boarding_0", "exiting_0"
    walk(b, 0, lambda p: p[0] == W)
    walk(b, 3, lambda p: p[1] == 0)
    walk(b, 2, lambda p: p[0] == 0)
    walk(e, 1, lambda p: p[1] == H)
    walk(e, 0, lambda p: not rec.policy._is_valid_action(e, 0, env))
    walk(e, 2, lambda p: not rec.policy._is_valid_action(e, 2, env))
    assert any(W in r for r in rec.rows["x"]) and any(H in r for r in rec.rows["y"]), "the walk must reach x == W and y == H"
    return rec.save()


def main() -> int:
    if not (gg.REF / "src" / "collectivecrossing").is_dir():
        print(f"reference not found at {gg.REF}: nothing to do (fixtures are committed)")
        return 0
    gg.import_reference()
    short = dict(truncated_config=dict(truncated_function="max_steps", max_steps=40))
    total = np.zeros((3, 4), np.int64)
    total += random_episodes("g15_action_masks_c1", gg.cfg_c1(**short), seeds=range(3, 7), max_states=40)
    total += random_episodes("g15_action_masks_c3_dense", gg.cfg_c3(
        truncated_config=dict(truncated_function="max_steps", max_steps=30)), seeds=[40, 41], max_states=30, p_wait=0.2)
    # sealed door (door_right - door_left == 1): the whole division row is wall
    total += random_episodes("g15_action_masks_sealed_door", gg.cfg_c1(tram_door_left=5, tram_door_right=6, **short),
                             seeds=range(10, 13), max_states=40)
    total += edge_walk("g15_action_masks_edge_walk", gg.cfg_c1(
        num_boarding_agents=2, num_exiting_agents=2, truncated_config=dict(truncated_function="max_steps", max_steps=200)), seed=5)
    # all_at_destination: arrived agents stay in env.agents, inactive, and share cells of the destination rows
    total += greedy_episodes("g15_action_masks_all_at_destination", gg.cfg_c1(
        width=8, tram_length=6, tram_door_left=2, tram_door_right=4, num_boarding_agents=6, num_exiting_agents=5,
        terminated_config=dict(terminated_function="all_at_destination"),
        truncated_config=dict(truncated_function="max_steps", max_steps=60)), seeds=[7, 8], max_states=60)
    total += random_episodes("g15_action_masks_100x100", gg.cfg_big(
        num_boarding_agents=6, num_exiting_agents=5, truncated_config=dict(truncated_function="max_steps", max_steps=60)),
        seeds=[60], max_states=60)
    print("whole set:")
    for ci, cname in enumerate(CAUSES):
        print(f"    cleared by {cname:10s} right/up/left/down = {total[ci].tolist()}")
    assert (total > 0).all(), "every cause must occur for every direction somewhere in the set"
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
