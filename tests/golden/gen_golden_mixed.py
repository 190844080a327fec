#!/usr/bin/env python3
"""Mixed-control fixtures ``g15_mixed_*``: episodes of the REFERENCE in which one side's actions come from the reference's
own policy object (``create_greedy_policy(epsilon=0)`` / ``create_waiting_policy(epsilon=0)``,
``policy.get_action(aid, obs[aid], env)`` for the ids of ``env.agents`` on that side -- the loop of
scripts/run_greedy_policy_demo.py:67-109) and the other side's from a seeded numpy generator.

Built on the helpers of ``gen_golden.py`` (the reference import behind ``_refshim``, ``Recorder``, the ``cfg_*`` builders);
the fixtures (tests/golden/mixed/) are the usual arrays (see that file's docstring) plus

  scripted_mask  u64   bit a = agent slot a was driven by the policy
  policy         str   "greedy" | "waiting"

``actions`` holds what the reference's ``step`` received: the policy's action in the scripted slots, the generator's in
the others, 255 for agents that were not in the action dict.  ``garbage_bytes`` is what the tests put into the scripted
slots of the tensor they hand to the device: uniform bytes in 0..4, seeded by the fixture's name.

Usage: python tests/golden/gen_golden_mixed.py      (no-op when the reference is absent)
"""

from __future__ import annotations

import json
import sys
import zlib
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent
# A directory of their own: the step tests glob tests/golden/*.npz and expect every fixture there to fit the step kernel's
# LDS tables, which the 100 x 100 episode (recorded for the unfused path) does not.
MIXED = HERE / "mixed"
sys.path.insert(0, str(HERE))

import gen_golden as gg  # noqa: E402


def garbage_bytes(name: str, shape) -> np.ndarray:
    """Uniform bytes in 0..4, seeded by the fixture's name: what goes into the scripted slots of the action tensor."""
    return np.random.default_rng(zlib.crc32(name.encode())).integers(0, 5, size=shape, dtype=np.uint8)


def slots_of(cfg: dict, scripted) -> list[int]:
    nb, n = cfg["num_boarding_agents"], cfg["num_boarding_agents"] + cfg["num_exiting_agents"]
    if scripted == "boarding":
        return list(range(nb))
    if scripted == "exiting":
        return list(range(nb, n))
    return sorted(int(s) for s in scripted)


def run_mixed(name, cfg, seeds, K, scripted, policy, shuffle=False, p_absent=0.0, act_done=False):
    """reset(seed) then K steps: the scripted slots ask the reference's policy object (one per env), the others draw
    uniform actions; ``shuffle`` permutes the dict order (move order), ``act_done`` / ``p_absent`` as in run_random for the
    tensor-driven side."""
    from baseline_policies import create_greedy_policy, create_waiting_policy
    rec = gg.Recorder(cfg, len(seeds), K)
    sl = slots_of(cfg, scripted)
    scripted_ids = {rec.ids[i] for i in sl}
    for e, seed in enumerate(seeds):
        env = rec.envs[e]
        obs, _ = env.reset(seed=int(seed))
        rec.snapshot_init(e)
        pol = (create_greedy_policy if policy == "greedy" else create_waiting_policy)(epsilon=0.0)
        rng = np.random.default_rng(15000 + int(seed))
        for s in range(K):
            live = list(env.agents)
            acts = {}
            for aid in rec.ids:
                if aid in scripted_ids:
                    if aid in live:
                        acts[aid] = int(pol.get_action(aid, obs.get(aid), env))
                elif (act_done or aid in live) and rng.random() >= p_absent:
                    acts[aid] = int(rng.integers(0, 5))
            if shuffle:
                keys = list(acts)
                acts = {keys[i]: acts[keys[i]] for i in rng.permutation(len(keys))}
            rec.step(s, e, acts)
            obs = {aid: env._get_agent_observation(aid) for aid in env.agents}
    mask = sum(1 << i for i in sl)
    a = rec.a["actions"]
    live_scripted = (a[:, :, sl] != gg.ABSENT)
    differ = live_scripted & (a[:, :, sl] != garbage_bytes(name, a.shape)[:, :, sl])
    print(f"{name}: {int(live_scripted.sum())} scripted agent-steps, {int(differ.sum())} differ from the garbage byte")
    assert 2 * int(differ.sum()) >= int(live_scripted.sum()) > 0, "choose other seeds: the fixture must discriminate"
    MIXED.mkdir(exist_ok=True)
    out = MIXED / f"{name}.npz"
    np.savez_compressed(out, config_json=np.array(json.dumps(cfg)), **rec.a, seeds=np.asarray(seeds, np.int64),
                        scripted_mask=np.uint64(mask), policy=np.array(policy))
    print(f"wrote mixed/{out.name}: E={rec.E} K={rec.K} N={rec.N} {out.stat().st_size / 1024:.0f} KiB")


def main() -> int:
    if not (gg.REF / "src" / "collectivecrossing").is_dir():
        print(f"reference not found at {gg.REF}: nothing to do (fixtures are committed)")
        return 0
    gg.import_reference()
    short = dict(truncated_config=dict(truncated_function="max_steps", max_steps=40))
    # C1 geometry: greedy exiting agents against random boarding agents, and the other way round with the waiting policy
    run_mixed("g15_mixed_c1_exiting_greedy", gg.cfg_c1(**short), seeds=range(3, 7), K=46, scripted="exiting", policy="greedy")
    run_mixed("g15_mixed_c1_boarding_waiting", gg.cfg_c1(**short), seeds=range(20, 24), K=46, scripted="boarding",
              policy="waiting")
    # C3 class: 32 agents, dense
    run_mixed("g15_mixed_c3_exiting_greedy", gg.cfg_c3(truncated_config=dict(truncated_function="max_steps", max_steps=36)),
              seeds=[40, 41], K=40, scripted="exiting", policy="greedy")
    # an odd agent count (and an odd E x N), every other slot scripted
    run_mixed("g15_mixed_n5_odd_alternating", gg.cfg_c1(num_boarding_agents=3, num_exiting_agents=2, **short),
              seeds=range(50, 53), K=46, scripted=[0, 2, 4], policy="greedy")
    # 100 x 100: no LDS tables, the library's unfused path
    run_mixed("g15_mixed_100x100_boarding_waiting", gg.cfg_big(
        num_boarding_agents=6, num_exiting_agents=5, truncated_config=dict(truncated_function="max_steps", max_steps=90)),
        seeds=[60], K=96, scripted="boarding", policy="waiting")
    # shuffled dict order = move order; the tensor side also names done agents and omits some
    run_mixed("g15_mixed_c1_shuffled_boarding_greedy", gg.cfg_c1(**short), seeds=range(70, 74), K=46, scripted="boarding",
              policy="greedy", shuffle=True, p_absent=0.1, act_done=True)
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
