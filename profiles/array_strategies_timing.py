"""Time the split step and array-form user strategies (not part of bench.py).

    python profiles/array_strategies_timing.py            -> profiles/array_strategies_timing.txt

C2 geometry (12 x 8, 5 + 3 agents) at 4096 and at 64 envs, microseconds per env-step of the whole batch:
  (a) step()                      the short-launch kernel, built-in config, of THIS build (not a build of the parent
                                  commit: the split step leaves csrc/ccx_step.hip and its compile flags alone)
  (b) step_begin + step_finish()  the two split kernels with the built-in rules; floor: 2.45 us per launch
                                  (profiles/r04_launch_floor.txt: a launch with 5.6 MB of streaming stores), twice
  (c) step() with the g12 "all" mix / the g15 plugins in array form (tests/golden/array_strategies.py)
  (d) the only way to run (c) without array-form strategies: single-env CollectiveCrossingEnv objects on the host slow
      path, timed for a sample of envs and scaled to E
Each of (a)-(c) eager (one Python call per launch: bound by the host's enqueue cost, about 4 us per library launch) and
graph-replayed (torch.cuda.graph on the handle's stream, 25 steps per graph: the device time of the chain).  Method:
5 warm-up blocks, then the median of CCX_TIMING_BLOCKS (default 40) blocks of 25 steps, each block between two events on
the handle's stream.
"""

from __future__ import annotations

import json
import os
import sys
import time
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests" / "golden"))

import array_strategies as ast  # noqa: E402
import custom_strategies as cs  # noqa: E402

from collectivecrossing_amd import CollectiveCrossingEnv  # noqa: E402
from collectivecrossing_amd import configs as C  # noqa: E402
from collectivecrossing_amd import strategies as S  # noqa: E402
from collectivecrossing_amd.batched import BatchedCollectiveCrossing  # noqa: E402
from collectivecrossing_amd.reset import build_reset_pool  # noqa: E402

BLOCKS = int(os.environ.get("CCX_TIMING_BLOCKS", "40"))
PER_BLOCK = 25
LAUNCH_FLOOR_US = 2.45


NOTES = (
    "us per env-step of the whole batch, medians. (a) is step() of this build, not of a build of the parent commit (the "
    "short-launch kernel's source and flags are unchanged). (b)/(a) is about 2 because (b) is two dependent launches where (a) is "
    "one: each pays the launch floor (2.45 us with a C2 step's stores, 1.56 us empty), and finish re-reads from memory "
    "what the fused kernel keeps in registers (state -> cell word -> LDS staging -> barrier -> stores: two dependent "
    "global round trips). Eager figures are bound by the host's enqueue cost per library call, the same at 64 and 4096 "
    "envs. (c) is dominated by the user's torch code between the halves (about 15 small torch kernels for the g12 mix, "
    "about 25 for g15), not by the split kernels. (d) = seconds per step of single-env objects on the host slow path, "
    "sampled on 4 envs x 25 steps and multiplied by E. HBM bytes of the two kernels: profiles/array_strategies_pmc.txt; "
    "algorithmic bytes per C2 agent-step: begin 10 read + 9 written, finish 11 read + user arrays (8 + 1 + 1) "
    "+ 164 written (152 observation row, 8 reward, flag byte, term_present byte, 2 state flag bytes).")


def builtin_config():
    return C.CollectiveCrossingConfig(**ast.C2, truncated_config=C.MaxStepsTruncatedConfig(max_steps=100))


def time_blocks(stream, fn, calls=PER_BLOCK, steps_per_call=1):
    """Median microseconds per env-step over BLOCKS blocks of `calls` calls of fn (events on `stream`)."""
    out = []
    with torch.cuda.stream(stream):
        for b in range(BLOCKS + 5):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            for _ in range(calls):
                fn()
            e1.record(stream)
            e1.synchronize()
            if b >= 5:
                out.append(e0.elapsed_time(e1) * 1000.0 / (calls * steps_per_call))
    return float(np.median(out))


def measure(config, E, body):
    """(eager us, graph-replayed us) per step of body(batch, actions) with auto-reset keeping the episodes alive."""
    stream = torch.cuda.Stream()
    batch = BatchedCollectiveCrossing(config, E)
    batch.use_stream(stream)
    batch.set_reset_pool(build_reset_pool(config, 0, 256))
    batch.reset_from_pool()
    actions = torch.from_numpy(np.random.default_rng(0).integers(0, 5, size=(E, 8), dtype=np.uint8)).cuda()
    torch.cuda.synchronize()
    eager = time_blocks(stream, lambda: body(batch, actions))
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=stream):     # one graph = one block of steps: a chain of dependent launches
        for _ in range(PER_BLOCK):
            body(batch, actions)
    replay = time_blocks(stream, graph.replay, calls=1, steps_per_call=PER_BLOCK)
    batch.close()
    return eager, replay


def step_body(batch, a):
    batch.step(a)


def split_body(batch, a):
    batch.step_begin(a)
    batch.step_finish(auto_reset=True)


def array_body(batch, a):
    batch.step_begin(a)
    batch.step_finish(*batch.run_array_strategies(), auto_reset=True)


def host_slow_path(config, envs=4, steps=25):
    """Seconds per env-step of ONE single-env object with per-agent strategies on the host."""
    ids = None
    t = 0.0
    for e in range(envs):
        env = CollectiveCrossingEnv(config=config)
        env.reset(seed=e)
        ids = list(env._agents)
        rng = np.random.default_rng(e)
        env.step({a: 4 for a in ids})
        t0 = time.perf_counter()
        for _ in range(steps):
            _, _, te, tr, _ = env.step({a: int(rng.integers(0, 5)) for a in ids})
            if te["__all__"] or tr["__all__"]:
                env.reset(seed=e)
        t += time.perf_counter() - t0
        env.close()
    return t / (envs * steps)


def main() -> None:
    undo = [ast.register(S, ast.make_g12_twins(S.RewardFunction, S.TerminatedFunction, S.TruncatedFunction), cs.NAMES),
            ast.register(S, ast.make_g15(S.RewardFunction, S.TerminatedFunction, S.TruncatedFunction), ast.G15_NAMES)]
    g12 = cs.build_config(C, C, C, C, cs.MIXES["all"], max_steps=100)
    g15 = ast.g15_config(C, C, C, C, ast.C2, 100)
    lines = []
    for E in (4096, 64):
        a = measure(builtin_config(), E, step_body)
        b = measure(builtin_config(), E, split_body)
        c12 = measure(g12, E, array_body)
        c15 = measure(g15, E, array_body)
        d12, d15 = host_slow_path(g12) * E * 1e6, host_slow_path(g15) * E * 1e6
        lines.append({
            "envs": E, "agents": 8,
            "a_step_us": {"eager": round(a[0], 2), "graph": round(a[1], 2)},
            "b_begin_finish_us": {"eager": round(b[0], 2), "graph": round(b[1], 2), "launch_floor_us": 2 * LAUNCH_FLOOR_US},
            "b_over_a": {"eager": round(b[0] / a[0], 2), "graph": round(b[1] / a[1], 2)},
            "c_g12_all_us": {"eager": round(c12[0], 2), "graph": round(c12[1], 2)},
            "c_g15_us": {"eager": round(c15[0], 2), "graph": round(c15[1], 2)},
            "d_host_slow_path_us": {"g12_all": round(d12, 1), "g15": round(d15, 1)},
            "d_over_c": {"g12_all_eager": round(d12 / c12[0], 1), "g12_all_graph": round(d12 / c12[1], 1),
                         "g15_eager": round(d15 / c15[0], 1), "g15_graph": round(d15 / c15[1], 1)},
        })
        print(json.dumps(lines[-1]), flush=True)
    for u in undo:
        u()
    lines.append({"notes": NOTES})
    out = Path(os.environ.get("CCX_TIMING_OUT", ROOT / "profiles" / "array_strategies_timing.txt"))
    out.write_text("".join(json.dumps(line) + "\n" for line in lines))


if __name__ == "__main__":
    main()
