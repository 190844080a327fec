#!/usr/bin/env python3
"""Device time of CCX_DUELING (include/ccx.h) from replayed HIP graphs, in ONE process on ONE build so that every variant sees
the same machine.  Per shape (E envs of N agents, heads of H = 64, masks given, a rate of 0.1):

  mlp_q 5 / mlp_q 6       ccx_mlp_q_actions with a plain (O = 5) / dueling (O = 6) head: one launch
  (a) pair 5 / 6          YARDSTICK: the existing composition head(obs) -> q_actions (two launches), with dueling between them
                          for O = 6 (three launches)
  sides_q 5 / sides_q 6   ccx_sides_q_actions with a boarding and an exiting head: one launch
  (a) sides pair 5 / 6    YARDSTICK: sides(obs) -> [dueling ->] q_actions
  into x3                 ccx_dueling_forward on three arrays of E N rows: one launch
  3 singles               three single calls
  (b) torch x3            YARDSTICK: v + a - a.mean(-1, keepdim=True) on the three arrays, captured torch ops
  bwd                     ccx_dueling_backward: one launch
  (b) torch grad          YARDSTICK: torch.autograd.grad of that expression with the same cotangent, captured

The protocol of td_loss_timing.py: a graph holds CALLS calls; a repeat replays it REPLAYS times between two
synchronisations; the variants alternate over 15 repeats; the median is reported with min .. max.  Measured, not gated.

    python profiles/dueling_timing.py [--out profiles/dueling_timing.txt]
"""

import argparse
import statistics
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
REPEATS = 15
HIDDEN, EPS = 64, 0.1
# label, workload, envs, calls per graph, replays per repeat
SHAPES = [("C2 4096 x 8", "c2", 4096, 10, 10), ("C3 4096 x 32", "c3", 4096, 10, 10), ("C2 64 x 8", "c2", 64, 20, 10)]
ACTOR = ("mlp_q 5", "pair 5", "mlp_q 6", "pair 6", "sides_q 5", "sides pair 5", "sides_q 6", "sides pair 6")
COMBINE = ("into x3", "3 singles", "torch x3", "bwd", "torch grad")


def torch_dueling(va):
    a, v = va[..., :5], va[..., 5:]
    return v + a - a.mean(-1, keepdim=True)


def measure(cfg, E, calls, replays):
    import torch

    from collectivecrossing_amd import BatchedCollectiveCrossing, QLearning, SideHeads

    env = BatchedCollectiveCrossing(cfg, E)
    N, dev = env.num_agents, env.device
    side = torch.cuda.Stream()
    graphs = {}
    with torch.cuda.stream(side):
        env.use_stream(side)
        env.make_reset_pool(seed0=0, size=4096)
        env.reset_from_pool()
        env.rollout_greedy(30, auto_reset=False, want_obs=False, want_actions=False)       # some agents have arrived: dead slots
        ql = QLearning(env, epsilon=EPS)
        torch.manual_seed(0)
        obs, masks = env.observe(), env.action_masks()
        head = {O: env.mlp_head(HIDDEN, O=O) for O in (5, 6)}
        sides = {O: SideHeads(env, {s: env.mlp_head(HIDDEN, O=O) for s in ("boarding", "exiting")}) for O in (5, 6)}
        y = {O: torch.empty((E, N, O), device=dev) for O in (5, 6)}
        q = torch.empty((E, N, 5), device=dev)
        fused, pair = ql.alloc_q_actions(), ql.alloc_q_actions()
        vas = tuple(torch.randn((E, N, 6), device=dev) for _ in range(3))
        qs = tuple(torch.empty((E, N, 5), device=dev) for _ in range(3))
        gq, gva = torch.randn((E, N, 5), device=dev), torch.empty((E, N, 6), device=dev)
        x = vas[0].clone().requires_grad_(True)
        held = {}

        def pair_of(net, O):
            def body():
                with torch.no_grad():
                    net(obs, out=y[O])
                ql.q_actions(ql.dueling(y[6], out=q) if O == 6 else y[5], masks, out=pair)
            return body

        def singles():
            for va, out in zip(vas, qs):
                ql.dueling(va, out=out)

        def t_x3():
            with torch.no_grad():
                held["x3"] = [torch_dueling(va) for va in vas]

        def t_grad():
            held["g"] = torch.autograd.grad(torch_dueling(x), x, gq)

        bodies = {"into x3": lambda: ql.dueling_into(vas, qs), "3 singles": singles, "torch x3": t_x3,
                  "bwd": lambda: ql.dueling_backward(gq, out=gva), "torch grad": t_grad}
        for O in (5, 6):
            bodies[f"mlp_q {O}"] = lambda O=O: ql.mlp_q_actions(head[O], obs, masks, out=fused)
            bodies[f"pair {O}"] = pair_of(head[O], O)
            bodies[f"sides_q {O}"] = lambda O=O: ql.sides_q_actions(sides[O], obs, masks, out=fused)
            bodies[f"sides pair {O}"] = pair_of(sides[O], O)
        # the fused launch and its yardstick compute the same actions, the torch yardsticks the same values (to rounding):
        # a wrong yardstick would be no yardstick
        for O in (5, 6):
            for a, b in ((f"mlp_q {O}", f"pair {O}"), (f"sides_q {O}", f"sides pair {O}")):
                bodies[a]()
                bodies[b]()
                side.synchronize()
                assert torch.equal(fused.actions, pair.actions), (a, b)
        bodies["into x3"]()
        t_x3()
        bodies["bwd"]()
        t_grad()
        side.synchronize()
        assert all(torch.allclose(a, b, rtol=1e-5, atol=1e-5) for a, b in zip(qs, held["x3"]))
        assert torch.allclose(gva, held["g"][0], rtol=1e-5, atol=1e-5)
        for name, body in bodies.items():
            body()                                                  # warm-up: code objects, allocator blocks
            side.synchronize()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, stream=side):
                for _ in range(calls):
                    body()
            for _ in range(2):
                g.replay()
            side.synchronize()
            graphs[name] = g
        times = {k: [] for k in graphs}
        for _ in range(REPEATS):
            for name, g in graphs.items():                          # alternate the variants
                side.synchronize()
                t0 = time.perf_counter()
                for _ in range(replays):
                    g.replay()
                side.synchronize()
                times[name].append((time.perf_counter() - t0) / (replays * calls) * 1e6)
        graphs.clear()
        held.clear()
    env.use_stream(None)
    env.close()
    return times


def cell(v):
    return f"{statistics.median(v):.1f} ({min(v):.1f} .. {max(v):.1f})"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", type=Path, default=ROOT / "profiles" / "dueling_timing.txt")
    args = ap.parse_args()
    sys.path.insert(0, str(ROOT))
    import bench
    import torch

    assert torch.cuda.is_available(), "this is a measurement on the GPU"
    lines = [f"# {torch.cuda.get_device_name(0)}; us per call, median of {REPEATS} alternating repeats (min .. max); a repeat = replays of a "
             f"graph of several calls between two synchronisations",
             f"# heads of H = {HIDDEN}, masks given, rate {EPS}.  mlp_q / sides_q O: ccx_mlp_q_actions / ccx_sides_q_actions, ONE launch, O = 5 plain,",
             "# O = 6 dueling; (a) pair: head(obs) -> [dueling ->] q_actions, two / three launches.  into x3: ccx_dueling_forward on three",
             "# arrays of E N rows, one launch; 3 singles: three calls; (b) torch x3 / torch grad: v + a - a.mean(-1) and its autograd.grad as",
             "# captured torch ops; bwd: ccx_dueling_backward"]
    names = {"pair 5": "(a) pair 5", "pair 6": "(a) pair 6", "sides pair 5": "(a) sides pair 5", "sides pair 6": "(a) sides pair 6",
             "torch x3": "(b) torch x3", "torch grad": "(b) torch grad"}
    rows = []
    for label, workload, E, calls, replays in SHAPES:
        cfg, _ = bench.workload_config(workload)
        rows.append((label, measure(cfg, E, calls, replays)))
        print(label, {k: round(statistics.median(v), 2) for k, v in rows[-1][1].items()}, flush=True)
    for cols, ratios in ((ACTOR, (("mlp_q 5", "pair 5"), ("mlp_q 6", "pair 6"), ("sides_q 5", "sides pair 5"), ("sides_q 6", "sides pair 6"))),
                         (COMBINE, (("into x3", "3 singles"), ("into x3", "torch x3"), ("bwd", "torch grad")))):
        lines.append(f"{'shape':<14}" + "".join(f"{names.get(c, c):>24}" for c in cols) + "".join(f"{a + '/' + b:>24}" for a, b in ratios))
        for label, t in rows:
            med = {k: statistics.median(v) for k, v in t.items()}
            lines.append(f"{label:<14}" + "".join(f"{cell(t[c]):>24}" for c in cols) + "".join(f"{med[a] / med[b]:>24.3f}" for a, b in ratios))
    print("\n".join(lines), flush=True)
    args.out.parent.mkdir(parents=True, exist_ok=True)
    args.out.write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
