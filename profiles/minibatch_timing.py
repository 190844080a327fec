#!/usr/bin/env python3
"""Device time of `ccx_minibatch_next` / `ccx_minibatch_fetch` (include/ccx.h CCX_MINIBATCH) from replayed HIP graphs, in ONE
process on ONE build so that every variant sees the same machine.  Per shape (E envs x N agents, a rollout of K = 64 steps, M =
K E records) and minibatch size B (M / 4 and M / 32):

  next rows         RolloutMinibatches.next on row-form observations with obs0: two launches (draw + gather, the state)
  next compact      the same on compact records (the gather expands them)
  fetch             RolloutMinibatches.fetch, row form, on the first B indices of epoch 0's permutation: one launch
  (a) rows          YARDSTICK: the captured torch composition on the same index: seven `index_select(out=)`
  (a) compact       YARDSTICK: six of them, `index_select` on the compact array and `expand_observations`
  (b) copy          YARDSTICK: `torch.Tensor.copy_` of the bytes the row-form gather reads (as many again are written)
  (c) randperm      `torch.randperm(M)`, eager (not captured): the draw that goes away, once per EPOCH in the examples

The protocol of td_loss_timing.py: a graph holds CALLS calls; a repeat replays it REPLAYS times between two synchronisations;
the variants alternate over 15 repeats; the median is reported with min .. max.

    python profiles/minibatch_timing.py [--out profiles/minibatch_timing.txt]
"""

import argparse
import statistics
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
REPEATS = 15
K = 64
# workload, label, calls per graph, replays per repeat
SHAPES = [("c2", "C2 4096 x 8", 10, 5), ("c3", "C3 4096 x 32", 5, 2)]
DIVISORS = (4, 32)
COLS = ("next rows", "next compact", "fetch", "a rows", "a compact", "copy", "randperm")


def measure(cfg, E, calls, replays):
    import torch

    from collectivecrossing_amd import BatchedCollectiveCrossing, RolloutMinibatches

    env = BatchedCollectiveCrossing(cfg, E)
    N, L, dev = env.num_agents, env.obs_len, env.device
    M = K * E
    side = torch.cuda.Stream()
    results = {}
    with torch.cuda.stream(side):
        env.use_stream(side)
        env.set_rng_seed(7)
        u8, f32 = torch.uint8, torch.float32
        gen = torch.Generator(device=dev).manual_seed(1)
        compact = torch.randint(0, 9, (K, E, N, 4), device=dev, generator=gen).to(f32)
        compact0 = torch.randint(0, 9, (E, N, 4), device=dev, generator=gen).to(f32)
        rows, rows0 = env.expand_observations(compact), env.expand_observations(compact0)
        small = dict(actions=torch.randint(0, 5, (K, E, N), device=dev, generator=gen).to(u8),
                     logp=-torch.rand((K, E, N), device=dev, generator=gen), advantages=torch.randn((K, E, N), device=dev, generator=gen),
                     returns=torch.randn((K, E, N), device=dev, generator=gen),
                     masks=(torch.randint(0, 32, (K, E, N), device=dev, generator=gen) | 0x10).to(u8),
                     valid=(torch.rand((K, E, N), device=dev, generator=gen) < 0.8).to(u8) * 4)
        # the row the step acted on, as the yardsticks' flat arrays [M, ...]
        flat = {k: t.reshape(M, N) for k, t in small.items()}
        flat_rows = torch.cat([rows0, rows.reshape(M, N, L)[:M - E]])
        flat_compact = torch.cat([compact0, compact.reshape(M, N, 4)[:M - E]])
        perm_out = torch.empty((M,), dtype=torch.int64, device=dev)
        for div in DIVISORS:
            B = M // div
            mr = RolloutMinibatches(env, num_steps=K, batch_size=B)
            mr.set_source(rows, obs0=rows0, **small)
            mc = RolloutMinibatches(env, num_steps=K, batch_size=B)
            mc.set_source(compact, obs0=compact0, **small)
            out_r, out_c, out_f = mr.alloc(), mc.alloc(), mr.alloc()
            idx = mr.permutation(0)[:B].clone()
            sel = {k: torch.empty((B, N), dtype=t.dtype, device=dev) for k, t in flat.items()}
            sel_rows, sel_compact = torch.empty((B, N, L), device=dev), torch.empty((B, N, 4), device=dev)
            exp = torch.empty((B, N, L), device=dev)
            gather_bytes = B * N * (4 * L + 14) + 4 * B                  # read; as many are written (the index once)
            src = torch.empty(gather_bytes, dtype=u8, device=dev)
            dst = torch.empty_like(src)

            def a_rows():
                torch.index_select(flat_rows, 0, idx, out=sel_rows)
                for k, t in flat.items():
                    torch.index_select(t, 0, idx, out=sel[k])

            def a_compact():
                torch.index_select(flat_compact, 0, idx, out=sel_compact)
                for k, t in flat.items():
                    torch.index_select(t, 0, idx, out=sel[k])
                env.expand_observations(sel_compact, out=exp)

            bodies = {"next rows": lambda: mr.next(out=out_r), "next compact": lambda: mc.next(out=out_c),
                      "fetch": lambda: mr.fetch(idx, out=out_f), "a rows": a_rows, "a compact": a_compact,
                      "copy": lambda: dst.copy_(src), "randperm": lambda: torch.randperm(M, device=dev, out=perm_out)}
            # the yardsticks move the same things: the first draw of epoch 0 equals the gather of its indices
            mr.next(out=out_r)
            mc.next(out=out_c)
            a_rows()
            a_compact()
            side.synchronize()
            assert torch.equal(out_r.index, idx) and torch.equal(out_c.index, idx)
            assert torch.equal(out_r.obs, sel_rows) and torch.equal(out_c.obs, exp) and torch.equal(out_r.obs, out_c.obs)
            assert all(torch.equal(getattr(out_r, k), sel[k]) and torch.equal(getattr(out_c, k), sel[k]) for k in flat)
            graphs = {}
            for name, body in bodies.items():
                body()                                                  # warm-up: code objects, allocator blocks
                side.synchronize()
                if name == "randperm":                                  # (its sort is not captured: eager calls, host time included)
                    graphs[name] = None
                    continue
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
                        if g is None:
                            for _ in range(calls):
                                bodies[name]()
                        else:
                            g.replay()
                    side.synchronize()
                    times[name].append((time.perf_counter() - t0) / (replays * calls) * 1e6)
            graphs.clear()
            results[B] = (times, 2 * gather_bytes)
    env.use_stream(None)
    env.close()
    return results, M


def cell(v):
    return f"{statistics.median(v):.1f} ({min(v):.1f} .. {max(v):.1f})"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", type=Path, default=ROOT / "profiles" / "minibatch_timing.txt")
    args = ap.parse_args()
    sys.path.insert(0, str(ROOT))
    import bench
    import torch

    assert torch.cuda.is_available(), "this is a measurement on the GPU"
    lines = [f"# {torch.cuda.get_device_name(0)}; us per call, median of {REPEATS} alternating repeats (min .. max); a repeat = replays of a "
             f"graph of several calls between two synchronisations",
             f"# a rollout of K = {K} steps, M = K E records; next: RolloutMinibatches.next (rows / compact source, obs0 given); fetch: the row-form",
             "# gather on given indices; (a) the captured torch composition on the same index: seven index_select(out=) / six + the compact",
             "# array + expand_observations; (b) a torch copy of the bytes the row-form gather reads (as many are written); (c) torch.randperm(M)"]
    names = {"a rows": "(a) rows", "a compact": "(a) compact", "copy": "(b) copy", "randperm": "(c) randperm"}
    head = (f"{'shape':<14}{'M':>8}{'B':>7}{'moved MB':>10}" + "".join(f"{names.get(c, c):>28}" for c in COLS)
            + f"{'rows/(a)':>10}{'compact/(a)':>13}{'rows/(b)':>10}")
    lines.append(head)
    print("\n".join(lines), flush=True)
    for workload, label, calls, replays in SHAPES:
        cfg, E = bench.workload_config(workload)
        results, M = measure(cfg, E, calls, replays)
        for B, (t, moved) in results.items():
            med = {k: statistics.median(v) for k, v in t.items()}
            row = f"{label:<14}{M:>8}{B:>7}{moved / 1e6:>10.1f}" + "".join(f"{cell(t[c]):>28}" for c in COLS)
            row += f"{med['next rows'] / med['a rows']:>10.4f}{med['next compact'] / med['a compact']:>13.4f}{med['next rows'] / med['copy']:>10.4f}"
            lines.append(row)
            print(row, flush=True)
    args.out.parent.mkdir(parents=True, exist_ok=True)
    args.out.write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
