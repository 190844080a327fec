#!/usr/bin/env python3
"""Device time of per-side policy heads (include/ccx.h CCX_SIDES: two Linear(L, 64) -> Tanh -> Linear(64, 5), one per side) from
replayed HIP graphs, in ONE process on ONE build so that every variant sees the same machine.  Per shape, the actor step:

  sides.sample_actions    ccx_sides_sample_actions over both sides: rows -> actions, logp, one kernel
  (a) gather + sample     THE YARDSTICK, the captured composition it replaces: per side index_select -> MlpHead -> index_copy_
                          into the logits, then ccx_sample_actions (seven kernels)
  (b) shared head         ccx_mlp_sample_actions with ONE head for all slots (context: what one network costs)
  boarding only           ccx_sides_sample_actions with SideHeads({"boarding": ...}): the exiting rows are not read

and the learner's pair on a [16, E, N, L] minibatch:

  sides fwd + bwd         sides(x, hidden_out=) and backward_into(out=): one kernel and two launches per side
  gathered fwd + bwd      per side index_select of x and of grad_y -> MlpHead(hidden_out=) -> mlp_backward(out=)

The protocol of mlp_timing.py: a graph holds CALLS calls; a repeat replays it REPLAYS times between two synchronisations; the
variants alternate over 15 repeats; the median is reported with min .. max.  Measured, not gated.

    python profiles/side_heads_timing.py [--out profiles/side_heads_timing.txt]
"""

import argparse
import statistics
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "profiles"))
H, KROWS = 64, 16
# label, workload, envs, calls per graph, replays per repeat (actor), the same for the learner's pair
SHAPES = [("C2 4096 x 8", "c2", 4096, 20, 10, 4, 3), ("C3 4096 x 32", "c3", 4096, 10, 10, 2, 2), ("C2 64 x 8", "c2", 64, 20, 10, 10, 5)]


def measure(cfg, E, calls, replays, lcalls, lreplays):
    import torch
    from mlp_timing import time_graphs

    from collectivecrossing_amd import BatchedCollectiveCrossing, SideHeads

    env = BatchedCollectiveCrossing(cfg, E)
    env.make_reset_pool(seed0=0, size=4096)
    env.reset_from_pool()
    N, L, dev = env.num_agents, env.obs_len, env.device
    side = torch.cuda.Stream()
    with torch.cuda.stream(side), torch.no_grad():
        env.use_stream(side)
        torch.manual_seed(0)
        sides = SideHeads(env, {"boarding": env.mlp_head(H), "exiting": env.mlp_head(H)})
        boarding = SideHeads(env, {"boarding": sides.heads[0]})
        shared = env.mlp_head(H)
        idx = [torch.tensor([a for a in range(N) if mask >> a & 1], device=dev) for mask, _ in sides.groups]
        obs, masks = env.observe(), env.action_masks()
        logits = torch.zeros((E, N, 5), device=dev)
        out = env.alloc_sample(want_logp=True)
        held = {}

        def gather_sample():
            for i, (_, head) in zip(idx, sides.groups):
                held["g"] = head(torch.index_select(obs, 1, i))
                logits.index_copy_(1, i, held["g"])
            env.sample_actions(logits, masks, out=out)

        actor = {"sides.sample_actions": lambda: sides.sample_actions(obs, masks, out=out), "gather + sample": gather_sample,
                 "shared head": lambda: env.mlp_sample_actions(shared, obs, masks, out=out),
                 "boarding only": lambda: boarding.sample_actions(obs, masks, out=out)}
        gather_sample()
        want = env.sample_actions(logits, masks)
        got = sides.sample_actions(obs, masks)
        side.synchronize()
        assert torch.equal(want.actions, got.actions) and torch.equal(want.logp.view(torch.int32), got.logp.view(torch.int32))
        times = time_graphs(torch, side, actor, calls, replays)

        # ---- the learner's pair on [KROWS, E, N, L]
        lead = (KROWS, E, N)
        x = obs.expand(KROWS, E, N, L).contiguous()
        gy = torch.randn(lead + (5,), device=dev)
        y, hid = torch.empty(lead + (5,), device=dev), torch.empty(lead + (H,), device=dev)
        grads = sides.alloc_backward(lead)
        per_side = []
        for i, (_, head) in zip(idx, sides.groups):
            S = i.numel()
            per_side.append((i, head, torch.empty((KROWS, E, S, L), device=dev), torch.empty((KROWS, E, S, 5), device=dev),
                             torch.empty((KROWS, E, S, 5), device=dev), torch.empty((KROWS, E, S, H), device=dev),
                             env.alloc_mlp_backward(head, (KROWS, E, S))))

        def sides_pair():
            sides(x, out=y, hidden_out=hid)
            sides.backward_into(x, hid, gy, out=grads)

        def gathered_pair():
            for i, head, gx, ggy, gout, ghid, gres in per_side:
                torch.index_select(x, 2, i, out=gx)
                torch.index_select(gy, 2, i, out=ggy)
                head(gx, out=gout, hidden_out=ghid)
                env.mlp_backward(head, gx, ghid, ggy, out=gres)

        sides_pair()
        gathered_pair()
        side.synchronize()
        for o, (*_, gres) in zip(grads, per_side):
            assert torch.equal(o.w1t.view(torch.int32), gres.w1t.view(torch.int32)) and torch.equal(o.b2.view(torch.int32), gres.b2.view(torch.int32))
        times.update(time_graphs(torch, side, {"sides fwd + bwd": sides_pair, "gathered fwd + bwd": gathered_pair}, lcalls, lreplays))
        held.clear()
    env.use_stream(None)
    env.close()
    return times, E * N


def cell(v):
    return "-" if v is None else f"{statistics.median(v):.1f} ({min(v):.1f} .. {max(v):.1f})"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", type=Path, default=ROOT / "profiles" / "side_heads_timing.txt")
    args = ap.parse_args()
    sys.path.insert(0, str(ROOT))
    import bench
    import torch
    from mlp_timing import REPEATS

    assert torch.cuda.is_available(), "this is a measurement on the GPU"
    lines = [f"# {torch.cuda.get_device_name(0)}; us per call, median of {REPEATS} alternating repeats (min .. max); a repeat = replays of a "
             f"graph of several calls between two synchronisations",
             f"# two heads Linear(L, {H}) -> Tanh -> Linear({H}, 5), boarding and exiting.  sides.sample_actions: ccx_sides_sample_actions, rows ->",
             "# actions and logp in one kernel; (a) per side index_select -> MlpHead -> index_copy_, then ccx_sample_actions: the yardstick;",
             "# (b) ccx_mlp_sample_actions with one shared head; boarding only: SideHeads over the boarding slots alone.",
             f"# learner: forward with hidden and backward on [{KROWS}, E, N, L]: sides(x, hidden_out=) + backward_into against per side",
             "# index_select of x and grad_y -> MlpHead -> mlp_backward"]
    cols = ("sides.sample_actions", "gather + sample", "shared head", "boarding only", "sides fwd + bwd", "gathered fwd + bwd")
    names = {"gather + sample": "(a) gather + sample", "shared head": "(b) shared head"}
    lines.append(f"{'shape':<14}{'rows':>8}" + "".join(f"{names.get(c, c):>27}" for c in cols) + f"{'sides/(a)':>11}{'only/(b)':>10}{'learner':>9}")
    print("\n".join(lines), flush=True)
    for label, workload, E, calls, replays, lcalls, lreplays in SHAPES:
        cfg, _ = bench.workload_config(workload)
        t, rows = measure(cfg, E, calls, replays, lcalls, lreplays)
        med = {k: statistics.median(v) for k, v in t.items()}
        row = (f"{label:<14}{rows:>8}" + "".join(f"{cell(t.get(c)):>27}" for c in cols)
               + f"{med['sides.sample_actions'] / med['gather + sample']:>11.3f}{med['boarding only'] / med['shared head']:>10.3f}"
               + f"{med['sides fwd + bwd'] / med['gathered fwd + bwd']:>9.3f}")
        lines.append(row)
        print(row, flush=True)
    args.out.parent.mkdir(parents=True, exist_ok=True)
    args.out.write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
