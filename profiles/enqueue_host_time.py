#!/usr/bin/env python3
"""Host time of an enqueueing call with the handle's stream current: this tree against its parent commit.

The calls (``observe``, ``sample_actions``, ``mlp_sample_actions`` with H = 64, ``evaluate_actions(out=)``, ``ppo_loss(out=)``,
``q_actions(out=)``) run on the stream-order harness's small shapes (E = 64, N = 8, 257 rows for the row-wise ops), static
buffers, no grad.  Their kernels last microseconds, so a host clock around CALLS calls that end in a synchronise measures
the enqueue: the Python between the caller and the launch.

A repeat is a fresh child process (``--child``) that imports the package from one directory, warms every call up and times
it once.  Three versions alternate, in a rotating order, REPEATS times each: this tree, and TWO copies of the parent
commit's package (with the same ``libccx.so``).  The two parents differ by nothing but chance, so the distance of their
medians is the margin: a call passes when this tree's median is no slower than the slower parent's.

    python profiles/enqueue_host_time.py --parent DIR_A --parent-copy DIR_B [--out profiles/enqueue_host_time.txt]

``DIR_A`` / ``DIR_B`` hold ``collectivecrossing_amd/`` of the parent commit, e.g. from ``git archive HEAD~1
collectivecrossing_amd | tar -x -C DIR_A`` plus a copy of the built ``libccx.so``.
"""

import argparse
import json
import statistics
import subprocess
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
E, N, ROWS, H = 64, 8, 257, 64
CALLS, WARMUP, REPEATS = 3000, 500, 15
OPS = ("observe", "sample_actions", "mlp_sample_actions", "evaluate_actions", "ppo_loss", "q_actions")


def child(pkg_root: str) -> None:
    sys.path.insert(0, pkg_root)
    import torch

    import collectivecrossing_amd as pkg
    from collectivecrossing_amd import configs as cfgs
    from collectivecrossing_amd.qlearn import QLearning

    assert Path(pkg.__file__).resolve().is_relative_to(Path(pkg_root).resolve()), pkg.__file__
    cfg = cfgs.CollectiveCrossingConfig(
        width=12, height=8, division_y=4, tram_door_left=5, tram_door_right=7, tram_length=9, num_boarding_agents=5,
        num_exiting_agents=3, exiting_destination_area_y=0, boarding_destination_area_y=8,
        truncated_config=cfgs.MaxStepsTruncatedConfig(max_steps=12),
        terminated_config=cfgs.IndividualAtDestinationTerminatedConfig())
    torch.manual_seed(0)
    b = pkg.BatchedCollectiveCrossing(cfg, E)                  # (the handle's stream is the current one)
    b.make_reset_pool(seed0=11, size=128)
    b.reset_from_pool()
    b.set_rng_seed(5)
    dev, f = b.device, torch.float32
    with torch.no_grad():
        obs, masks = b.observe(), b.action_masks()
        logits, sample = torch.randn((E, N, 5), device=dev), b.alloc_sample(True, True)
        head = b.mlp_head(H)
        rl = torch.randn((ROWS, 5), device=dev)
        ra = torch.randint(0, 5, (ROWS,), device=dev).to(torch.uint8)
        ev = b.alloc_evaluate((ROWS,))
        rv, rlp, radv, rret = (torch.randn((ROWS,), device=dev, dtype=f) for _ in range(4))
        ppo = b.alloc_ppo_loss((ROWS,))
        ql = QLearning(b, epsilon=0.1)
        qa = ql.alloc_q_actions()
        ops = {
            "observe": lambda: b.observe(out=obs),
            "sample_actions": lambda: b.sample_actions(logits, masks, out=sample),
            "mlp_sample_actions": lambda: b.mlp_sample_actions(head, obs, masks, out=sample),
            "evaluate_actions": lambda: b.evaluate_actions(rl, ra, out=ev),
            "ppo_loss": lambda: b.ppo_loss(rl, rv, ra, rlp, radv, rret, out=ppo),
            "q_actions": lambda: ql.q_actions(logits, masks, out=qa),
        }
        us = {}
        for name in OPS:
            call = ops[name]
            for _ in range(WARMUP):
                call()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(CALLS):
                call()
            torch.cuda.synchronize()
            us[name] = (time.perf_counter() - t0) / CALLS * 1e6
    b.close()
    print("RESULT " + json.dumps(us), flush=True)


def run_child(pkg_root: Path) -> dict:
    p = subprocess.run([sys.executable, str(Path(__file__).resolve()), "--child", str(pkg_root)], capture_output=True, text=True,
                       timeout=300, cwd=str(pkg_root))
    if p.returncode != 0:
        raise SystemExit(f"child on {pkg_root} ended with {p.returncode}:\n{p.stdout}\n{p.stderr}")
    return json.loads(next(line for line in p.stdout.splitlines() if line.startswith("RESULT "))[7:])


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--child")
    ap.add_argument("--parent", type=Path)
    ap.add_argument("--parent-copy", type=Path)
    ap.add_argument("--out", type=Path, default=ROOT / "profiles" / "enqueue_host_time.txt")
    args = ap.parse_args()
    if args.child:
        return child(args.child)
    if args.parent is None or args.parent_copy is None:
        ap.error("--parent and --parent-copy are required")
    versions = {"change": ROOT, "parent A": args.parent.resolve(), "parent B": args.parent_copy.resolve()}
    names = list(versions)
    got = {v: {op: [] for op in OPS} for v in names}
    for r in range(REPEATS):
        for v in names[r % 3:] + names[:r % 3]:
            for op, t in run_child(versions[v]).items():
                got[v][op].append(t)
        print(f"# repeat {r + 1} / {REPEATS}", flush=True)
    lines = [f"# host us per call, handle's stream current; E = {E}, N = {N}, {ROWS} rows; {CALLS} calls + synchronise after {WARMUP}",
             f"# warm-up calls; {REPEATS} fresh processes per version, alternating.  parent A / B: two copies of the parent commit.",
             "# margin = |median A - median B|; pass: median(change) <= max(median A, median B)"]
    ok = True
    for op in OPS:
        med = {v: statistics.median(got[v][op]) for v in names}
        lines.append(f"\n{op}")
        for v in names:
            lines.append(f"  {v:>9}  " + " ".join(f"{t:7.3f}" for t in got[v][op]))
        passed = med["change"] <= max(med["parent A"], med["parent B"])
        ok = ok and passed
        lines.append("  medians  " + "  ".join(f"{v} {med[v]:.3f}" for v in names)
                     + f"  margin {abs(med['parent A'] - med['parent B']):.3f}  {'PASS' if passed else 'FAIL'}")
    text = "\n".join(lines) + "\n"
    print(text, flush=True)
    args.out.parent.mkdir(parents=True, exist_ok=True)
    args.out.write_text(text)
    if not ok:
        raise SystemExit(1)


if __name__ == "__main__":
    main()
