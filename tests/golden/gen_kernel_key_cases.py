"""Prints the CASES table of tests/_kernel_keys.py: for every key the sweep reaches, the smallest case that selects it in
the LAST launch of its call -- and, for the rollout kernel, one per tile filling (the planner's own, full tiles), per cause
of PLAIN = false (a move order, an in-kernel policy, a user table: each alone) and per cause of OUT 2 (a slab or tile region
off the 128-byte lines; an aligned slab at residue 16); one more per rollout key that a forcing occ_tables setting reaches
(_kernel_keys.occ_is_forced), and per kernel and (GLOG, PAIR) two with actions_out: next to the other outputs, and alone.

    python tests/golden/gen_kernel_key_cases.py > cases.txt          (CPU; needs the built library)

Smallest: batches of the reduced space before larger ones, library defaults before tunables, the smallest grid that admits N, the smallest N, a batch of at least three tiles
with a ragged last one (one env per tile: three envs) before any other, then the fewest envs, the shortest call (K from 1 and 3 for the step kernel, 5 and 17 for the rollout kernel), the most outputs.
Keys that this reduced space (few agent counts, E up to 140) does not reach are looked for in the test's own sweep space."""
import ctypes as C
import itertools
import sys
from pathlib import Path

import numpy as np

sys.path[:0] = [str(Path(__file__).resolve().parents[2]), str(Path(__file__).resolve().parents[1])]
import _kernel_keys as kk  # noqa: E402
from _shape_plan import CALL_FIELDS, gen  # noqa: E402

GEN_KS = [1, 3, 5, 17]
GEN_N = [1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 16, 17, 18, 32, 33, 34, 49, 50, 63, 64]
GEN_E = list(range(1, 161))
BIG = [(40, 30), (64, 48), (100, 100)]           # grids whose occupancy tables the planner itself gives up


def smallest_grid(n):
    return min((g for g in kk.GRIDS if n in kk.agent_counts(*g)), key=lambda g: g[0] * g[1])


def gen_calls():
    out = []
    for dname, K, sk, oname in itertools.product(kk.DRIVE_NAMES, GEN_KS, (-1, 0), kk.OUTPUTS):
        drive = kk.DRIVE_NAMES[dname][0]
        policy, mixed = drive[2], drive[4]
        for masks, reset in itertools.product((0, 1), (0, 1)):
            if (masks and policy) or (reset and (policy or mixed or oname == "none")):
                continue
            out.append((dname, K, sk, oname, masks, reset))
    return out


def main():
    from collectivecrossing_amd import _lib
    lib = C.CDLL(str(_lib.LIB_PATH))
    names = gen.bind(lib)
    kk.bind_keys(lib)
    gcalls = gen_calls()
    calls = np.array([kk.call_in(K, kk.DRIVE_NAMES[d][0], m, r, sk) for d, K, sk, o, m, r in gcalls], np.int32)
    facts = np.array([kk.OUTPUTS[o] for d, K, sk, o, m, r in gcalls], np.int32)
    f = CALL_FIELDS
    cause = (calls[:, f.index("order")] != 0) * 1 + (calls[:, f.index("policy")] != 0) * 2      # 0 none, 1 order, 2 policy, 3 both
    crank = [(sk != -1, K, -list(kk.OUTPUTS).index(o), m, r, list(kk.DRIVE_NAMES).index(d)) for d, K, sk, o, m, r in gcalls]
    order = sorted(range(len(gcalls)), key=lambda i: crank[i])
    calls, facts, cause = np.ascontiguousarray(calls[order]), np.ascontiguousarray(facts[order]), cause[order]
    gcalls = [gcalls[i] for i in order]
    crank = [crank[i] for i in order]
    best = {}

    def visit(handle):
        w, h, n, e, lanes, occ, rt, tt = handle
        pin = kk.plan_in(*handle)
        out = np.empty((len(calls), 2, 8), np.int32)
        assert lib.ccxi_call_keys(C.byref(pin), (C.c_int * 2)(2, 2), calls.ctypes.data, facts.ctypes.data, len(calls), out.ctypes.data) == 0
        keys = kk.pack(out[:, 1])
        plan = [dict(zip(names, gen.plan_row(lib, len(names), [getattr(pin, x) if x != "rows" else rows for x in gen.IN_FIELDS], 2)))
                for rows in (1, 0)]
        ao = calls[:, f.index("actions_out")] != 0
        uniq, first = np.unique(keys * 256 + cause * 64 + (facts[:, 5] != 0) * 32 + (facts[:, 0] != 0) * 16 + (calls[:, 0] >= 5) * 8
                                + ao * 4 + (facts[:, 1] == 0) * 2, return_index=True)
        forced = kk.occ_is_forced(lib, names, handle)
        if occ != -1 and not forced:
            return                                         # (a setting that changes nothing: the default handle is the case)
        for u, i in zip(uniq, first):
            key = kk.unpack(u // 256)
            if key[0] < 0:
                continue
            c, residue, has_obs = int(cause[i]), int(facts[i, 5]), int(facts[i, 0])
            tag, ew = "", plan[0]["kp_EW"]
            if (key[0] == kk.KERNEL_ROLLOUT) != (gcalls[i][1] >= 5):
                continue                                   # K = 1, 3 for the step kernel's keys, 5 and 17 for the rollout kernel's
            slot = key
            if ao[i]:
                # the chosen actions as an output, next to the others and alone: one case per kernel and (GLOG, PAIR)
                if forced or lanes or rt or tt or residue or gcalls[i][4] or gcalls[i][5]:
                    continue
                tag = "actions_out_only" if facts[i, 1] == 0 else "actions_out"
                slot = key[:3]
                if key[0] == kk.KERNEL_ROLLOUT:
                    ew = plan[0 if has_obs else 1]["kp_EW"]
                else:
                    ew = plan[0]["step_envs_per_wave"]
            elif key[0] == kk.KERNEL_ROLLOUT:
                ew = plan[0 if has_obs else 1]["kp_EW"]
                tag = "occ_forced" if forced else "full" if lanes else "default"
                causes = [x for x, on in (("order", c & 1), ("policy", c & 2), ("tables", rt or tt)) if on]
                if not key[5]:
                    if len(causes) != 1:
                        continue
                    if not forced:
                        tag += "/" + causes[0]
                elif rt or tt:
                    continue
                if key[3] == 2:
                    row = n * (6 + 4 * n) * 4
                    off_lines = ((ew * row) | (e * row)) & 127
                    if bool(off_lines) == bool(residue):
                        continue
                    if not forced:
                        tag += "/residue16" if residue else "/off_lines"
                elif residue:
                    continue
            else:
                if key[0] == kk.KERNEL_STEP:
                    ew = plan[0]["step_envs_per_wave"]
                if residue or rt or tt or forced:
                    continue
            tiles = -(-e // max(ew, 1))
            good = tiles >= 3 and (ew <= 1 or e % ew != 0)
            rank = (e > GEN_E[-1], crank[i][0], lanes != 0 and tag in ("", "occ_forced"), w * h, n, not good, e, rt + tt) + crank[i][1:]
            d, K, sk, o, m, r = gcalls[i]
            case = (key, (w, h), n, e, K, d, o, "reward" if rt else "terminated" if tt else "none", m, r, lanes, occ, sk, tag)
            if (slot, tag) not in best or rank < best[slot, tag][0]:
                best[slot, tag] = (rank, case)

    def settings():
        for lanes, occ in itertools.product((0, 64), (-1, 0, 1)):
            yield lanes, occ, 0, 0
            yield lanes, occ, 0, 1

    for n in GEN_N:
        for (w, h) in [smallest_grid(n)] + [g for g in BIG if n in kk.agent_counts(*g)]:
            for e in GEN_E:
                for lanes, occ, rt, tt in settings():
                    visit((w, h, n, e, lanes, occ, rt, tt))
                    if lanes == 0 and kk.reward_table_fits(lib, len(names), names, w, h, n, e, lanes, occ):
                        visit((w, h, n, e, lanes, occ, 1, 0))
    reached = kk.sweep_keys(lib, names)
    have = {c[0] for _, c in best.values()}
    missing = reached - have - {k for k in reached if k[0] == kk.KERNEL_OBSERVE}
    if missing:
        print("# looked for in the sweep's own space:", sorted(missing), file=sys.stderr)
        for handle in kk.handle_space(lib, names):
            pin = kk.plan_in(*handle)
            out = np.empty((len(calls), 2, 8), np.int32)
            lib.ccxi_call_keys(C.byref(pin), (C.c_int * 2)(2, 2), calls.ctypes.data, facts.ctypes.data, len(calls), out.ctypes.data)
            if missing & {kk.unpack(p) for p in np.unique(kk.pack(out[:, 1]))}:
                # (the batch sizes between the reduced space and this one: the first that reaches the key wins by its rank)
                w, h, n, e, *rest = handle
                if (w, h) == smallest_grid(n) or (w, h) in BIG:
                    for e2 in sorted(set(range(GEN_E[-1] + 1, e, 8)) | {e}):
                        visit((w, h, n, e2, *rest))
    for handle in kk.handle_space(lib, names):             # every handle of the sweep whose occ_tables setting forces the choice
        if kk.occ_is_forced(lib, names, handle):
            visit(handle)
    # (forcing settings that the sweep's batch sizes reach only far beyond the reduced space: the sizes in between)
    for _, case in list(best.values()):
        if case[-1] == "occ_forced" and case[3] > GEN_E[-1]:
            for e2 in (257, 513, 1025, 1537, 2049, 3073, 4097, 5121, 6145, 8193):
                if e2 < case[3]:
                    visit((*case[1], case[2], e2, case[10], case[11], int(case[7] == "reward"), int(case[7] == "terminated")))
    have = {c[0] for _, c in best.values()}
    print("# still missing:", sorted(reached - have - {k for k in reached if k[0] == kk.KERNEL_OBSERVE}), file=sys.stderr)
    for _, case in sorted(best.values(), key=lambda v: (v[1][0], v[1][-1], v[1])):
        if case[0] in reached:
            print(f"    {case},")
    for key in sorted(k for k in reached if k[0] == kk.KERNEL_OBSERVE):
        n = 1 if key[1] == 0 else 2 if key[1] == 1 else (1 << (key[1] - 1)) + (2 if key[2] else 1)
        print(f"    {(key, smallest_grid(n), n, 2 * (64 >> key[1]) + 1, 0, 'observe', 'rows', 'none', 0, 0, 0, -1, -1, '')},")


if __name__ == "__main__":
    main()
