"""The per-call planner (csrc/ccx_plan.hip: plan_call, plan_launch) against an independent restatement of its rules
(tests/_call_plan_spec.py), on a machine without a GPU.

The handle plans come from tests/golden/shape_plan/parent_plans.npz (the MI355X's own occupancy figures): the 12 x 8 grid
with 8 agents at six batch sizes, 5 agents for the odd slab, and two synthetic batches at the 32-bit limit that no test
could allocate.  ``ccxi_plan_call`` must equal the spec field for field over a sweep of calls and tunables; literal anchors,
worked out by hand from the rules, keep the spec honest; and the sweep must reach both sides of every decision of the spec
and more than one value of every field."""

import ctypes as C
import itertools

import numpy as np
import pytest

import _call_plan_spec as spec
from _shape_plan import DRIVES, bind_call, call, gen, plan_call, setting_of

SHAPE_FIELDS = ["num_blocks", "resident_blocks", "step_bytes", "paced", "pace_adapt", "pace_min_k", "adapt_min_k",
                "ring_when_paced", "step_ok"]
SYNTHETIC = {(4194303, 64): (1, 1), (4194303, 63): (1, 1)}     # (E, N) -> blocks_per_cu of the two shapes, made up


class Planner:
    """ccxi_plan_call and ccxi_plan of the built library, and the recorded handles."""

    def __init__(self):
        from collectivecrossing_amd import _lib

        if not _lib.LIB_PATH.exists():
            pytest.skip("libccx.so not built (run __graft_entry__.build())")
        self.lib = lib = C.CDLL(str(_lib.LIB_PATH))
        self.plan_names = gen.bind(lib)
        self.names = bind_call(lib)
        self.table = gen.load_table()

    def handle(self, E, N):
        """(planner inputs, blocks_per_cu[2], the two shapes as the spec reads them) of a default handle on the 12 x 8 grid."""
        t, f = self.table, gen.IN_FIELDS
        if (E, N) in SYNTHETIC:
            values = [gen.plan_inputs(12, 8, N, E, None, 0, 256, 1)[n] for n in f]
            per_cu = SYNTHETIC[E, N]
        else:
            ins = t["inputs"]
            hit = np.flatnonzero((ins[f.index("width")] == 12) & (ins[f.index("height")] == 8) & (ins[f.index("N")] == N)
                                 & (ins[f.index("E")] == E) & (ins[f.index("rows")] == 1))
            i = next(int(i) for i in hit if setting_of(t, i) is None)
            assert ins[f.index("rows"), i + 1] == 0 and t["refused"][i] == 0
            values, per_cu = ins[:, i], (int(t["blocks_per_cu"][i]), int(t["blocks_per_cu"][i + 1]))
        shapes = []
        for rows, b in zip((1, 0), per_cu):
            v = list(values)
            v[f.index("rows")] = rows
            out = dict(zip(self.plan_names, gen.plan_row(self.lib, len(self.plan_names), v, b)))
            shapes.append({n: out[n] for n in SHAPE_FIELDS})
        return list(values), per_cu, shapes

    def plan(self, handle, c, launch=0):
        values, per_cu, _ = handle
        return dict(zip(self.names, plan_call(self.lib, len(self.names), values, per_cu, c, launch)))


@pytest.fixture(scope="module")
def planner():
    return Planner()


def test_field_names(planner):
    assert planner.names == spec.FIELDS


def test_the_handles_of_the_sweep_are_the_ones_meant(planner):
    shape = lambda E, N=8: planner.handle(E, N)[2][0]
    s = shape(2304)
    assert s["paced"] == 1 and s["ring_when_paced"] == 1
    s = shape(4096)
    assert (s["num_blocks"], s["pace_min_k"], s["adapt_min_k"], s["step_ok"], s["paced"]) == (256, 16, 64, 1, 1)
    s = shape(17768)
    assert (s["num_blocks"], s["resident_blocks"], s["pace_min_k"], s["adapt_min_k"]) == (1111, 1024, 4, 16)
    assert s["step_bytes"] == 21_250_048
    s = shape(65536)
    assert (s["num_blocks"], s["resident_blocks"]) == (4096, 1024)
    assert planner.handle(4096, 8)[2][1]["paced"] == 0           # the no-rows shape is never paced


# ---- the sweep ---------------------------------------------------------------------------------------------------------
def sweep_calls(shapes):
    """Every combination of the call's dimensions and the tunables for one handle."""
    ks = {1, 2, 15, 16, 17}
    for s in shapes:
        for m in (s["pace_min_k"], s["adapt_min_k"]):
            ks |= {m - 1, m, m + 1}
    ks = sorted(k for k in ks if k >= 1)
    return itertools.product(ks, DRIVES, (1, 0), (0, 1), (0, 1), (0, 1),            # K, drive, rows, capturing, masks, reset rows
                             (0, 1, 2), (0, 1, 2), (0, 1), (-1, 0), (0, 1, 2, 7), (0, 1))
    # hand2, round_launches, small_shape, step_kernel, max_launch_steps, reset_obs_fused


# The full product is ~400 000 calls per handle.  Every STRIDE-th combination is taken, from a different offset per handle:
# STRIDE is prime and larger than every dimension, so consecutive picks differ in several dimensions at once and every pair
# of values of two dimensions comes up; the coverage assertions below say what the picks must reach.
STRIDE = 41
HANDLES = [(2304, 8), (4096, 8), (17768, 8), (20000, 8), (65536, 8), (100003, 8), (100003, 5), (17776, 5), (4194303, 64),
           (4194303, 63)]


def test_planner_equals_the_spec_over_the_sweep(planner):
    spec.reached.clear()
    seen = {n: set() for n in spec.FIELDS}
    wrong, count = [], 0
    for hi, (E, N) in enumerate(HANDLES):
        handle = planner.handle(E, N)
        shapes = handle[2]
        for combo in itertools.islice(sweep_calls(shapes), hi % STRIDE, None, STRIDE):
            K, drive, rows, capturing, masks, reset, hand2, rounds, small, stepk, mls, rof = combo
            c = call(K, drive, rows, capturing, masks, reset, hand2=hand2, round_launches=rounds, small_shape=small,
                     step_kernel=stepk, max_launch_steps=mls, reset_obs_fused=rof)
            first = spec.plan(E, N, shapes, c, 0)
            for launch in sorted({0, max(first["launches"] - 1, 0)}):
                want = first if launch == 0 else spec.plan(E, N, shapes, c, launch)
                got = planner.plan(handle, c, launch)
                count += 1
                for n in spec.FIELDS:
                    seen[n].add(want[n])
                if got != want and len(wrong) < 5:
                    wrong.append(((E, N), c, launch, {n: (got[n], want[n]) for n in spec.FIELDS if got[n] != want[n]}))
    assert not wrong, wrong
    assert count > 50_000
    # coverage: both sides of every decision of the spec, more than one value of every field
    missed = [(d, side) for d in spec.DECISIONS for side in (True, False) if not spec.reached[d, side]]
    assert not missed, missed
    constant = [n for n in spec.FIELDS if len(seen[n]) < 2]
    assert not constant, constant


# ---- anchors: worked out by hand from the rules ----------------------------------------------------------------------------
def check(planner, E, N, c, launch=0, **want):
    handle = planner.handle(E, N)
    got = planner.plan(handle, c, launch)
    assert got == spec.plan(E, N, handle[2], c, launch)
    assert {n: got[n] for n in want} == want, (E, N, c, launch)


def test_anchor_balanced_rounds_17768(planner):
    # 1111 workgroups on 1024 slots: the second round is 87 < 0.3 x 1024 full, and
    # 21 250 048 / 7000 x 0.5 x 1111 / 1024 = 1647 >= 1200: balanced rounds wherever the launch is paced (pace_min_k = 4)
    assert 1111 - 1024 == 87 < 0.3 * 1024 and round(21_250_048 / 7000 * 0.5 * 1111 / 1024) == 1647
    policy = DRIVES[2]
    check(planner, 17768, 8, call(3, policy), kernel=1, paced=0, by_rounds=0, per_round=1111, rounds=1)
    check(planner, 17768, 8, call(4, policy), kernel=1, paced=1, by_rounds=1, per_round=556, rounds=2)   # block_base 0, 556: 556 + 555
    assert 1111 - 556 == 555
    for K in (3, 4, 64):
        check(planner, 17768, 8, call(K, policy, round_launches=0), by_rounds=0, rounds=1)
    check(planner, 17768, 8, call(3, policy, round_launches=2), by_rounds=1, per_round=556, rounds=2)


def test_anchor_rounds_by_size_65536(planner):
    assert 43 * spec.obs_step_bytes(65536, 8) == 3_426_746_368 and 44 * spec.obs_step_bytes(65536, 8) == 3_506_438_144
    check(planner, 65536, 8, call(43), kernel=1, by_rounds=0, per_round=4096, rounds=1, launches=1)
    check(planner, 65536, 8, call(44), kernel=1, by_rounds=1, per_round=1024, rounds=4, launches=1)


def test_anchor_cuts(planner):
    # 4 GiB per stream: 0xFFFFFFFF // (100 003 x 8 x 16) = 335 -> 334 steps per launch
    check(planner, 100003, 8, call(500), steps_per_launch=334, launches=2, k=334, refused=0)
    check(planner, 100003, 8, call(500), launch=1, k=166)
    # ... with 5 agents 536 -> 535, and E x N odd: even launches
    check(planner, 100003, 5, call(1000), steps_per_launch=534, launches=2, k=534)
    check(planner, 100003, 5, call(1000), launch=1, k=466)
    check(planner, 100003, 5, call(1000, rows=0), steps_per_launch=535, launches=2, k=535)
    # E x N = 4 194 303 x 64: 2^32 - 1024 bytes in the widest stream of ONE step
    check(planner, 4194303, 64, call(3), steps_per_launch=1, launches=3, k=1, refused=0)
    # ... an odd E x N there cannot be cut with rows, can without, and a single step needs no cut
    check(planner, 4194303, 63, call(2), refused=1, launches=0)
    check(planner, 4194303, 63, call(2, rows=0), refused=0, launches=2, steps_per_launch=1)
    check(planner, 4194303, 63, call(1), refused=0, launches=1)
    check(planner, 100003, 5, call(2, max_launch_steps=1), refused=1, launches=0)
    check(planner, 100003, 5, call(2, max_launch_steps=2), refused=0, launches=1)
    # the mixed entry point: 16 steps per launch whatever max_launch_steps says; step by step without the step kernel
    mixed = DRIVES[4]
    check(planner, 4096, 8, call(40, mixed, max_launch_steps=7), steps_per_launch=16, launches=3, k=16, kernel=0, stepwise=0)
    check(planner, 4096, 8, call(40, mixed, max_launch_steps=7), launch=2, k=8, kernel=0)
    check(planner, 4096, 8, call(40, mixed, step_kernel=0), steps_per_launch=1, launches=40, k=1, kernel=1, stepwise=1)


def test_anchor_kernel_and_pacing_4096(planner):
    rest = dict(paced=0, adaptive=0, pace_adapt=0, flip_slot=0, hand_flags=0, by_rounds=0)
    check(planner, 4096, 8, call(16), kernel=0, **rest)
    check(planner, 4096, 8, call(17), kernel=1, shape=0, paced=1, adaptive=0, hand_flags=0, flip_slot=0)
    check(planner, 4096, 8, call(64), kernel=1, paced=1, adaptive=1, pace_adapt=1, flip_slot=1, hand_flags=0)
    check(planner, 4096, 8, call(64, capturing=1), kernel=1, paced=1, adaptive=1, pace_adapt=0, flip_slot=0)
    check(planner, 4096, 8, call(15, DRIVES[2]), kernel=1, paced=0, hand_flags=1)
    check(planner, 4096, 8, call(64, rows=0), kernel=1, shape=1, paced=0, adaptive=0, hand_flags=1, flip_slot=0)
    check(planner, 4096, 8, call(64, rows=0, small_shape=0), kernel=1, shape=0, paced=0, hand_flags=1)
    check(planner, 4096, 8, call(16, step_kernel=0), kernel=1, paced=1, hand_flags=0)
    check(planner, 2304, 8, call(64), kernel=1, paced=1, hand_flags=1)         # ring when paced
    check(planner, 2304, 8, call(64, hand2=0), kernel=1, paced=1, hand_flags=0)


def test_anchor_what_the_step_launch_fuses(planner):
    both = dict(masks=1, reset=1)
    check(planner, 4096, 8, call(1, **both), kernel=0, masks_fused=1, reset_obs_fused=1)
    check(planner, 4096, 8, call(1, DRIVES[1], **both), kernel=0, masks_fused=0, reset_obs_fused=0)       # a move order
    check(planner, 4096, 8, call(2, **both), kernel=0, masks_fused=0, reset_obs_fused=0)
    check(planner, 4096, 8, call(2, max_launch_steps=1, **both), kernel=0, k=1, masks_fused=0, reset_obs_fused=0)   # cut into single steps
    check(planner, 4096, 8, call(1, DRIVES[4], **both), kernel=0, masks_fused=1, reset_obs_fused=0)       # mixed: never the rows
    check(planner, 4096, 8, call(1, reset_obs_fused=0, **both), kernel=0, masks_fused=1, reset_obs_fused=0)
    check(planner, 4096, 8, call(1, masks=0, reset=0), kernel=0, masks_fused=0, reset_obs_fused=0)
    check(planner, 4096, 8, call(1, step_kernel=0, **both), kernel=1, masks_fused=0, reset_obs_fused=0)
