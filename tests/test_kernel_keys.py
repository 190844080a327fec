"""Which instantiation of rollout_kernel, step_kernel and observe_kernel a call launches, on a machine without a GPU: the pure
planner (ccxi_plan, ccxi_plan_call) and the key functions the launch code itself switches on (csrc/ccx_keys.h, through
ccxi_call_key / ccxi_call_keys / ccxi_observe_key) swept over the legal space that tests/_kernel_keys.py states, against
that file's catalogue (CASES), its list of compiled instantiations that are never selected (UNREACHABLE) and the counts
DESIGN.md quotes.  tests/test_gpu_kernel_keys.py runs every case of the catalogue."""

import ctypes as C
import itertools

import numpy as np
import pytest

import _kernel_keys as kk
from _shape_plan import gen

# DESIGN.md 4, "Instantiations": compiled, reachable with the library's defaults, only through a setting (the launch shape,
# the occ_tables or the step_kernel tunable), never
COUNTS = {"compiled": 406, "default": 326, "setting_only": 0, "unreachable": 80}


@pytest.fixture(scope="module")
def lib():
    from collectivecrossing_amd import _lib

    if not _lib.LIB_PATH.exists():
        pytest.skip("libccx.so not built (run __graft_entry__.build())")
    lib = C.CDLL(str(_lib.LIB_PATH))
    lib.names = gen.bind(lib)
    kk.bind_keys(lib)
    return lib


@pytest.fixture(scope="module")
def reached(lib):
    return kk.sweep_keys(lib, lib.names)


def _names(keys):
    return sorted(kk.describe(k) for k in keys)


def test_the_sweep_reaches_the_catalogue_and_nothing_else(reached):
    catalogue = {c[0] for c in kk.CASES}
    assert not reached - catalogue, f"reached by the sweep, no case in the catalogue: {_names(reached - catalogue)}"
    assert not catalogue - reached, f"in the catalogue, never reached by the sweep: {_names(catalogue - reached)}"


def test_every_representative_selects_its_key(lib):
    for case in kk.CASES:
        assert kk.key_of_case(lib, case) == case[0], (case, kk.describe(kk.key_of_case(lib, case)))


def test_every_compiled_instantiation_is_reached_or_listed_as_unreachable(reached):
    compiled = kk.compiled_keys()
    assert reached <= compiled, f"selected but not compiled: {_names(reached - compiled)}"
    listed = set(kk.UNREACHABLE)
    assert not listed & reached, f"listed as unreachable, reached by the sweep: {_names(listed & reached)}"
    assert not compiled - reached - listed, f"compiled, never selected and not listed: {_names(compiled - reached - listed)}"
    assert listed <= compiled, f"listed as unreachable, not compiled at all: {_names(listed - compiled)}"
    assert all(isinstance(why, str) and len(why) > 20 for why in kk.UNREACHABLE.values())


def test_the_counts_the_design_document_quotes(lib, reached):
    default = kk.sweep_keys(lib, lib.names, defaults_only=True)
    assert default <= reached
    got = {"compiled": len(kk.compiled_keys()), "default": len(default), "setting_only": len(reached - default),
           "unreachable": len(kk.UNREACHABLE)}
    assert got == COUNTS
    assert got["default"] + got["setting_only"] + got["unreachable"] == got["compiled"]
    # per kernel: rollout 224, step 168, observe 14 compiled
    per = {k: sum(1 for key in kk.compiled_keys() if key[0] == k) for k in kk.KERNEL_NAMES}
    assert per == {kk.KERNEL_ROLLOUT: 224, kk.KERNEL_STEP: 168, kk.KERNEL_OBSERVE: 14}


def test_no_key_depends_on_the_occupancy_figure(lib):
    """blocks_per_cu 1..8 for both shapes (and the two most unequal pairs) on a sub-space that keeps every grid class, lane
    group, tile filling and setting: the keys of every call of the space, launch by launch, are those of the figure 2."""
    handles = [(w, h, n, e, lanes, occ, 0, tt)
               for (w, h) in ((4, 4), (12, 8), (64, 48), (100, 100)) for n in (1, 2, 3, 7, 8, 12, 33, 50, 64) if n in kk.agent_counts(w, h)
               for e in (3, 129, 4096, 65536) for lanes, occ, tt in itertools.product((0, 64), (-1, 0, 1), (0, 1))]
    assert len(handles) > 1000
    for handle in handles:
        pin = kk.plan_in(*handle)
        base = kk.keys_of_handle(lib, pin, (2, 2))
        for per_cu in [(b, b) for b in range(1, 9)] + [(1, 8), (8, 1)]:
            assert np.array_equal(kk.keys_of_handle(lib, pin, per_cu), base), (handle, per_cu)


def test_the_space_is_the_one_the_catalogue_states():
    assert kk.GRIDS[0] == (4, 4) and kk.GRIDS[-1] == (100, 100) and {(12, 8), (20, 12), (32, 16)} <= set(kk.GRIDS)
    assert min(kk.ENVS) == 1 and max(kk.ENVS) == 65536 and any(e % 8 for e in kk.ENVS)
    assert kk.KS == [1, 2, 16, 17, 64]
    space = kk.call_space()
    calls = [dict(zip(kk.CALL_FIELDS, c)) for c, _ in space]
    assert {(c["actions"], c["order"], c["policy"], c["actions_out"], c["mixed"]) for c in calls} == set(kk.DRIVES)
    assert {c["step_kernel"] for c in calls} == {-1, 0, 1} and {c["K"] for c in calls} == set(kk.KS)
    assert {c["masks_bound"] for c in calls} == {0, 1} == {c["reset_obs_on"] for c in calls}
    assert {f[5] for _, f in space} == {0, 16} and {f[0] for _, f in space} == {0, 1}
    assert list(kk.agent_counts(4, 4)) == [1, 2, 3, 4] and list(kk.agent_counts(100, 100))[-1] == 64


# cases per (kernel, GLOG): one parametrised GPU test each (the rollout kernel's split by OUT mode); 1092 in all
CASE_COUNTS = {(0, 0): 14, (0, 1): 14, (0, 2): 28, (0, 3): 28, (0, 4): 28, (0, 5): 28, (0, 6): 28, (1, 0): 70, (1, 1): 70, (1, 2): 140,
               (1, 3): 140, (1, 4): 172, (1, 5): 156, (1, 6): 164, (2, 0): 1, (2, 1): 1, (2, 2): 2, (2, 3): 2, (2, 4): 2, (2, 5): 2, (2, 6): 2}


def test_no_case_has_left_the_catalogue():
    got = {}
    for c in kk.CASES:
        got[c[0][0], c[0][1]] = got.get((c[0][0], c[0][1]), 0) + 1
    assert got == CASE_COUNTS and len(kk.CASES) == len(set(kk.CASES)) == 1092


def test_every_variant_the_gpu_test_runs_is_in_the_catalogue(lib):
    """Every rollout key at both tile fillings where both exist, every PLAIN = false key with each cause alone, every OUT 2 key
    with each of its causes, every rollout key that a forcing occ_tables setting reaches once that way, and per kernel and
    (GLOG, PAIR) a case with actions_out next to the other outputs and one with actions_out alone."""
    by_key, by_group = {}, {}
    for c in map(kk.case_dict, kk.CASES):
        if c["variant"].startswith("actions_out"):
            by_group.setdefault(c["key"][:3], set()).add(c["variant"])
            drive = kk.DRIVE_NAMES[c["drive"]][0]
            assert drive[3] == 1 and (c["outputs"] == "none") == (c["variant"] == "actions_out_only"), c
            assert c["key"][0] == kk.KERNEL_STEP and c["key"][5] or c["key"][0] == kk.KERNEL_ROLLOUT and not c["key"][5], c
            if c["key"][0] == kk.KERNEL_ROLLOUT and c["outputs"] == "none":
                assert c["key"][3] == 1, c                               # (actions_out alone asks for outputs: OUT 1)
        else:
            by_key.setdefault(c["key"], set()).add(c["variant"])
    groups = {k[:3] for k in by_key if k[0] != kk.KERNEL_OBSERVE}
    assert len(groups) == 24 and all(by_group.get(g) == {"actions_out", "actions_out_only"} for g in groups), by_group
    forced = kk.forced_occ_keys(lib, lib.names)
    assert {k[4] for k in forced} == {0, 1}                              # tables given up where they fit, kept where the planner drops them
    for key, variants in by_key.items():
        if key[0] != kk.KERNEL_ROLLOUT:
            assert variants == {""}, (key, variants)
            continue
        assert ("occ_forced" in variants) == (key in forced), (key, variants)
        for c in map(kk.case_dict, kk.CASES):
            if c["key"] == key and c["variant"] == "occ_forced":
                assert c["occ_tables"] == key[4] and kk.occ_is_forced(
                    lib, lib.names, (*c["grid"], c["N"], c["E"], c["lanes"], c["occ_tables"], int(c["tables"] == "reward"),
                                     int(c["tables"] == "terminated"))), c
        variants = variants - {"occ_forced"}
        # (the planner's own filling reaches these two families only in batches beyond the generator's reduced space)
        full_only = key[1:4] in ((4, 0, 3), (5, 1, 3))
        assert {v.split("/")[0] for v in variants} == ({"full"} if full_only else {"default", "full"}), (key, variants)
        if not key[5]:                                                   # not PLAIN
            causes = {v.split("/")[1] for v in variants}
            assert causes == {"order", "policy", "tables"}, (key, variants)
        if key[3] == 2:
            # An aligned slab at residue 16 needs a tile region of whole 128-byte lines: EW N (6 + 4N) 4 = 8 EW N (3 + 2N) bytes.
            # For odd N both N and 3 + 2N are odd, so EW must be a multiple of 16 -- and a lane group of 8 or more (GLOG >= 3)
            # has at most 8 envs to a tile: those keys are OUT 2 through "off_lines" alone.
            never_aligned = key[2] == 0 and key[1] >= 3
            assert {v.split("/")[-1] for v in variants} == ({"off_lines"} if never_aligned else {"off_lines", "residue16"}), (key, variants)
