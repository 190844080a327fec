"""Which instantiation of the three stepping kernels a call launches: the bindings of the key functions
(csrc/ccx_keys.h), the sweep of the pure planner and key functions over the legal space, the representative case of every
key the sweep reaches, and the list of compiled instantiations it never reaches.

    rollout_kernel / rollout_kernel_v128 <GLOG 0..6, PAIR, OUT 0..3, OCC, PLAIN>       7 x 2 x 4 x 2 x 2 = 224 compiled
    step_kernel <GLOG, PAIR, K1, ORD, POL, MSK, RSO>         7 x 2 x (8 of K1 ORD POL + 2 MSK + 2 RSO) = 168 compiled
    observe_kernel <GLOG, PAIR>                                                                  14 compiled

A key is ``(kernel, v0 .. v6)``: the kernel (KERNEL_*) and its template arguments in the order of the template's parameter
list, zero-padded -- what ``ccxi_call_key`` returns and what ``ccxi_handle_last_key`` reports of a live handle.

THE SWEEP (``sweep_keys``).  Handles: the grids of GRIDS (4 x 4 up to 100 x 100, the benchmark geometries 12 x 8, 20 x 12
and 32 x 16 among them) x every agent count 1..64 that ``strict_reference_limits=False`` admits on the grid
(N <= min(W H // 4, 64)) x the batch sizes of ENVS (1 .. 65 536, ragged ones among them) x the tile filling (the planner's
own, or ``ccx_set_launch_shape(64, 0)``) x the ``occ_tables`` tunable (-1, 0, 1) x user tables (none, a terminated table,
a reward table where the planner says it fits).  Calls on every handle: every entry of ``_shape_plan.DRIVES`` x K in
{1, 2, 16, 17, 64} x the ``step_kernel`` tunable (-1, 0, 1) x the outputs (none; rewards, flags and compact rows; those
and observation rows at residue 0 and at residue 16 of a 128-byte line) x masks bound or not x reset-obs on or off (the
last two where the entry point passes them on: masks on ccx_step / ccx_rollout / ccx_rollout_mixed, reset-obs on ccx_rollout
with rows or compact rows).  Every call is planned with both of the handle's shapes (rows and no rows) and contributes the
key of its first and of its last launch.  The occupancy figure is 2 workgroups per CU for both shapes; a sub-sweep feeds 1..8
and shows that no key depends on it (tests/test_kernel_keys.py).
"""

from __future__ import annotations

import ctypes as C
import itertools

import numpy as np

from _shape_plan import CALL_FIELDS, DRIVES, TUNABLE_DEFAULTS, CallIn, gen

KERNEL_STEP, KERNEL_ROLLOUT, KERNEL_OBSERVE = 0, 1, 2
KERNEL_NAMES = {KERNEL_STEP: "step", KERNEL_ROLLOUT: "rollout", KERNEL_OBSERVE: "observe"}
FACT_FIELDS = ["obs", "reward", "agent_flags", "env_flags", "obs_compact", "obs_residue"]


class Key(C.Structure):
    _fields_ = [("kernel", C.c_int32), ("v", C.c_int32 * 7)]

    def tuple(self):
        return (int(self.kernel), *[int(x) for x in self.v])


class KeyFacts(C.Structure):
    _fields_ = [(n, C.c_int32) for n in FACT_FIELDS]


CALL_DTYPE = np.dtype([(n, np.int32) for n in CALL_FIELDS])
FACT_DTYPE = np.dtype([(n, np.int32) for n in FACT_FIELDS])
assert CALL_DTYPE.itemsize == C.sizeof(CallIn) and FACT_DTYPE.itemsize == C.sizeof(KeyFacts)


def bind_keys(lib):
    lib.ccxi_call_key.restype = C.c_int
    lib.ccxi_call_key.argtypes = [C.POINTER(gen.PlanIn), C.POINTER(C.c_int), C.POINTER(CallIn), C.POINTER(KeyFacts), C.c_int,
                                  C.POINTER(Key)]
    lib.ccxi_call_keys.restype = C.c_int
    lib.ccxi_call_keys.argtypes = [C.POINTER(gen.PlanIn), C.POINTER(C.c_int), C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
    lib.ccxi_observe_key.restype = C.c_int
    lib.ccxi_observe_key.argtypes = [C.POINTER(gen.PlanIn), C.POINTER(Key)]
    lib.ccxi_handle_last_key.restype = C.c_int
    lib.ccxi_handle_last_key.argtypes = [C.c_void_p, C.c_int, C.POINTER(Key)]


# ---- the space ---------------------------------------------------------------------------------------------------------
GRIDS = [(4, 4), (6, 16), (12, 8), (20, 12), (32, 16), (40, 30), (64, 48), (100, 100)]
ENVS = [1, 3, 33, 100, 129, 511, 1000, 4096, 10001, 65536]
KS = [1, 2, 16, 17, 64]
# outputs of a call: (obs, reward, agent_flags, env_flags, obs_compact, obs_residue)
OUTPUTS = {"none": (0, 0, 0, 0, 0, 0), "small": (0, 1, 1, 1, 1, 0), "rows": (1, 1, 1, 1, 1, 0), "rows16": (1, 1, 1, 1, 1, 16)}
NUM_CUS = 256
# how a case is driven: name -> (entry of _shape_plan.DRIVES, in-kernel / scripted policy or None)
DRIVE_NAMES = {"tensor": (DRIVES[0], None), "order": (DRIVES[1], None), "greedy": (DRIVES[2], "greedy"),
               "greedy_actions_out": (DRIVES[3], "greedy"), "mixed": (DRIVES[4], "greedy"), "mixed_order": (DRIVES[5], "greedy"),
               "mixed_all_actions_out": (DRIVES[6], "greedy")}


def agent_counts(w, h):
    return range(1, min(w * h // 4, 64) + 1)


def plan_in(w, h, n, e, lanes=0, occ_tables=-1, reward_table=0, term_table=0):
    d = gen.plan_inputs(w, h, n, e, None, 0, NUM_CUS, 1)
    d.update(lanes_per_wave=lanes, occ_tables=occ_tables, reward_table=reward_table, term_table=term_table)
    return gen.PlanIn(*[float(d[f]) if f == "pace_start_ns" else int(d[f]) for f in gen.IN_FIELDS])


def call_in(K, drive, masks=0, reset=0, step_kernel=-1, **tunables):
    actions, order, policy, actions_out, mixed = drive
    d = dict(TUNABLE_DEFAULTS, K=K, actions=actions, order=order, policy=policy, actions_out=actions_out, mixed=mixed,
             writes_obs=0, capturing=0, masks_bound=masks, reset_obs_on=reset, step_kernel=step_kernel, **tunables)
    return tuple(int(d[n]) for n in CALL_FIELDS)


def call_space():
    """Every (call, outputs) of the sweep that an entry point can make: (call tuple, facts tuple)."""
    out = []
    for drive, K, sk, (oname, facts) in itertools.product(DRIVES, KS, (-1, 0, 1), OUTPUTS.items()):
        _actions, _order, policy, _actions_out, mixed = drive
        for masks, reset in itertools.product((0, 1), (0, 1)):
            if masks and policy:
                continue                  # ccx_rollout_policy does not hand the bound masks to its launches
            if reset and (policy or mixed or oname == "none"):
                continue                  # only ccx_rollout passes the restarted rows on, and only with rows or compact rows
            out.append((call_in(K, drive, masks, reset, sk), facts))
    return out


_SPACE = None


def _space_arrays():
    global _SPACE
    if _SPACE is None:
        space = call_space()
        calls = np.array([c for c, _ in space], dtype=np.int32).view(CALL_DTYPE).reshape(-1)
        facts = np.array([f for _, f in space], dtype=np.int32).view(FACT_DTYPE).reshape(-1)
        _SPACE = (space, np.ascontiguousarray(calls), np.ascontiguousarray(facts))
    return _SPACE


def keys_of_handle(lib, pin, per_cu=(2, 2)):
    """int32 [n calls, 2 (first, last launch), 8]: the keys of every call of the space on the handle planned from ``pin``."""
    _, calls, facts = _space_arrays()
    out = np.empty((len(calls), 2, 8), np.int32)
    rc = lib.ccxi_call_keys(C.byref(pin), (C.c_int * 2)(*per_cu), calls.ctypes.data, facts.ctypes.data, len(calls), out.ctypes.data)
    assert rc == 0
    return out


def reward_table_fits(lib, nfields, names, w, h, n, e, lanes, occ):
    """ccx_set_reward_table's own rule (ccx_plan.hip: reward_table_fits): both shapes stay within 150 KiB of LDS."""
    i = names.index("lds_bytes")
    for rows in (1, 0):
        d = gen.plan_inputs(w, h, n, e, None, 0, NUM_CUS, rows)
        d.update(lanes_per_wave=lanes, occ_tables=occ, reward_table=1)
        if gen.plan_row(lib, nfields, [d[f] for f in gen.IN_FIELDS], 2)[i] > 150 * 1024:
            return False
    return True


def handle_space(lib, names):
    """(w, h, n, e, lanes, occ_tables, reward_table, term_table) of every handle of the sweep."""
    for (w, h) in GRIDS:
        for n in agent_counts(w, h):
            for e in ENVS:
                if e * n >= 1 << 28:
                    continue
                for lanes, occ in itertools.product((0, 64), (-1, 0, 1)):
                    yield (w, h, n, e, lanes, occ, 0, 0)
                    yield (w, h, n, e, lanes, occ, 0, 1)
                    if reward_table_fits(lib, len(names), names, w, h, n, e, lanes, occ):
                        yield (w, h, n, e, lanes, occ, 1, 0)


def occ_is_forced(lib, names, handle):
    """The occ_tables tunable of the handle is set AND changes what the planner would have chosen, for both of its shapes:
    every rollout launch of such a handle runs its key "the other way" (tables given up where they fit, kept where the planner
    gives them up)."""
    w, h, n, e, lanes, occ, rt, tt = handle
    if occ == -1:
        return False
    i = names.index("occ")
    for rows in (1, 0):
        got = []
        for o in (occ, -1):
            d = gen.plan_inputs(w, h, n, e, None, 0, NUM_CUS, rows)
            d.update(lanes_per_wave=lanes, occ_tables=o, reward_table=rt, term_table=tt)
            got.append(gen.plan_row(lib, len(names), [d[f] for f in gen.IN_FIELDS], 2)[i])
        if got[0] == got[1]:
            return False
    return True


def forced_occ_keys(lib, names):
    """The rollout keys that handles of the sweep with a forcing occ_tables setting (occ_is_forced) reach."""
    seen = set()
    for handle in handle_space(lib, names):
        if occ_is_forced(lib, names, handle):
            seen.update(np.unique(pack(keys_of_handle(lib, plan_in(*handle)))).tolist())
    return {k for k in map(unpack, seen) if k[0] == KERNEL_ROLLOUT}


_PACK = np.array([1 << 24, 1 << 20, 1 << 16, 1 << 12, 1 << 8, 1 << 4, 1 << 2, 1], np.int64)   # (kernel + 1, v0 .. v6): a key as one integer


def pack(keys):
    k = keys.astype(np.int64)
    k[..., 0] += 1
    return k @ _PACK


def unpack(p):
    p = int(p)
    return ((p >> 24) - 1, (p >> 20) & 15, (p >> 16) & 15, (p >> 12) & 15, (p >> 8) & 15, (p >> 4) & 15, (p >> 2) & 3, p & 3)


def sweep_keys(lib, names, defaults_only=False, per_cu=(2, 2)):
    """The set of keys the space reaches, the observe kernel's included.  ``defaults_only``: what is left of the space with
    the planner's own tile filling and both tunables at -1."""
    space, _, _ = _space_arrays()
    rows = np.array([c[CALL_FIELDS.index("step_kernel")] == -1 for c, _ in space]) if defaults_only else slice(None)
    seen = set()
    k = Key()
    for handle in handle_space(lib, names):
        if defaults_only and (handle[4] != 0 or handle[5] != -1):
            continue
        pin = plan_in(*handle)
        assert lib.ccxi_observe_key(C.byref(pin), C.byref(k)) == 0
        seen.add(int(pack(np.array(k.tuple(), np.int32))))
        seen.update(np.unique(pack(keys_of_handle(lib, pin, per_cu)[rows])).tolist())
    return {unpack(p) for p in seen if (p >> 24) > 0}           # (kernel -1: a refused call)


# ---- what is compiled --------------------------------------------------------------------------------------------------
def compiled_keys():
    ks = set()
    for g, pair in itertools.product(range(7), (0, 1)):
        ks.add((KERNEL_OBSERVE, g, pair, 0, 0, 0, 0, 0))
        for out, occ, plain in itertools.product(range(4), (0, 1), (0, 1)):
            ks.add((KERNEL_ROLLOUT, g, pair, out, occ, plain, 0, 0))
        for k1, ord_, pol in itertools.product((0, 1), (0, 1), (0, 1)):          # ccx_step.hip: pick
            ks.add((KERNEL_STEP, g, pair, k1, ord_, pol, 0, 0))
        for pol in (0, 1):                                                       # pick_msk
            ks.add((KERNEL_STEP, g, pair, 1, 0, pol, 1, 0))
        for msk in (0, 1):                                                       # pick_rso
            ks.add((KERNEL_STEP, g, pair, 1, 0, 0, msk, 1))
    return ks


def describe(key):
    k, v = key[0], key[1:]
    if k == KERNEL_ROLLOUT:
        return f"rollout<GLOG {v[0]}, PAIR {v[1]}, OUT {v[2]}, OCC {v[3]}, PLAIN {v[4]}>"
    if k == KERNEL_STEP:
        return f"step<GLOG {v[0]}, PAIR {v[1]}, K1 {v[2]}, ORD {v[3]}, POL {v[4]}, MSK {v[5]}, RSO {v[6]}>"
    return f"observe<GLOG {v[0]}, PAIR {v[1]}>"


# ---- what is never selected -----------------------------------------------------------------------------------------------
def _unreachable():
    """{key: reason} of every compiled instantiation that no call of the sweep selects.  The first two rules are structural
    (the lane group is ceil(log2 N) and PAIR is "N even"); the OUT 3 rules follow from the size of a tile: OUT 3 needs more
    store iterations per row writer than the kernel caches addresses for (csrc/ccx_keys.h: kFastObsIters = 10), a tile holds
    EW x N <= 64 agents, so it has ceil(EW N (3 + 2N) / 64) iterations of float2 units, half of that for even N."""
    u = {}
    rollout = [(out, occ, plain) for out in range(4) for occ in (0, 1) for plain in (0, 1)]
    step = [k for k in compiled_keys() if k[0] == KERNEL_STEP and k[1] == 0 and k[2] == 0]
    for glog, pair, why in ((0, 1, "GLOG 0 is N = 1, which is odd: never PAIR"), (1, 0, "GLOG 1 is N = 2, which is even: always PAIR")):
        u[(KERNEL_OBSERVE, glog, pair, 0, 0, 0, 0, 0)] = why
        for out, occ, plain in rollout:
            u[(KERNEL_ROLLOUT, glog, pair, out, occ, plain, 0, 0)] = why
        for k in step:
            u[(KERNEL_STEP, glog, pair) + k[3:]] = why
    few = {(0, 0): "N = 1: at most 64 x 5 / 64 = 5 store iterations per tile, never more than 10 per row writer",
           (1, 1): "N = 2: at most 32 x 2 x 7 / 2 / 64 = 4 store iterations per tile",
           (2, 0): "N = 3: at most 16 x 3 x 9 / 64 = 7 store iterations per tile",
           (2, 1): "N = 4: at most 16 x 4 x 11 / 2 / 64 = 6 store iterations per tile",
           (3, 1): "N = 6: at most 8 x 6 x 15 / 2 / 64 = 6 store iterations per tile; N = 8: 10, and its slab (8 x 38 floats per "
                   "env) is a whole number of 128-byte lines whatever E is"}
    for (glog, pair), why in few.items():
        for occ, plain in itertools.product((0, 1), (0, 1)):
            u[(KERNEL_ROLLOUT, glog, pair, 3, occ, plain, 0, 0)] = "OUT 3 needs long rows. " + why
    for plain in (0, 1):
        # (a rule of the planner, not of the kernel: the sweep is what says so)
        u[(KERNEL_ROLLOUT, 3, 0, 3, 1, plain, 0, 0)] = (
            "OUT 3 needs long rows. N = 5: at most 8 x 5 x 13 / 64 = 9 iterations; N = 7: 15, more than 10 only for ONE row "
            "writer on full tiles of 8 envs, a shape the planner plans only for batches whose occupancy tables it has given up")
    return u


UNREACHABLE = _unreachable()

# ---- the catalogue ----------------------------------------------------------------------------------------------------------
# One case per reachable key and variant, as tests/golden/gen_kernel_key_cases.py printed them (its docstring says what
# "smallest" means): (key, (W, H), N, E, K, drive (DRIVE_NAMES), outputs (OUTPUTS), user tables ("none", "terminated",
# "reward"), masks bound, reset-obs on, lanes_per_wave of ccx_set_launch_shape (0: the planner's own), occ_tables tunable,
# step_kernel tunable, variant).  The variant of a rollout key: the tile filling ("default": the planner's own, one env per
# wave at these batch sizes; "full": 64 lanes), then for PLAIN = false the ONE cause of it ("order", "policy", "tables"), then for
# OUT 2 the cause of that ("off_lines": a slab or tile region that is not a multiple of 128 bytes; "residue16": an aligned slab
# whose obs array lies at residue 16; keys of odd N at GLOG >= 3 have no such variant: a tile region of at most 8 envs with odd N
# is 8 x odd bytes per env and never a whole number of lines).  A "policy" case runs twice on the GPU: the greedy and the waiting
# policy.  "occ_forced": the key reached through an occ_tables setting that overrides the planner's own choice on that handle
# (occ_is_forced: tables given up on a grid where they fit, kept where the planner gives them up) -- one per rollout key that the
# sweep reaches that way.  "actions_out" / "actions_out_only": the policy-carrying keys (rollout kernel not PLAIN, step kernel
# POL) with the chosen actions as an output, next to every other output and as the ONLY one (which alone makes the rollout
# kernel write: OUT 1) -- one of each per kernel and (GLOG, PAIR).
CASE_FIELDS = ("key", "grid", "N", "E", "K", "drive", "outputs", "tables", "masks", "reset", "lanes", "occ_tables", "step_kernel", "variant")
CASES = [
    ((0, 0, 0, 0, 0, 0, 0, 0), (4, 4), 1, 3, 3, 'tensor', 'rows', 'none', 0, 0, 0, -1, -1, ''),
    ((0, 0, 0, 0, 0, 1, 0, 0), (4, 4), 1, 3, 3, 'mixed', 'rows', 'none', 0, 0, 0, -1, -1, ''),
    ((0, 0, 0, 0, 1, 0, 0, 0), (4, 4), 1, 3, 3, 'order', 'rows', 'none', 0, 0, 0, -1, -1, ''),
    ((0, 0, 0, 0, 1, 1, 0, 0), (4, 4), 1, 3, 3, 'mixed_order', 'rows', 'none', 0, 0, 0, -1, -1, ''),
    ((0, 0, 0, 1, 0, 0, 0, 0), (4, 4), 1, 3, 1, 'tensor', 'rows', 'none', 0, 0, 0, -1, -1, ''),
    ((0, 0, 0, 1, 0, 0, 0, 1), (4, 4), 1, 3, 1, 'tensor', 'rows', 'none', 0, 1, 0, -1, -1, ''),
    ((0, 0, 0, 1, 0, 0, 1, 0), (4, 4), 1, 3, 1, 'tensor', 'rows', 'none', 1, 0, 0, -1, -1, ''),
    ((0, 0, 0, 1, 0, 0, 1, 1), (4, 4), 1, 3, 1, 'tensor', 'rows', 'none', 1, 1, 0, -1, -1, ''),
    ((0, 0, 0, 1, 0, 1, 0, 0), (4, 4), 1, 3, 1, 'mixed', 'rows', 'none', 0, 0, 0, -1, -1, ''),
    ((0, 0, 0, 1, 0, 1, 0, 0), (4, 4), 1, 3, 1, 'mixed_all_actions_out', 'rows', 'none', 0, 0, 0, -1, -1, 'actions_out'),
    ((0, 0, 0, 1, 0, 1, 0, 0), (4, 4), 1, 3, 1, 'mixed_all_actions_out', 'none', 'none', 0, 0, 0, -1, -1, 'actions_out_only'),
    ((0, 0, 0, 1, 0, 1, 1, 0), (4, 4), 1, 3, 1, 'mixed', 'rows', 'none', 1, 0, 0, -1, -1, ''),
    ((0, 0, 0, 1, 1, 0, 0, 0), (4, 4), 1, 3, 1, 'order', 'rows', 'none', 0, 0, 0, -1, -1, ''),
    ((0, 0, 0, 1, 1, 1, 0, 0), (4, 4), 1, 3, 1, 'mixed_order', 'rows', 'none', 0, 0, 0, -1, -1, ''),
    ((0, 1, 1, 0, 0, 0, 0, 0), (4, 4), 2, 3, 3, 'tensor', 'rows', 'none', 0, 0, 0, -1, -1, ''),
    ((0, 1, 1, 0, 0, 1, 0, 0), (4, 4), 2, 3, 3, 'mixed', 'rows', 'none', 0, 0, 0, -1, -1, ''),
    ((0, 1, 1, 0, 1, 0, 0, 0), (4, 4), 2, 3, 3, 'order', 'rows', 'none', 0, 0, 0, -1, -1, ''),
    ((0, 1, 1, 0, 1, 1, 0, 0), (4, 4), 2, 3, 3, 'mixed_order', 'rows', 'none', 0, 0, 0, -1, -1, ''),
    ((0, 1, 1, 1, 0, 0, 0, 0), (4, 4), 2, 3, 1, 'tensor', 'rows', 'none', 0, 0, 0, -1, -1, ''),
    ((0, 1, 1, 1, 0, 0, 0, 1), (4, 4), 2, 3, 1, 'tensor', 'rows', 'none', 0, 1, 0, -1, -1, ''),
    ((0, 1, 1, 1, 0, 0, 1, 0), (4, 4), 2, 3, 1, 'tensor', 'rows', 'none', 1, 0, 0, -1, -1, ''),
    ((0, 1, 1, 1, 0, 0, 1, 1), (4, 4), 2, 3, 1, 'tensor', 'rows', 'none', 1, 1, 0, -1, -1, ''),
    ((0, 1, 1, 1, 0, 1, 0, 0), (4, 4), 2, 3, 1, 'mixed', 'rows', 'none', 0, 0, 0, -1, -1, ''),
    ((0, 1, 1, 1, 0, 1, 0, 0), (4, 4), 2, 3, 1, 'mixed_all_actions_out', 'rows', 'none', 0, 0, 0, -1, -1, 'actions_out'),
    ((0, 1, 1, 1, 0, 1, 0, 0), (4, 4), 2, 3, 1, 'mixed_all_actions_out', 'none', 'none', 0, 0, 0, -1, -1, 'actions_out_only'),
    ((0, 1, 1, 1, 0, 1, 1, 0), (4, 4), 2, 3, 1, 'mixed', 'rows', 'none', 1, 0, 0, -1, -1, ''),
    ((0, 1, 1, 1, 1, 0, 0, 0), (4, 4), 2, 3, 1, 'order', 'rows', 'none', 0, 0, 0, -1, -1, ''),
    ((0, 1, 1, 1, 1, 1, 0, 0), (4, 4), 2, 3, 1, 'mixed_order', 'rows', 'none', 0, 0, 0, -1, -1, ''),
    ((0, 2, 0, 0, 0, 0, 0, 0), (4, 4), 3, 3, 3, 'tensor', 'rows', 'none', 0, 0, 0, -1, -1, ''),
    ((0, 2, 0, 0, 0, 1, 0, 0), (4, 4), 3, 3, 3, 'mixed', 'rows', 'none', 0, 0, 0, -1, -1, ''),
    ((0, 2, 0, 0, 1, 0, 0, 0), (4, 4), 3, 3, 3, 'order', 'rows', 'none', 0, 0, 0, -1, -1, ''),
    ((0, 2, 0, 0, 1, 1, 0, 0), (4, 4), 3, 3, 3, 'mixed_order', 'rows', 'none', 0, 0, 0, -1, -1, ''),
    ((0, 2, 0, 1, 0, 0, 0, 0), (4, 4), 3, 3, 1, 'tensor', 'rows', 'none', 0, 0, 0, -1, -1, ''),
    ((0, 2, 0, 1, 0, 0, 0, 1), (4, 4), 3, 3, 1, 'tensor', 'rows', 'none', 0, 1, 0, -1, -1, ''),
    ((0, 2, 0, 1, 0, 0, 1, 0), (4, 4), 3, 3, 1, 'tensor', 'rows', 'none', 1, 0, 0, -1, -1, ''),
    ((0, 2, 0, 1, 0, 0, 1, 1), (4, 4), 3, 3, 1, 'tensor', 'rows', 'none', 1, 1, 0, -1, -1, ''),
    ((0, 2, 0, 1, 0, 1, 0, 0), (4, 4), 3, 3, 1, 'mixed', 'rows', 'none', 0, 0, 0, -1, -1, ''),
    ((0, 2, 0, 1, 0, 1, 0, 0), (4, 4), 3, 3, 1, 'mixed_all_actions_out', 'rows', 'none', 0, 0, 0, -1, -1, 'actions_out'),
    ((0, 2, 0, 1, 0, 1, 0, 0), (4, 4), 3, 3, 1, 'mixed_all_actions_out', 'none', 'none', 0, 0, 0, -1, -1, 'actions_out_only'),
    ((0, 2, 0, 1, 0, 1, 1, 0), (4, 4), 3, 3, 1, 'mixed', 'rows', 'none', 1, 0, 0, -1, -1, ''),
    ((0, 2, 0, 1, 1, 0, 0, 0), (4, 4), 3, 3, 1, 'order', 'rows', 'none', 0, 0, 0, -1, -1, ''),
    ((0, 2, 0, 1, 1, 1, 0, 0), (4, 4), 3, 3, 1, 'mixed_order', 'rows', 'none', 0, 0, 0, -1, -1, ''),
    ((0, 2, 1, 0, 0, 0, 0, 0), (4, 4), 4, 3, 3, 'tensor', 'rows', 'none', 0, 0, 0, -1, -1, ''),
    ((0, 2, 1, 0, 0, 1, 0, 0), (4, 4), 4, 3, 3, 'mixed', 'rows', 'none', 0, 0, 0, -1, -1, ''),
    ((0, 2, 1, 0, 1, 0, 0, 0), (4, 4), 4, 3, 3, 'order', 'rows', 'none', 0, 0, 0, -1, -1, ''),
    ((0, 2, 1, 0, 1, 1, 0, 0), (4, 4), 4, 3, 3, 'mixed_order', 'rows', 'none', 0, 0, 0, -1, -1, ''),
    ((0, 2, 1, 1, 0, 0, 0, 0), (4, 4), 4, 3, 1, 'tensor', 'rows', 'none', 0, 0, 0, -1, -1, ''),
    ((0, 2, 1, 1, 0, 0, 0, 1), (4, 4), 4, 3, 1, 'tensor', 'rows', 'none', 0, 1, 0, -1, -1, ''),
    ((0, 2, 1, 1, 0, 0, 1, 0), (4, 4), 4, 3, 1, 'tensor', 'rows', 'none', 1, 0, 0, -1, -1, ''),
    ((0, 2, 1, 1, 0, 0, 1, 1), (4, 4), 4, 3, 1, 'tensor', 'rows', 'none', 1, 1, 0, -1, -1, ''),
    ((0, 2, 1, 1, 0, 1, 0, 0), (4, 4), 4, 3, 1, 'mixed', 'rows', 'none', 0, 0, 0, -1, -1, ''),
    ((0, 2, 1, 1, 0, 1, 0, 0), (4, 4), 4, 3, 1, 'mixed_all_actions_out', 'rows', 'none', 0, 0, 0, -1, -1, 'actions_out'),
    ((0, 2, 1, 1, 0, 1, 0, 0), (4, 4), 4, 3, 1, 'mixed_all_actions_out', 'none', 'none', 0, 0, 0, -1, -1, 'actions_out_only'),
    ((0, 2, 1, 1, 0, 1, 1, 0), (4, 4), 4, 3, 1, 'mixed', 'rows', 'none', 1, 0, 0, -1, -1, ''),
    ((0, 2, 1, 1, 1, 0, 0, 0), (4, 4), 4, 3, 1, 'order', 'rows', 'none', 0, 0, 0, -1, -1, ''),
    ((0, 2, 1, 1, 1, 1, 0, 0), (4, 4), 4, 3, 1, 'mixed_order', 'rows', 'none', 0, 0, 0, -1, -1, ''),
    ((0, 3, 0, 0, 0, 0, 0, 0), (6, 16), 5, 3, 3, 'tensor', 'rows', 'none', 0, 0, 0, -1, -1, ''),
    ((0, 3, 0, 0, 0, 1, 0, 0), (6, 16), 5, 3, 3, 'mixed', 'rows', 'none', 0, 0, 0, -1, -1, ''),
    ((0, 3, 0, 0, 1, 0, 0, 0), (6, 16), 5, 3, 3, 'order', 'rows', 'none', 0, 0, 0, -1, -1, ''),
    ((0, 3, 0, 0, 1, 1, 0, 0), (6, 16), 5, 3, 3, 'mixed_order', 'rows', 'none', 0, 0, 0, -1, -1, ''),
    ((0, 3, 0, 1, 0, 0, 0, 0), (6, 16), 5, 3, 1, 'tensor', 'rows', 'none', 0, 0, 0, -1, -1, ''),
    ((0, 3, 0, 1, 0, 0, 0, 1), (6, 16), 5, 3, 1, 'tensor', 'rows', 'none', 0, 1, 0, -1, -1, ''),
    ((0, 3, 0, 1, 0, 0, 1, 0), (6, 16), 5, 3, 1, 'tensor', 'rows', 'none', 1, 0, 0, -1, -1, ''),
    ((0, 3, 0, 1, 0, 0, 1, 1), (6, 16), 5, 3, 1, 'tensor', 'rows', 'none', 1, 1, 0, -1, -1, ''),
    ((0, 3, 0, 1, 0, 1, 0, 0), (6, 16), 5, 3, 1, 'mixed', 'rows', 'none', 0, 0, 0, -1, -1, ''),
    ((0, 3, 0, 1, 0, 1, 0, 0), (6, 16), 5, 3, 1, 'mixed_all_actions_out', 'rows', 'none', 0, 0, 0, -1, -1, 'actions_out'),
    ((0, 3, 0, 1, 0, 1, 0, 0), (6, 16), 5, 3, 1, 'mixed_all_actions_out', 'none', 'none', 0, 0, 0, -1, -1, 'actions_out_only'),
    ((0, 3, 0, 1, 0, 1, 1, 0), (6, 16), 5, 3, 1, 'mixed', 'rows', 'none', 1, 0, 0, -1, -1, ''),
    ((0, 3, 0, 1, 1, 0, 0, 0), (6, 16), 5, 3, 1, 'order', 'rows', 'none', 0, 0, 0, -1, -1, ''),
    ((0, 3, 0, 1, 1, 1, 0, 0), (6, 16), 5, 3, 1, 'mixed_order', 'rows', 'none', 0, 0, 0, -1, -1, ''),
    ((0, 3, 1, 0, 0, 0, 0, 0), (6, 16), 6, 3, 3, 'tensor', 'rows', 'none', 0, 0, 0, -1, -1, ''),
    ((0, 3, 1, 0, 0, 1, 0, 0), (6, 16), 6, 3, 3, 'mixed', 'rows', 'none', 0, 0, 0, -1, -1, ''),
    ((0, 3, 1, 0, 1, 0, 0, 0), (6, 16), 6, 3, 3, 'order', 'rows', 'none', 0, 0, 0, -1, -1, ''),
    ((0, 3, 1, 0, 1, 1, 0, 0), (6, 16), 6, 3, 3, 'mixed_order', 'rows', 'none', 0, 0, 0, -1, -1, ''),
    ((0, 3, 1, 1, 0, 0, 0, 0), (6, 16), 6, 3, 1, 'tensor', 'rows', 'none', 0, 0, 0, -1, -1, ''),
    ((0, 3, 1, 1, 0, 0, 0, 1), (6, 16), 6, 3, 1, 'tensor', 'rows', 'none', 0, 1, 0, -1, -1, ''),
    ((0, 3, 1, 1, 0, 0, 1, 0), (6, 16), 6, 3, 1, 'tensor', 'rows', 'none', 1, 0, 0, -1, -1, ''),
    ((0, 3, 1, 1, 0, 0, 1, 1), (6, 16), 6, 3, 1, 'tensor', 'rows', 'none', 1, 1, 0, -1, -1, ''),
    ((0, 3, 1, 1, 0, 1, 0, 0), (6, 16), 6, 3, 1, 'mixed', 'rows', 'none', 0, 0, 0, -1, -1, ''),
    ((0, 3, 1, 1, 0, 1, 0, 0), (6, 16), 6, 3, 1, 'mixed_all_actions_out', 'rows', 'none', 0, 0, 0, -1, -1, 'actions_out'),
    ((0, 3, 1, 1, 0, 1, 0, 0), (6, 16), 6, 3, 1, 'mixed_all_actions_out', 'none', 'none', 0, 0, 0, -1, -1, 'actions_out_only'),
    ((0, 3, 1, 1, 0, 1, 1, 0), (6, 16), 6, 3, 1, 'mixed', 'rows', 'none', 1, 0, 0, -1, -1, ''),
    ((0, 3, 1, 1, 1, 0, 0, 0), (6, 16), 6, 3, 1, 'order', 'rows', 'none', 0, 0, 0, -1, -1, ''),
    ((0, 3, 1, 1, 1, 1, 0, 0), (6, 16), 6, 3, 1, 'mixed_order', 'rows', 'none', 0, 0, 0, -1, -1, ''),
    ((0, 4, 0, 0, 0, 0, 0, 0), (6, 16), 9, 3, 3, 'tensor', 'rows', 'none', 0, 0, 0, -1, -1, ''),
    ((0, 4, 0, 0, 0, 1, 0, 0), (6, 16), 9, 3, 3, 'mixed', 'rows', 'none', 0, 0, 0, -1, -1, ''),
    ((0, 4, 0, 0, 1, 0, 0, 0), (6, 16), 9, 3, 3, 'order', 'rows', 'none', 0, 0, 0, -1, -1, ''),
    ((0, 4, 0, 0, 1, 1, 0, 0), (6, 16), 9, 3, 3, 'mixed_order', 'rows', 'none', 0, 0, 0, -1, -1, ''),
    ((0, 4, 0, 1, 0, 0, 0, 0), (6, 16), 9, 3, 1, 'tensor', 'rows', 'none', 0, 0, 0, -1, -1, ''),
    ((0, 4, 0, 1, 0, 0, 0, 1), (6, 16), 9, 3, 1, 'tensor', 'rows', 'none', 0, 1, 0, -1, -1, ''),
    ((0, 4, 0, 1, 0, 0, 1, 0), (6, 16), 9, 3, 1, 'tensor', 'rows', 'none', 1, 0, 0, -1, -1, ''),
    ((0, 4, 0, 1, 0, 0, 1, 1), (6, 16), 9, 3, 1, 'tensor', 'rows', 'none', 1, 1, 0, -1, -1, ''),
    ((0, 4, 0, 1, 0, 1, 0, 0), (6, 16), 9, 3, 1, 'mixed', 'rows', 'none', 0, 0, 0, -1, -1, ''),
    ((0, 4, 0, 1, 0, 1, 0, 0), (6, 16), 9, 3, 1, 'mixed_all_actions_out', 'rows', 'none', 0, 0, 0, -1, -1, 'actions_out'),
    ((0, 4, 0, 1, 0, 1, 0, 0), (6, 16), 9, 3, 1, 'mixed_all_actions_out', 'none', 'none', 0, 0, 0, -1, -1, 'actions_out_only'),
    ((0, 4, 0, 1, 0, 1, 1, 0), (6, 16), 9, 3, 1, 'mixed', 'rows', 'none', 1, 0, 0, -1, -1, ''),
    ((0, 4, 0, 1, 1, 0, 0, 0), (6, 16), 9, 3, 1, 'order', 'rows', 'none', 0, 0, 0, -1, -1, ''),
    ((0, 4, 0, 1, 1, 1, 0, 0), (6, 16), 9, 3, 1, 'mixed_order', 'rows', 'none', 0, 0, 0, -1, -1, ''),
    ((0, 4, 1, 0, 0, 0, 0, 0), (6, 16), 10, 3, 3, 'tensor', 'rows', 'none', 0, 0, 0, -1, -1, ''),
    ((0, 4, 1, 0, 0, 1, 0, 0), (6, 16), 10, 3, 3, 'mixed', 'rows', 'none', 0, 0, 0, -1, -1, ''),
    ((0, 4, 1, 0, 1, 0, 0, 0), (6, 16), 10, 3, 3, 'order', 'rows', 'none', 0, 0, 0, -1, -1, ''),
    ((0, 4, 1, 0, 1, 1, 0, 0), (6, 16), 10, 3, 3, 'mixed_order', 'rows', 'none', 0, 0, 0, -1, -1, ''),
    ((0, 4, 1, 1, 0, 0, 0, 0), (6, 16), 10, 3, 1, 'tensor', 'rows', 'none', 0, 0, 0, -1, -1, ''),
    ((0, 4, 1, 1, 0, 0, 0, 1), (6, 16), 10, 3, 1, 'tensor', 'rows', 'none', 0, 1, 0, -1, -1, ''),
    ((0, 4, 1, 1, 0, 0, 1, 0), (6, 16), 10, 3, 1, 'tensor', 'rows', 'none', 1, 0, 0, -1, -1, ''),
    ((0, 4, 1, 1, 0, 0, 1, 1), (6, 16), 10, 3, 1, 'tensor', 'rows', 'none', 1, 1, 0, -1, -1, ''),
    ((0, 4, 1, 1, 0, 1, 0, 0), (6, 16), 10, 3, 1, 'mixed', 'rows', 'none', 0, 0, 0, -1, -1, ''),
    ((0, 4, 1, 1, 0, 1, 0, 0), (6, 16), 10, 3, 1, 'mixed_all_actions_out', 'rows', 'none', 0, 0, 0, -1, -1, 'actions_out'),
    ((0, 4, 1, 1, 0, 1, 0, 0), (6, 16), 10, 3, 1, 'mixed_all_actions_out', 'none', 'none', 0, 0, 0, -1, -1, 'actions_out_only'),
    ((0, 4, 1, 1, 0, 1, 1, 0), (6, 16), 10, 3, 1, 'mixed', 'rows', 'none', 1, 0, 0, -1, -1, ''),
    ((0, 4, 1, 1, 1, 0, 0, 0), (6, 16), 10, 3, 1, 'order', 'rows', 'none', 0, 0, 0, -1, -1, ''),
    ((0, 4, 1, 1, 1, 1, 0, 0), (6, 16), 10, 3, 1, 'mixed_order', 'rows', 'none', 0, 0, 0, -1, -1, ''),
    ((0, 5, 0, 0, 0, 0, 0, 0), (6, 16), 17, 3, 3, 'tensor', 'rows', 'none', 0, 0, 0, -1, -1, ''),
    ((0, 5, 0, 0, 0, 1, 0, 0), (6, 16), 17, 3, 3, 'mixed', 'rows', 'none', 0, 0, 0, -1, -1, ''),
    ((0, 5, 0, 0, 1, 0, 0, 0), (6, 16), 17, 3, 3, 'order', 'rows', 'none', 0, 0, 0, -1, -1, ''),
    ((0, 5, 0, 0, 1, 1, 0, 0), (6, 16), 17, 3, 3, 'mixed_order', 'rows', 'none', 0, 0, 0, -1, -1, ''),
    ((0, 5, 0, 1, 0, 0, 0, 0), (6, 16), 17, 3, 1, 'tensor', 'rows', 'none', 0, 0, 0, -1, -1, ''),
    ((0, 5, 0, 1, 0, 0, 0, 1), (6, 16), 17, 3, 1, 'tensor', 'rows', 'none', 0, 1, 0, -1, -1, ''),
    ((0, 5, 0, 1, 0, 0, 1, 0), (6, 16), 17, 3, 1, 'tensor', 'rows', 'none', 1, 0, 0, -1, -1, ''),
    ((0, 5, 0, 1, 0, 0, 1, 1), (6, 16), 17, 3, 1, 'tensor', 'rows', 'none', 1, 1, 0, -1, -1, ''),
    ((0, 5, 0, 1, 0, 1, 0, 0), (6, 16), 17, 3, 1, 'mixed', 'rows', 'none', 0, 0, 0, -1, -1, ''),
    ((0, 5, 0, 1, 0, 1, 0, 0), (6, 16), 17, 3, 1, 'mixed_all_actions_out', 'rows', 'none', 0, 0, 0, -1, -1, 'actions_out'),
    ((0, 5, 0, 1, 0, 1, 0, 0), (6, 16), 17, 3, 1, 'mixed_all_actions_out', 'none', 'none', 0, 0, 0, -1, -1, 'actions_out_only'),
    ((0, 5, 0, 1, 0, 1, 1, 0), (6, 16), 17, 3, 1, 'mixed', 'rows', 'none', 1, 0, 0, -1, -1, ''),
    ((0, 5, 0, 1, 1, 0, 0, 0), (6, 16), 17, 3, 1, 'order', 'rows', 'none', 0, 0, 0, -1, -1, ''),
    ((0, 5, 0, 1, 1, 1, 0, 0), (6, 16), 17, 3, 1, 'mixed_order', 'rows', 'none', 0, 0, 0, -1, -1, ''),
    ((0, 5, 1, 0, 0, 0, 0, 0), (6, 16), 18, 3, 3, 'tensor', 'rows', 'none', 0, 0, 0, -1, -1, ''),
    ((0, 5, 1, 0, 0, 1, 0, 0), (6, 16), 18, 3, 3, 'mixed', 'rows', 'none', 0, 0, 0, -1, -1, ''),
    ((0, 5, 1, 0, 1, 0, 0, 0), (6, 16), 18, 3, 3, 'order', 'rows', 'none', 0, 0, 0, -1, -1, ''),
    ((0, 5, 1, 0, 1, 1, 0, 0), (6, 16), 18, 3, 3, 'mixed_order', 'rows', 'none', 0, 0, 0, -1, -1, ''),
    ((0, 5, 1, 1, 0, 0, 0, 0), (6, 16), 18, 3, 1, 'tensor', 'rows', 'none', 0, 0, 0, -1, -1, ''),
    ((0, 5, 1, 1, 0, 0, 0, 1), (6, 16), 18, 3, 1, 'tensor', 'rows', 'none', 0, 1, 0, -1, -1, ''),
    ((0, 5, 1, 1, 0, 0, 1, 0), (6, 16), 18, 3, 1, 'tensor', 'rows', 'none', 1, 0, 0, -1, -1, ''),
    ((0, 5, 1, 1, 0, 0, 1, 1), (6, 16), 18, 3, 1, 'tensor', 'rows', 'none', 1, 1, 0, -1, -1, ''),
    ((0, 5, 1, 1, 0, 1, 0, 0), (6, 16), 18, 3, 1, 'mixed', 'rows', 'none', 0, 0, 0, -1, -1, ''),
    ((0, 5, 1, 1, 0, 1, 0, 0), (6, 16), 18, 3, 1, 'mixed_all_actions_out', 'rows', 'none', 0, 0, 0, -1, -1, 'actions_out'),
    ((0, 5, 1, 1, 0, 1, 0, 0), (6, 16), 18, 3, 1, 'mixed_all_actions_out', 'none', 'none', 0, 0, 0, -1, -1, 'actions_out_only'),
    ((0, 5, 1, 1, 0, 1, 1, 0), (6, 16), 18, 3, 1, 'mixed', 'rows', 'none', 1, 0, 0, -1, -1, ''),
    ((0, 5, 1, 1, 1, 0, 0, 0), (6, 16), 18, 3, 1, 'order', 'rows', 'none', 0, 0, 0, -1, -1, ''),
    ((0, 5, 1, 1, 1, 1, 0, 0), (6, 16), 18, 3, 1, 'mixed_order', 'rows', 'none', 0, 0, 0, -1, -1, ''),
    ((0, 6, 0, 0, 0, 0, 0, 0), (20, 12), 33, 3, 3, 'tensor', 'rows', 'none', 0, 0, 0, -1, -1, ''),
    ((0, 6, 0, 0, 0, 1, 0, 0), (20, 12), 33, 3, 3, 'mixed', 'rows', 'none', 0, 0, 0, -1, -1, ''),
    ((0, 6, 0, 0, 1, 0, 0, 0), (20, 12), 33, 3, 3, 'order', 'rows', 'none', 0, 0, 0, -1, -1, ''),
    ((0, 6, 0, 0, 1, 1, 0, 0), (20, 12), 33, 3, 3, 'mixed_order', 'rows', 'none', 0, 0, 0, -1, -1, ''),
    ((0, 6, 0, 1, 0, 0, 0, 0), (20, 12), 33, 3, 1, 'tensor', 'rows', 'none', 0, 0, 0, -1, -1, ''),
    ((0, 6, 0, 1, 0, 0, 0, 1), (20, 12), 33, 3, 1, 'tensor', 'rows', 'none', 0, 1, 0, -1, -1, ''),
    ((0, 6, 0, 1, 0, 0, 1, 0), (20, 12), 33, 3, 1, 'tensor', 'rows', 'none', 1, 0, 0, -1, -1, ''),
    ((0, 6, 0, 1, 0, 0, 1, 1), (20, 12), 33, 3, 1, 'tensor', 'rows', 'none', 1, 1, 0, -1, -1, ''),
    ((0, 6, 0, 1, 0, 1, 0, 0), (20, 12), 33, 3, 1, 'mixed', 'rows', 'none', 0, 0, 0, -1, -1, ''),
    ((0, 6, 0, 1, 0, 1, 0, 0), (20, 12), 33, 3, 1, 'mixed_all_actions_out', 'rows', 'none', 0, 0, 0, -1, -1, 'actions_out'),
    ((0, 6, 0, 1, 0, 1, 0, 0), (20, 12), 33, 3, 1, 'mixed_all_actions_out', 'none', 'none', 0, 0, 0, -1, -1, 'actions_out_only'),
    ((0, 6, 0, 1, 0, 1, 1, 0), (20, 12), 33, 3, 1, 'mixed', 'rows', 'none', 1, 0, 0, -1, -1, ''),
    ((0, 6, 0, 1, 1, 0, 0, 0), (20, 12), 33, 3, 1, 'order', 'rows', 'none', 0, 0, 0, -1, -1, ''),
    ((0, 6, 0, 1, 1, 1, 0, 0), (20, 12), 33, 3, 1, 'mixed_order', 'rows', 'none', 0, 0, 0, -1, -1, ''),
    ((0, 6, 1, 0, 0, 0, 0, 0), (20, 12), 34, 3, 3, 'tensor', 'rows', 'none', 0, 0, 0, -1, -1, ''),
    ((0, 6, 1, 0, 0, 1, 0, 0), (20, 12), 34, 3, 3, 'mixed', 'rows', 'none', 0, 0, 0, -1, -1, ''),
    ((0, 6, 1, 0, 1, 0, 0, 0), (20, 12), 34, 3, 3, 'order', 'rows', 'none', 0, 0, 0, -1, -1, ''),
    ((0, 6, 1, 0, 1, 1, 0, 0), (20, 12), 34, 3, 3, 'mixed_order', 'rows', 'none', 0, 0, 0, -1, -1, ''),
    ((0, 6, 1, 1, 0, 0, 0, 0), (20, 12), 34, 3, 1, 'tensor', 'rows', 'none', 0, 0, 0, -1, -1, ''),
    ((0, 6, 1, 1, 0, 0, 0, 1), (20, 12), 34, 3, 1, 'tensor', 'rows', 'none', 0, 1, 0, -1, -1, ''),
    ((0, 6, 1, 1, 0, 0, 1, 0), (20, 12), 34, 3, 1, 'tensor', 'rows', 'none', 1, 0, 0, -1, -1, ''),
    ((0, 6, 1, 1, 0, 0, 1, 1), (20, 12), 34, 3, 1, 'tensor', 'rows', 'none', 1, 1, 0, -1, -1, ''),
    ((0, 6, 1, 1, 0, 1, 0, 0), (20, 12), 34, 3, 1, 'mixed', 'rows', 'none', 0, 0, 0, -1, -1, ''),
    ((0, 6, 1, 1, 0, 1, 0, 0), (20, 12), 34, 3, 1, 'mixed_all_actions_out', 'rows', 'none', 0, 0, 0, -1, -1, 'actions_out'),
    ((0, 6, 1, 1, 0, 1, 0, 0), (20, 12), 34, 3, 1, 'mixed_all_actions_out', 'none', 'none', 0, 0, 0, -1, -1, 'actions_out_only'),
    ((0, 6, 1, 1, 0, 1, 1, 0), (20, 12), 34, 3, 1, 'mixed', 'rows', 'none', 1, 0, 0, -1, -1, ''),
    ((0, 6, 1, 1, 1, 0, 0, 0), (20, 12), 34, 3, 1, 'order', 'rows', 'none', 0, 0, 0, -1, -1, ''),
    ((0, 6, 1, 1, 1, 1, 0, 0), (20, 12), 34, 3, 1, 'mixed_order', 'rows', 'none', 0, 0, 0, -1, -1, ''),
    ((1, 0, 0, 0, 0, 0, 0, 0), (100, 100), 1, 3, 5, 'order', 'none', 'none', 0, 0, 0, -1, -1, 'default/order'),
    ((1, 0, 0, 0, 0, 0, 0, 0), (100, 100), 1, 3, 5, 'greedy', 'none', 'none', 0, 0, 0, -1, -1, 'default/policy'),
    ((1, 0, 0, 0, 0, 0, 0, 0), (64, 48), 1, 3, 5, 'tensor', 'none', 'reward', 0, 0, 0, -1, -1, 'default/tables'),
    ((1, 0, 0, 0, 0, 0, 0, 0), (40, 30), 1, 129, 17, 'order', 'none', 'none', 0, 0, 64, -1, -1, 'full/order'),
    ((1, 0, 0, 0, 0, 0, 0, 0), (40, 30), 1, 129, 5, 'greedy', 'none', 'none', 0, 0, 64, -1, -1, 'full/policy'),
    ((1, 0, 0, 0, 0, 0, 0, 0), (40, 30), 1, 129, 17, 'tensor', 'none', 'terminated', 0, 0, 64, -1, -1, 'full/tables'),
    ((1, 0, 0, 0, 0, 0, 0, 0), (4, 4), 1, 3, 5, 'greedy', 'none', 'none', 0, 0, 0, 0, -1, 'occ_forced'),
    ((1, 0, 0, 0, 0, 1, 0, 0), (100, 100), 1, 3, 5, 'tensor', 'none', 'none', 0, 0, 0, -1, -1, 'default'),
    ((1, 0, 0, 0, 0, 1, 0, 0), (40, 30), 1, 129, 17, 'tensor', 'none', 'none', 0, 0, 64, -1, -1, 'full'),
    ((1, 0, 0, 0, 0, 1, 0, 0), (4, 4), 1, 3, 17, 'tensor', 'none', 'none', 0, 0, 0, 0, -1, 'occ_forced'),
    ((1, 0, 0, 0, 1, 0, 0, 0), (4, 4), 1, 3, 17, 'order', 'none', 'none', 0, 0, 0, -1, -1, 'default/order'),
    ((1, 0, 0, 0, 1, 0, 0, 0), (4, 4), 1, 3, 5, 'greedy', 'none', 'none', 0, 0, 0, -1, -1, 'default/policy'),
    ((1, 0, 0, 0, 1, 0, 0, 0), (4, 4), 1, 3, 17, 'tensor', 'none', 'reward', 0, 0, 0, -1, -1, 'default/tables'),
    ((1, 0, 0, 0, 1, 0, 0, 0), (4, 4), 1, 129, 17, 'order', 'none', 'none', 0, 0, 64, -1, -1, 'full/order'),
    ((1, 0, 0, 0, 1, 0, 0, 0), (4, 4), 1, 129, 5, 'greedy', 'none', 'none', 0, 0, 64, -1, -1, 'full/policy'),
    ((1, 0, 0, 0, 1, 0, 0, 0), (4, 4), 1, 129, 17, 'tensor', 'none', 'terminated', 0, 0, 64, -1, -1, 'full/tables'),
    ((1, 0, 0, 0, 1, 0, 0, 0), (6, 16), 1, 65536, 5, 'order', 'none', 'none', 0, 0, 0, 1, -1, 'occ_forced'),
    ((1, 0, 0, 0, 1, 1, 0, 0), (4, 4), 1, 3, 17, 'tensor', 'none', 'none', 0, 0, 0, -1, -1, 'default'),
    ((1, 0, 0, 0, 1, 1, 0, 0), (4, 4), 1, 129, 17, 'tensor', 'none', 'none', 0, 0, 64, -1, -1, 'full'),
    ((1, 0, 0, 0, 1, 1, 0, 0), (6, 16), 1, 65536, 5, 'tensor', 'none', 'none', 0, 0, 0, 1, -1, 'occ_forced'),
    ((1, 0, 0, 1, 0, 0, 0, 0), (100, 100), 1, 3, 5, 'order', 'small', 'none', 0, 0, 0, -1, -1, 'default/order'),
    ((1, 0, 0, 1, 0, 0, 0, 0), (100, 100), 1, 3, 5, 'greedy', 'small', 'none', 0, 0, 0, -1, -1, 'default/policy'),
    ((1, 0, 0, 1, 0, 0, 0, 0), (64, 48), 1, 3, 5, 'tensor', 'small', 'reward', 0, 0, 0, -1, -1, 'default/tables'),
    ((1, 0, 0, 1, 0, 0, 0, 0), (40, 30), 1, 129, 17, 'order', 'small', 'none', 0, 0, 64, -1, -1, 'full/order'),
    ((1, 0, 0, 1, 0, 0, 0, 0), (40, 30), 1, 129, 5, 'greedy', 'small', 'none', 0, 0, 64, -1, -1, 'full/policy'),
    ((1, 0, 0, 1, 0, 0, 0, 0), (40, 30), 1, 129, 17, 'tensor', 'small', 'terminated', 0, 0, 64, -1, -1, 'full/tables'),
    ((1, 0, 0, 1, 0, 0, 0, 0), (4, 4), 1, 3, 5, 'greedy', 'small', 'none', 0, 0, 0, 0, -1, 'occ_forced'),
    ((1, 0, 0, 1, 0, 1, 0, 0), (100, 100), 1, 3, 5, 'tensor', 'small', 'none', 0, 0, 0, -1, -1, 'default'),
    ((1, 0, 0, 1, 0, 1, 0, 0), (40, 30), 1, 129, 17, 'tensor', 'small', 'none', 0, 0, 64, -1, -1, 'full'),
    ((1, 0, 0, 1, 0, 1, 0, 0), (4, 4), 1, 3, 17, 'tensor', 'small', 'none', 0, 0, 0, 0, -1, 'occ_forced'),
    ((1, 0, 0, 1, 1, 0, 0, 0), (4, 4), 1, 3, 5, 'greedy_actions_out', 'none', 'none', 0, 0, 0, -1, -1, 'actions_out_only'),
    ((1, 0, 0, 1, 1, 0, 0, 0), (4, 4), 1, 3, 17, 'order', 'small', 'none', 0, 0, 0, -1, -1, 'default/order'),
    ((1, 0, 0, 1, 1, 0, 0, 0), (4, 4), 1, 3, 5, 'greedy', 'small', 'none', 0, 0, 0, -1, -1, 'default/policy'),
    ((1, 0, 0, 1, 1, 0, 0, 0), (4, 4), 1, 3, 17, 'tensor', 'small', 'reward', 0, 0, 0, -1, -1, 'default/tables'),
    ((1, 0, 0, 1, 1, 0, 0, 0), (4, 4), 1, 129, 17, 'order', 'small', 'none', 0, 0, 64, -1, -1, 'full/order'),
    ((1, 0, 0, 1, 1, 0, 0, 0), (4, 4), 1, 129, 5, 'greedy', 'small', 'none', 0, 0, 64, -1, -1, 'full/policy'),
    ((1, 0, 0, 1, 1, 0, 0, 0), (4, 4), 1, 129, 17, 'tensor', 'small', 'terminated', 0, 0, 64, -1, -1, 'full/tables'),
    ((1, 0, 0, 1, 1, 0, 0, 0), (6, 16), 1, 65536, 5, 'order', 'rows', 'none', 0, 0, 0, 1, -1, 'occ_forced'),
    ((1, 0, 0, 1, 1, 1, 0, 0), (4, 4), 1, 3, 17, 'tensor', 'small', 'none', 0, 0, 0, -1, -1, 'default'),
    ((1, 0, 0, 1, 1, 1, 0, 0), (4, 4), 1, 129, 17, 'tensor', 'small', 'none', 0, 0, 64, -1, -1, 'full'),
    ((1, 0, 0, 1, 1, 1, 0, 0), (6, 16), 1, 65536, 5, 'tensor', 'rows', 'none', 0, 0, 0, 1, -1, 'occ_forced'),
    ((1, 0, 0, 2, 0, 0, 0, 0), (100, 100), 1, 3, 5, 'order', 'rows', 'none', 0, 0, 0, -1, -1, 'default/order/off_lines'),
    ((1, 0, 0, 2, 0, 0, 0, 0), (100, 100), 1, 3, 5, 'greedy', 'rows', 'none', 0, 0, 0, -1, -1, 'default/policy/off_lines'),
    ((1, 0, 0, 2, 0, 0, 0, 0), (64, 48), 1, 3, 5, 'tensor', 'rows', 'reward', 0, 0, 0, -1, -1, 'default/tables/off_lines'),
    ((1, 0, 0, 2, 0, 0, 0, 0), (40, 30), 1, 129, 17, 'order', 'rows', 'none', 0, 0, 64, -1, -1, 'full/order/off_lines'),
    ((1, 0, 0, 2, 0, 0, 0, 0), (40, 30), 1, 144, 17, 'order', 'rows16', 'none', 0, 0, 64, -1, -1, 'full/order/residue16'),
    ((1, 0, 0, 2, 0, 0, 0, 0), (40, 30), 1, 129, 5, 'greedy', 'rows', 'none', 0, 0, 64, -1, -1, 'full/policy/off_lines'),
    ((1, 0, 0, 2, 0, 0, 0, 0), (40, 30), 1, 144, 5, 'greedy', 'rows16', 'none', 0, 0, 64, -1, -1, 'full/policy/residue16'),
    ((1, 0, 0, 2, 0, 0, 0, 0), (40, 30), 1, 129, 17, 'tensor', 'rows', 'terminated', 0, 0, 64, -1, -1, 'full/tables/off_lines'),
    ((1, 0, 0, 2, 0, 0, 0, 0), (40, 30), 1, 144, 17, 'tensor', 'rows16', 'terminated', 0, 0, 64, -1, -1, 'full/tables/residue16'),
    ((1, 0, 0, 2, 0, 0, 0, 0), (4, 4), 1, 3, 5, 'greedy', 'rows', 'none', 0, 0, 0, 0, -1, 'occ_forced'),
    ((1, 0, 0, 2, 0, 1, 0, 0), (100, 100), 1, 3, 5, 'tensor', 'rows', 'none', 0, 0, 0, -1, -1, 'default/off_lines'),
    ((1, 0, 0, 2, 0, 1, 0, 0), (40, 30), 1, 129, 17, 'tensor', 'rows', 'none', 0, 0, 64, -1, -1, 'full/off_lines'),
    ((1, 0, 0, 2, 0, 1, 0, 0), (40, 30), 1, 144, 17, 'tensor', 'rows16', 'none', 0, 0, 64, -1, -1, 'full/residue16'),
    ((1, 0, 0, 2, 0, 1, 0, 0), (4, 4), 1, 3, 17, 'tensor', 'rows', 'none', 0, 0, 0, 0, -1, 'occ_forced'),
    ((1, 0, 0, 2, 1, 0, 0, 0), (4, 4), 1, 3, 5, 'greedy_actions_out', 'rows', 'none', 0, 0, 0, -1, -1, 'actions_out'),
    ((1, 0, 0, 2, 1, 0, 0, 0), (4, 4), 1, 3, 17, 'order', 'rows', 'none', 0, 0, 0, -1, -1, 'default/order/off_lines'),
    ((1, 0, 0, 2, 1, 0, 0, 0), (4, 4), 1, 3, 5, 'greedy', 'rows', 'none', 0, 0, 0, -1, -1, 'default/policy/off_lines'),
    ((1, 0, 0, 2, 1, 0, 0, 0), (4, 4), 1, 3, 17, 'tensor', 'rows', 'reward', 0, 0, 0, -1, -1, 'default/tables/off_lines'),
    ((1, 0, 0, 2, 1, 0, 0, 0), (4, 4), 1, 129, 17, 'order', 'rows', 'none', 0, 0, 64, -1, -1, 'full/order/off_lines'),
    ((1, 0, 0, 2, 1, 0, 0, 0), (4, 4), 1, 144, 17, 'order', 'rows16', 'none', 0, 0, 64, -1, -1, 'full/order/residue16'),
    ((1, 0, 0, 2, 1, 0, 0, 0), (4, 4), 1, 129, 5, 'greedy', 'rows', 'none', 0, 0, 64, -1, -1, 'full/policy/off_lines'),
    ((1, 0, 0, 2, 1, 0, 0, 0), (4, 4), 1, 144, 5, 'greedy', 'rows16', 'none', 0, 0, 64, -1, -1, 'full/policy/residue16'),
    ((1, 0, 0, 2, 1, 0, 0, 0), (4, 4), 1, 129, 17, 'tensor', 'rows', 'terminated', 0, 0, 64, -1, -1, 'full/tables/off_lines'),
    ((1, 0, 0, 2, 1, 0, 0, 0), (4, 4), 1, 144, 17, 'tensor', 'rows16', 'terminated', 0, 0, 64, -1, -1, 'full/tables/residue16'),
    ((1, 0, 0, 2, 1, 0, 0, 0), (6, 16), 1, 65536, 5, 'order', 'rows16', 'none', 0, 0, 0, 1, -1, 'occ_forced'),
    ((1, 0, 0, 2, 1, 1, 0, 0), (4, 4), 1, 3, 17, 'tensor', 'rows', 'none', 0, 0, 0, -1, -1, 'default/off_lines'),
    ((1, 0, 0, 2, 1, 1, 0, 0), (4, 4), 1, 129, 17, 'tensor', 'rows', 'none', 0, 0, 64, -1, -1, 'full/off_lines'),
    ((1, 0, 0, 2, 1, 1, 0, 0), (4, 4), 1, 144, 17, 'tensor', 'rows16', 'none', 0, 0, 64, -1, -1, 'full/residue16'),
    ((1, 0, 0, 2, 1, 1, 0, 0), (6, 16), 1, 65536, 5, 'tensor', 'rows16', 'none', 0, 0, 0, 1, -1, 'occ_forced'),
    ((1, 1, 1, 0, 0, 0, 0, 0), (100, 100), 2, 3, 5, 'order', 'none', 'none', 0, 0, 0, -1, -1, 'default/order'),
    ((1, 1, 1, 0, 0, 0, 0, 0), (100, 100), 2, 3, 5, 'greedy', 'none', 'none', 0, 0, 0, -1, -1, 'default/policy'),
    ((1, 1, 1, 0, 0, 0, 0, 0), (64, 48), 2, 3, 5, 'tensor', 'none', 'reward', 0, 0, 0, -1, -1, 'default/tables'),
    ((1, 1, 1, 0, 0, 0, 0, 0), (40, 30), 2, 65, 17, 'order', 'none', 'none', 0, 0, 64, -1, -1, 'full/order'),
    ((1, 1, 1, 0, 0, 0, 0, 0), (40, 30), 2, 65, 5, 'greedy', 'none', 'none', 0, 0, 64, -1, -1, 'full/policy'),
    ((1, 1, 1, 0, 0, 0, 0, 0), (40, 30), 2, 65, 17, 'tensor', 'none', 'terminated', 0, 0, 64, -1, -1, 'full/tables'),
    ((1, 1, 1, 0, 0, 0, 0, 0), (4, 4), 2, 3, 5, 'greedy', 'none', 'none', 0, 0, 0, 0, -1, 'occ_forced'),
    ((1, 1, 1, 0, 0, 1, 0, 0), (100, 100), 2, 3, 5, 'tensor', 'none', 'none', 0, 0, 0, -1, -1, 'default'),
    ((1, 1, 1, 0, 0, 1, 0, 0), (40, 30), 2, 65, 17, 'tensor', 'none', 'none', 0, 0, 64, -1, -1, 'full'),
    ((1, 1, 1, 0, 0, 1, 0, 0), (4, 4), 2, 3, 17, 'tensor', 'none', 'none', 0, 0, 0, 0, -1, 'occ_forced'),
    ((1, 1, 1, 0, 1, 0, 0, 0), (4, 4), 2, 3, 17, 'order', 'none', 'none', 0, 0, 0, -1, -1, 'default/order'),
    ((1, 1, 1, 0, 1, 0, 0, 0), (4, 4), 2, 3, 5, 'greedy', 'none', 'none', 0, 0, 0, -1, -1, 'default/policy'),
    ((1, 1, 1, 0, 1, 0, 0, 0), (4, 4), 2, 3, 17, 'tensor', 'none', 'reward', 0, 0, 0, -1, -1, 'default/tables'),
    ((1, 1, 1, 0, 1, 0, 0, 0), (4, 4), 2, 65, 17, 'order', 'none', 'none', 0, 0, 64, -1, -1, 'full/order'),
    ((1, 1, 1, 0, 1, 0, 0, 0), (4, 4), 2, 65, 5, 'greedy', 'none', 'none', 0, 0, 64, -1, -1, 'full/policy'),
    ((1, 1, 1, 0, 1, 0, 0, 0), (4, 4), 2, 65, 17, 'tensor', 'none', 'terminated', 0, 0, 64, -1, -1, 'full/tables'),
    ((1, 1, 1, 0, 1, 0, 0, 0), (6, 16), 2, 65536, 5, 'order', 'none', 'none', 0, 0, 0, 1, -1, 'occ_forced'),
    ((1, 1, 1, 0, 1, 1, 0, 0), (4, 4), 2, 3, 17, 'tensor', 'none', 'none', 0, 0, 0, -1, -1, 'default'),
    ((1, 1, 1, 0, 1, 1, 0, 0), (4, 4), 2, 65, 17, 'tensor', 'none', 'none', 0, 0, 64, -1, -1, 'full'),
    ((1, 1, 1, 0, 1, 1, 0, 0), (6, 16), 2, 65536, 5, 'tensor', 'none', 'none', 0, 0, 0, 1, -1, 'occ_forced'),
    ((1, 1, 1, 1, 0, 0, 0, 0), (100, 100), 2, 3, 5, 'order', 'small', 'none', 0, 0, 0, -1, -1, 'default/order'),
    ((1, 1, 1, 1, 0, 0, 0, 0), (100, 100), 2, 3, 5, 'greedy', 'small', 'none', 0, 0, 0, -1, -1, 'default/policy'),
    ((1, 1, 1, 1, 0, 0, 0, 0), (64, 48), 2, 3, 5, 'tensor', 'small', 'reward', 0, 0, 0, -1, -1, 'default/tables'),
    ((1, 1, 1, 1, 0, 0, 0, 0), (40, 30), 2, 65, 17, 'order', 'small', 'none', 0, 0, 64, -1, -1, 'full/order'),
    ((1, 1, 1, 1, 0, 0, 0, 0), (40, 30), 2, 65, 5, 'greedy', 'small', 'none', 0, 0, 64, -1, -1, 'full/policy'),
    ((1, 1, 1, 1, 0, 0, 0, 0), (40, 30), 2, 65, 17, 'tensor', 'small', 'terminated', 0, 0, 64, -1, -1, 'full/tables'),
    ((1, 1, 1, 1, 0, 0, 0, 0), (4, 4), 2, 3, 5, 'greedy', 'small', 'none', 0, 0, 0, 0, -1, 'occ_forced'),
    ((1, 1, 1, 1, 0, 1, 0, 0), (100, 100), 2, 3, 5, 'tensor', 'small', 'none', 0, 0, 0, -1, -1, 'default'),
    ((1, 1, 1, 1, 0, 1, 0, 0), (40, 30), 2, 65, 17, 'tensor', 'small', 'none', 0, 0, 64, -1, -1, 'full'),
    ((1, 1, 1, 1, 0, 1, 0, 0), (4, 4), 2, 3, 17, 'tensor', 'small', 'none', 0, 0, 0, 0, -1, 'occ_forced'),
    ((1, 1, 1, 1, 1, 0, 0, 0), (4, 4), 2, 3, 5, 'greedy_actions_out', 'none', 'none', 0, 0, 0, -1, -1, 'actions_out_only'),
    ((1, 1, 1, 1, 1, 0, 0, 0), (4, 4), 2, 3, 17, 'order', 'small', 'none', 0, 0, 0, -1, -1, 'default/order'),
    ((1, 1, 1, 1, 1, 0, 0, 0), (4, 4), 2, 3, 5, 'greedy', 'small', 'none', 0, 0, 0, -1, -1, 'default/policy'),
    ((1, 1, 1, 1, 1, 0, 0, 0), (4, 4), 2, 3, 17, 'tensor', 'small', 'reward', 0, 0, 0, -1, -1, 'default/tables'),
    ((1, 1, 1, 1, 1, 0, 0, 0), (4, 4), 2, 65, 17, 'order', 'small', 'none', 0, 0, 64, -1, -1, 'full/order'),
    ((1, 1, 1, 1, 1, 0, 0, 0), (4, 4), 2, 65, 5, 'greedy', 'small', 'none', 0, 0, 64, -1, -1, 'full/policy'),
    ((1, 1, 1, 1, 1, 0, 0, 0), (4, 4), 2, 65, 17, 'tensor', 'small', 'terminated', 0, 0, 64, -1, -1, 'full/tables'),
    ((1, 1, 1, 1, 1, 0, 0, 0), (6, 16), 2, 65536, 5, 'order', 'rows', 'none', 0, 0, 0, 1, -1, 'occ_forced'),
    ((1, 1, 1, 1, 1, 1, 0, 0), (4, 4), 2, 3, 17, 'tensor', 'small', 'none', 0, 0, 0, -1, -1, 'default'),
    ((1, 1, 1, 1, 1, 1, 0, 0), (4, 4), 2, 65, 17, 'tensor', 'small', 'none', 0, 0, 64, -1, -1, 'full'),
    ((1, 1, 1, 1, 1, 1, 0, 0), (6, 16), 2, 65536, 5, 'tensor', 'rows', 'none', 0, 0, 0, 1, -1, 'occ_forced'),
    ((1, 1, 1, 2, 0, 0, 0, 0), (100, 100), 2, 3, 5, 'order', 'rows', 'none', 0, 0, 0, -1, -1, 'default/order/off_lines'),
    ((1, 1, 1, 2, 0, 0, 0, 0), (100, 100), 2, 3, 5, 'greedy', 'rows', 'none', 0, 0, 0, -1, -1, 'default/policy/off_lines'),
    ((1, 1, 1, 2, 0, 0, 0, 0), (64, 48), 2, 3, 5, 'tensor', 'rows', 'reward', 0, 0, 0, -1, -1, 'default/tables/off_lines'),
    ((1, 1, 1, 2, 0, 0, 0, 0), (40, 30), 2, 65, 17, 'order', 'rows', 'none', 0, 0, 64, -1, -1, 'full/order/off_lines'),
    ((1, 1, 1, 2, 0, 0, 0, 0), (40, 30), 2, 72, 17, 'order', 'rows16', 'none', 0, 0, 64, -1, -1, 'full/order/residue16'),
    ((1, 1, 1, 2, 0, 0, 0, 0), (40, 30), 2, 65, 5, 'greedy', 'rows', 'none', 0, 0, 64, -1, -1, 'full/policy/off_lines'),
    ((1, 1, 1, 2, 0, 0, 0, 0), (40, 30), 2, 72, 5, 'greedy', 'rows16', 'none', 0, 0, 64, -1, -1, 'full/policy/residue16'),
    ((1, 1, 1, 2, 0, 0, 0, 0), (40, 30), 2, 65, 17, 'tensor', 'rows', 'terminated', 0, 0, 64, -1, -1, 'full/tables/off_lines'),
    ((1, 1, 1, 2, 0, 0, 0, 0), (40, 30), 2, 72, 17, 'tensor', 'rows16', 'terminated', 0, 0, 64, -1, -1, 'full/tables/residue16'),
    ((1, 1, 1, 2, 0, 0, 0, 0), (4, 4), 2, 3, 5, 'greedy', 'rows', 'none', 0, 0, 0, 0, -1, 'occ_forced'),
    ((1, 1, 1, 2, 0, 1, 0, 0), (100, 100), 2, 3, 5, 'tensor', 'rows', 'none', 0, 0, 0, -1, -1, 'default/off_lines'),
    ((1, 1, 1, 2, 0, 1, 0, 0), (40, 30), 2, 65, 17, 'tensor', 'rows', 'none', 0, 0, 64, -1, -1, 'full/off_lines'),
    ((1, 1, 1, 2, 0, 1, 0, 0), (40, 30), 2, 72, 17, 'tensor', 'rows16', 'none', 0, 0, 64, -1, -1, 'full/residue16'),
    ((1, 1, 1, 2, 0, 1, 0, 0), (4, 4), 2, 3, 17, 'tensor', 'rows', 'none', 0, 0, 0, 0, -1, 'occ_forced'),
    ((1, 1, 1, 2, 1, 0, 0, 0), (4, 4), 2, 3, 5, 'greedy_actions_out', 'rows', 'none', 0, 0, 0, -1, -1, 'actions_out'),
    ((1, 1, 1, 2, 1, 0, 0, 0), (4, 4), 2, 3, 17, 'order', 'rows', 'none', 0, 0, 0, -1, -1, 'default/order/off_lines'),
    ((1, 1, 1, 2, 1, 0, 0, 0), (4, 4), 2, 3, 5, 'greedy', 'rows', 'none', 0, 0, 0, -1, -1, 'default/policy/off_lines'),
    ((1, 1, 1, 2, 1, 0, 0, 0), (4, 4), 2, 3, 17, 'tensor', 'rows', 'reward', 0, 0, 0, -1, -1, 'default/tables/off_lines'),
    ((1, 1, 1, 2, 1, 0, 0, 0), (4, 4), 2, 65, 17, 'order', 'rows', 'none', 0, 0, 64, -1, -1, 'full/order/off_lines'),
    ((1, 1, 1, 2, 1, 0, 0, 0), (4, 4), 2, 72, 17, 'order', 'rows16', 'none', 0, 0, 64, -1, -1, 'full/order/residue16'),
    ((1, 1, 1, 2, 1, 0, 0, 0), (4, 4), 2, 65, 5, 'greedy', 'rows', 'none', 0, 0, 64, -1, -1, 'full/policy/off_lines'),
    ((1, 1, 1, 2, 1, 0, 0, 0), (4, 4), 2, 72, 5, 'greedy', 'rows16', 'none', 0, 0, 64, -1, -1, 'full/policy/residue16'),
    ((1, 1, 1, 2, 1, 0, 0, 0), (4, 4), 2, 65, 17, 'tensor', 'rows', 'terminated', 0, 0, 64, -1, -1, 'full/tables/off_lines'),
    ((1, 1, 1, 2, 1, 0, 0, 0), (4, 4), 2, 72, 17, 'tensor', 'rows16', 'terminated', 0, 0, 64, -1, -1, 'full/tables/residue16'),
    ((1, 1, 1, 2, 1, 0, 0, 0), (6, 16), 2, 65536, 5, 'order', 'rows16', 'none', 0, 0, 0, 1, -1, 'occ_forced'),
    ((1, 1, 1, 2, 1, 1, 0, 0), (4, 4), 2, 3, 17, 'tensor', 'rows', 'none', 0, 0, 0, -1, -1, 'default/off_lines'),
    ((1, 1, 1, 2, 1, 1, 0, 0), (4, 4), 2, 65, 17, 'tensor', 'rows', 'none', 0, 0, 64, -1, -1, 'full/off_lines'),
    ((1, 1, 1, 2, 1, 1, 0, 0), (4, 4), 2, 72, 17, 'tensor', 'rows16', 'none', 0, 0, 64, -1, -1, 'full/residue16'),
    ((1, 1, 1, 2, 1, 1, 0, 0), (6, 16), 2, 65536, 5, 'tensor', 'rows16', 'none', 0, 0, 0, 1, -1, 'occ_forced'),
    ((1, 2, 0, 0, 0, 0, 0, 0), (100, 100), 3, 3, 5, 'order', 'none', 'none', 0, 0, 0, -1, -1, 'default/order'),
    ((1, 2, 0, 0, 0, 0, 0, 0), (100, 100), 3, 3, 5, 'greedy', 'none', 'none', 0, 0, 0, -1, -1, 'default/policy'),
    ((1, 2, 0, 0, 0, 0, 0, 0), (64, 48), 3, 3, 5, 'tensor', 'none', 'reward', 0, 0, 0, -1, -1, 'default/tables'),
    ((1, 2, 0, 0, 0, 0, 0, 0), (40, 30), 3, 33, 17, 'order', 'none', 'none', 0, 0, 64, -1, -1, 'full/order'),
    ((1, 2, 0, 0, 0, 0, 0, 0), (40, 30), 3, 33, 5, 'greedy', 'none', 'none', 0, 0, 64, -1, -1, 'full/policy'),
    ((1, 2, 0, 0, 0, 0, 0, 0), (40, 30), 3, 33, 17, 'tensor', 'none', 'terminated', 0, 0, 64, -1, -1, 'full/tables'),
    ((1, 2, 0, 0, 0, 0, 0, 0), (4, 4), 3, 3, 5, 'greedy', 'none', 'none', 0, 0, 0, 0, -1, 'occ_forced'),
    ((1, 2, 0, 0, 0, 1, 0, 0), (100, 100), 3, 3, 5, 'tensor', 'none', 'none', 0, 0, 0, -1, -1, 'default'),
    ((1, 2, 0, 0, 0, 1, 0, 0), (40, 30), 3, 33, 17, 'tensor', 'none', 'none', 0, 0, 64, -1, -1, 'full'),
    ((1, 2, 0, 0, 0, 1, 0, 0), (4, 4), 3, 3, 17, 'tensor', 'none', 'none', 0, 0, 0, 0, -1, 'occ_forced'),
    ((1, 2, 0, 0, 1, 0, 0, 0), (4, 4), 3, 3, 17, 'order', 'none', 'none', 0, 0, 0, -1, -1, 'default/order'),
    ((1, 2, 0, 0, 1, 0, 0, 0), (4, 4), 3, 3, 5, 'greedy', 'none', 'none', 0, 0, 0, -1, -1, 'default/policy'),
    ((1, 2, 0, 0, 1, 0, 0, 0), (4, 4), 3, 3, 17, 'tensor', 'none', 'reward', 0, 0, 0, -1, -1, 'default/tables'),
    ((1, 2, 0, 0, 1, 0, 0, 0), (4, 4), 3, 33, 17, 'order', 'none', 'none', 0, 0, 64, -1, -1, 'full/order'),
    ((1, 2, 0, 0, 1, 0, 0, 0), (4, 4), 3, 33, 5, 'greedy', 'none', 'none', 0, 0, 64, -1, -1, 'full/policy'),
    ((1, 2, 0, 0, 1, 0, 0, 0), (4, 4), 3, 33, 17, 'tensor', 'none', 'terminated', 0, 0, 64, -1, -1, 'full/tables'),
    ((1, 2, 0, 0, 1, 0, 0, 0), (20, 12), 3, 8193, 5, 'order', 'none', 'none', 0, 0, 0, 1, -1, 'occ_forced'),
    ((1, 2, 0, 0, 1, 1, 0, 0), (4, 4), 3, 3, 17, 'tensor', 'none', 'none', 0, 0, 0, -1, -1, 'default'),
    ((1, 2, 0, 0, 1, 1, 0, 0), (4, 4), 3, 33, 17, 'tensor', 'none', 'none', 0, 0, 64, -1, -1, 'full'),
    ((1, 2, 0, 0, 1, 1, 0, 0), (20, 12), 3, 8193, 5, 'tensor', 'none', 'none', 0, 0, 0, 1, -1, 'occ_forced'),
    ((1, 2, 0, 1, 0, 0, 0, 0), (100, 100), 3, 3, 5, 'order', 'small', 'none', 0, 0, 0, -1, -1, 'default/order'),
    ((1, 2, 0, 1, 0, 0, 0, 0), (100, 100), 3, 3, 5, 'greedy', 'small', 'none', 0, 0, 0, -1, -1, 'default/policy'),
    ((1, 2, 0, 1, 0, 0, 0, 0), (64, 48), 3, 3, 5, 'tensor', 'small', 'reward', 0, 0, 0, -1, -1, 'default/tables'),
    ((1, 2, 0, 1, 0, 0, 0, 0), (40, 30), 3, 33, 17, 'order', 'small', 'none', 0, 0, 64, -1, -1, 'full/order'),
    ((1, 2, 0, 1, 0, 0, 0, 0), (40, 30), 3, 33, 5, 'greedy', 'small', 'none', 0, 0, 64, -1, -1, 'full/policy'),
    ((1, 2, 0, 1, 0, 0, 0, 0), (40, 30), 3, 33, 17, 'tensor', 'small', 'terminated', 0, 0, 64, -1, -1, 'full/tables'),
    ((1, 2, 0, 1, 0, 0, 0, 0), (4, 4), 3, 3, 5, 'greedy', 'small', 'none', 0, 0, 0, 0, -1, 'occ_forced'),
    ((1, 2, 0, 1, 0, 1, 0, 0), (100, 100), 3, 3, 5, 'tensor', 'small', 'none', 0, 0, 0, -1, -1, 'default'),
    ((1, 2, 0, 1, 0, 1, 0, 0), (40, 30), 3, 33, 17, 'tensor', 'small', 'none', 0, 0, 64, -1, -1, 'full'),
    ((1, 2, 0, 1, 0, 1, 0, 0), (4, 4), 3, 3, 17, 'tensor', 'small', 'none', 0, 0, 0, 0, -1, 'occ_forced'),
    ((1, 2, 0, 1, 1, 0, 0, 0), (4, 4), 3, 3, 5, 'greedy_actions_out', 'none', 'none', 0, 0, 0, -1, -1, 'actions_out_only'),
    ((1, 2, 0, 1, 1, 0, 0, 0), (4, 4), 3, 3, 17, 'order', 'small', 'none', 0, 0, 0, -1, -1, 'default/order'),
    ((1, 2, 0, 1, 1, 0, 0, 0), (4, 4), 3, 3, 5, 'greedy', 'small', 'none', 0, 0, 0, -1, -1, 'default/policy'),
    ((1, 2, 0, 1, 1, 0, 0, 0), (4, 4), 3, 3, 17, 'tensor', 'small', 'reward', 0, 0, 0, -1, -1, 'default/tables'),
    ((1, 2, 0, 1, 1, 0, 0, 0), (4, 4), 3, 33, 17, 'order', 'small', 'none', 0, 0, 64, -1, -1, 'full/order'),
    ((1, 2, 0, 1, 1, 0, 0, 0), (4, 4), 3, 33, 5, 'greedy', 'small', 'none', 0, 0, 64, -1, -1, 'full/policy'),
    ((1, 2, 0, 1, 1, 0, 0, 0), (4, 4), 3, 33, 17, 'tensor', 'small', 'terminated', 0, 0, 64, -1, -1, 'full/tables'),
    ((1, 2, 0, 1, 1, 0, 0, 0), (20, 12), 3, 8193, 5, 'order', 'small', 'none', 0, 0, 0, 1, -1, 'occ_forced'),
    ((1, 2, 0, 1, 1, 1, 0, 0), (4, 4), 3, 3, 17, 'tensor', 'small', 'none', 0, 0, 0, -1, -1, 'default'),
    ((1, 2, 0, 1, 1, 1, 0, 0), (4, 4), 3, 33, 17, 'tensor', 'small', 'none', 0, 0, 64, -1, -1, 'full'),
    ((1, 2, 0, 1, 1, 1, 0, 0), (20, 12), 3, 8193, 5, 'tensor', 'small', 'none', 0, 0, 0, 1, -1, 'occ_forced'),
    ((1, 2, 0, 2, 0, 0, 0, 0), (100, 100), 3, 3, 5, 'order', 'rows', 'none', 0, 0, 0, -1, -1, 'default/order/off_lines'),
    ((1, 2, 0, 2, 0, 0, 0, 0), (100, 100), 3, 3, 5, 'greedy', 'rows', 'none', 0, 0, 0, -1, -1, 'default/policy/off_lines'),
    ((1, 2, 0, 2, 0, 0, 0, 0), (64, 48), 3, 3, 5, 'tensor', 'rows', 'reward', 0, 0, 0, -1, -1, 'default/tables/off_lines'),
    ((1, 2, 0, 2, 0, 0, 0, 0), (40, 30), 3, 33, 17, 'order', 'rows', 'none', 0, 0, 64, -1, -1, 'full/order/off_lines'),
    ((1, 2, 0, 2, 0, 0, 0, 0), (40, 30), 3, 16, 17, 'order', 'rows16', 'none', 0, 0, 64, -1, -1, 'full/order/residue16'),
    ((1, 2, 0, 2, 0, 0, 0, 0), (40, 30), 3, 33, 5, 'greedy', 'rows', 'none', 0, 0, 64, -1, -1, 'full/policy/off_lines'),
    ((1, 2, 0, 2, 0, 0, 0, 0), (40, 30), 3, 16, 5, 'greedy', 'rows16', 'none', 0, 0, 64, -1, -1, 'full/policy/residue16'),
    ((1, 2, 0, 2, 0, 0, 0, 0), (40, 30), 3, 33, 17, 'tensor', 'rows', 'terminated', 0, 0, 64, -1, -1, 'full/tables/off_lines'),
    ((1, 2, 0, 2, 0, 0, 0, 0), (40, 30), 3, 16, 17, 'tensor', 'rows16', 'terminated', 0, 0, 64, -1, -1, 'full/tables/residue16'),
    ((1, 2, 0, 2, 0, 0, 0, 0), (4, 4), 3, 3, 5, 'greedy', 'rows', 'none', 0, 0, 0, 0, -1, 'occ_forced'),
    ((1, 2, 0, 2, 0, 1, 0, 0), (100, 100), 3, 3, 5, 'tensor', 'rows', 'none', 0, 0, 0, -1, -1, 'default/off_lines'),
    ((1, 2, 0, 2, 0, 1, 0, 0), (40, 30), 3, 33, 17, 'tensor', 'rows', 'none', 0, 0, 64, -1, -1, 'full/off_lines'),
    ((1, 2, 0, 2, 0, 1, 0, 0), (40, 30), 3, 16, 17, 'tensor', 'rows16', 'none', 0, 0, 64, -1, -1, 'full/residue16'),
    ((1, 2, 0, 2, 0, 1, 0, 0), (4, 4), 3, 3, 17, 'tensor', 'rows', 'none', 0, 0, 0, 0, -1, 'occ_forced'),
    ((1, 2, 0, 2, 1, 0, 0, 0), (4, 4), 3, 3, 5, 'greedy_actions_out', 'rows', 'none', 0, 0, 0, -1, -1, 'actions_out'),
    ((1, 2, 0, 2, 1, 0, 0, 0), (4, 4), 3, 3, 17, 'order', 'rows', 'none', 0, 0, 0, -1, -1, 'default/order/off_lines'),
    ((1, 2, 0, 2, 1, 0, 0, 0), (4, 4), 3, 3, 5, 'greedy', 'rows', 'none', 0, 0, 0, -1, -1, 'default/policy/off_lines'),
    ((1, 2, 0, 2, 1, 0, 0, 0), (4, 4), 3, 3, 17, 'tensor', 'rows', 'reward', 0, 0, 0, -1, -1, 'default/tables/off_lines'),
    ((1, 2, 0, 2, 1, 0, 0, 0), (4, 4), 3, 33, 17, 'order', 'rows', 'none', 0, 0, 64, -1, -1, 'full/order/off_lines'),
    ((1, 2, 0, 2, 1, 0, 0, 0), (4, 4), 3, 16, 17, 'order', 'rows16', 'none', 0, 0, 64, -1, -1, 'full/order/residue16'),
    ((1, 2, 0, 2, 1, 0, 0, 0), (4, 4), 3, 33, 5, 'greedy', 'rows', 'none', 0, 0, 64, -1, -1, 'full/policy/off_lines'),
    ((1, 2, 0, 2, 1, 0, 0, 0), (4, 4), 3, 16, 5, 'greedy', 'rows16', 'none', 0, 0, 64, -1, -1, 'full/policy/residue16'),
    ((1, 2, 0, 2, 1, 0, 0, 0), (4, 4), 3, 33, 17, 'tensor', 'rows', 'terminated', 0, 0, 64, -1, -1, 'full/tables/off_lines'),
    ((1, 2, 0, 2, 1, 0, 0, 0), (4, 4), 3, 16, 17, 'tensor', 'rows16', 'terminated', 0, 0, 64, -1, -1, 'full/tables/residue16'),
    ((1, 2, 0, 2, 1, 0, 0, 0), (20, 12), 3, 8193, 5, 'order', 'rows', 'none', 0, 0, 0, 1, -1, 'occ_forced'),
    ((1, 2, 0, 2, 1, 1, 0, 0), (4, 4), 3, 3, 17, 'tensor', 'rows', 'none', 0, 0, 0, -1, -1, 'default/off_lines'),
    ((1, 2, 0, 2, 1, 1, 0, 0), (4, 4), 3, 33, 17, 'tensor', 'rows', 'none', 0, 0, 64, -1, -1, 'full/off_lines'),
    ((1, 2, 0, 2, 1, 1, 0, 0), (4, 4), 3, 16, 17, 'tensor', 'rows16', 'none', 0, 0, 64, -1, -1, 'full/residue16'),
    ((1, 2, 0, 2, 1, 1, 0, 0), (20, 12), 3, 8193, 5, 'tensor', 'rows', 'none', 0, 0, 0, 1, -1, 'occ_forced'),
    ((1, 2, 1, 0, 0, 0, 0, 0), (100, 100), 4, 3, 5, 'order', 'none', 'none', 0, 0, 0, -1, -1, 'default/order'),
    ((1, 2, 1, 0, 0, 0, 0, 0), (100, 100), 4, 3, 5, 'greedy', 'none', 'none', 0, 0, 0, -1, -1, 'default/policy'),
    ((1, 2, 1, 0, 0, 0, 0, 0), (64, 48), 4, 3, 5, 'tensor', 'none', 'reward', 0, 0, 0, -1, -1, 'default/tables'),
    ((1, 2, 1, 0, 0, 0, 0, 0), (40, 30), 4, 33, 17, 'order', 'none', 'none', 0, 0, 64, -1, -1, 'full/order'),
    ((1, 2, 1, 0, 0, 0, 0, 0), (40, 30), 4, 33, 5, 'greedy', 'none', 'none', 0, 0, 64, -1, -1, 'full/policy'),
    ((1, 2, 1, 0, 0, 0, 0, 0), (40, 30), 4, 33, 17, 'tensor', 'none', 'terminated', 0, 0, 64, -1, -1, 'full/tables'),
    ((1, 2, 1, 0, 0, 0, 0, 0), (4, 4), 4, 3, 5, 'greedy', 'none', 'none', 0, 0, 0, 0, -1, 'occ_forced'),
    ((1, 2, 1, 0, 0, 1, 0, 0), (100, 100), 4, 3, 5, 'tensor', 'none', 'none', 0, 0, 0, -1, -1, 'default'),
    ((1, 2, 1, 0, 0, 1, 0, 0), (40, 30), 4, 33, 17, 'tensor', 'none', 'none', 0, 0, 64, -1, -1, 'full'),
    ((1, 2, 1, 0, 0, 1, 0, 0), (4, 4), 4, 3, 17, 'tensor', 'none', 'none', 0, 0, 0, 0, -1, 'occ_forced'),
    ((1, 2, 1, 0, 1, 0, 0, 0), (4, 4), 4, 3, 17, 'order', 'none', 'none', 0, 0, 0, -1, -1, 'default/order'),
    ((1, 2, 1, 0, 1, 0, 0, 0), (4, 4), 4, 3, 5, 'greedy', 'none', 'none', 0, 0, 0, -1, -1, 'default/policy'),
    ((1, 2, 1, 0, 1, 0, 0, 0), (4, 4), 4, 3, 17, 'tensor', 'none', 'reward', 0, 0, 0, -1, -1, 'default/tables'),
    ((1, 2, 1, 0, 1, 0, 0, 0), (4, 4), 4, 33, 17, 'order', 'none', 'none', 0, 0, 64, -1, -1, 'full/order'),
    ((1, 2, 1, 0, 1, 0, 0, 0), (4, 4), 4, 33, 5, 'greedy', 'none', 'none', 0, 0, 64, -1, -1, 'full/policy'),
    ((1, 2, 1, 0, 1, 0, 0, 0), (4, 4), 4, 33, 17, 'tensor', 'none', 'terminated', 0, 0, 64, -1, -1, 'full/tables'),
    ((1, 2, 1, 0, 1, 0, 0, 0), (20, 12), 4, 8193, 5, 'order', 'none', 'none', 0, 0, 0, 1, -1, 'occ_forced'),
    ((1, 2, 1, 0, 1, 1, 0, 0), (4, 4), 4, 3, 17, 'tensor', 'none', 'none', 0, 0, 0, -1, -1, 'default'),
    ((1, 2, 1, 0, 1, 1, 0, 0), (4, 4), 4, 33, 17, 'tensor', 'none', 'none', 0, 0, 64, -1, -1, 'full'),
    ((1, 2, 1, 0, 1, 1, 0, 0), (20, 12), 4, 8193, 5, 'tensor', 'none', 'none', 0, 0, 0, 1, -1, 'occ_forced'),
    ((1, 2, 1, 1, 0, 0, 0, 0), (100, 100), 4, 3, 5, 'order', 'small', 'none', 0, 0, 0, -1, -1, 'default/order'),
    ((1, 2, 1, 1, 0, 0, 0, 0), (100, 100), 4, 3, 5, 'greedy', 'small', 'none', 0, 0, 0, -1, -1, 'default/policy'),
    ((1, 2, 1, 1, 0, 0, 0, 0), (64, 48), 4, 3, 5, 'tensor', 'small', 'reward', 0, 0, 0, -1, -1, 'default/tables'),
    ((1, 2, 1, 1, 0, 0, 0, 0), (40, 30), 4, 33, 17, 'order', 'small', 'none', 0, 0, 64, -1, -1, 'full/order'),
    ((1, 2, 1, 1, 0, 0, 0, 0), (40, 30), 4, 33, 5, 'greedy', 'small', 'none', 0, 0, 64, -1, -1, 'full/policy'),
    ((1, 2, 1, 1, 0, 0, 0, 0), (40, 30), 4, 33, 17, 'tensor', 'small', 'terminated', 0, 0, 64, -1, -1, 'full/tables'),
    ((1, 2, 1, 1, 0, 0, 0, 0), (4, 4), 4, 3, 5, 'greedy', 'small', 'none', 0, 0, 0, 0, -1, 'occ_forced'),
    ((1, 2, 1, 1, 0, 1, 0, 0), (100, 100), 4, 3, 5, 'tensor', 'small', 'none', 0, 0, 0, -1, -1, 'default'),
    ((1, 2, 1, 1, 0, 1, 0, 0), (40, 30), 4, 33, 17, 'tensor', 'small', 'none', 0, 0, 64, -1, -1, 'full'),
    ((1, 2, 1, 1, 0, 1, 0, 0), (4, 4), 4, 3, 17, 'tensor', 'small', 'none', 0, 0, 0, 0, -1, 'occ_forced'),
    ((1, 2, 1, 1, 1, 0, 0, 0), (4, 4), 4, 3, 5, 'greedy_actions_out', 'none', 'none', 0, 0, 0, -1, -1, 'actions_out_only'),
    ((1, 2, 1, 1, 1, 0, 0, 0), (4, 4), 4, 3, 17, 'order', 'small', 'none', 0, 0, 0, -1, -1, 'default/order'),
    ((1, 2, 1, 1, 1, 0, 0, 0), (4, 4), 4, 3, 5, 'greedy', 'small', 'none', 0, 0, 0, -1, -1, 'default/policy'),
    ((1, 2, 1, 1, 1, 0, 0, 0), (4, 4), 4, 3, 17, 'tensor', 'small', 'reward', 0, 0, 0, -1, -1, 'default/tables'),
    ((1, 2, 1, 1, 1, 0, 0, 0), (4, 4), 4, 33, 17, 'order', 'small', 'none', 0, 0, 64, -1, -1, 'full/order'),
    ((1, 2, 1, 1, 1, 0, 0, 0), (4, 4), 4, 33, 5, 'greedy', 'small', 'none', 0, 0, 64, -1, -1, 'full/policy'),
    ((1, 2, 1, 1, 1, 0, 0, 0), (4, 4), 4, 33, 17, 'tensor', 'small', 'terminated', 0, 0, 64, -1, -1, 'full/tables'),
    ((1, 2, 1, 1, 1, 0, 0, 0), (20, 12), 4, 8193, 5, 'order', 'small', 'none', 0, 0, 0, 1, -1, 'occ_forced'),
    ((1, 2, 1, 1, 1, 1, 0, 0), (4, 4), 4, 3, 17, 'tensor', 'small', 'none', 0, 0, 0, -1, -1, 'default'),
    ((1, 2, 1, 1, 1, 1, 0, 0), (4, 4), 4, 33, 17, 'tensor', 'small', 'none', 0, 0, 64, -1, -1, 'full'),
    ((1, 2, 1, 1, 1, 1, 0, 0), (20, 12), 4, 8193, 5, 'tensor', 'small', 'none', 0, 0, 0, 1, -1, 'occ_forced'),
    ((1, 2, 1, 2, 0, 0, 0, 0), (100, 100), 4, 3, 5, 'order', 'rows', 'none', 0, 0, 0, -1, -1, 'default/order/off_lines'),
    ((1, 2, 1, 2, 0, 0, 0, 0), (100, 100), 4, 3, 5, 'greedy', 'rows', 'none', 0, 0, 0, -1, -1, 'default/policy/off_lines'),
    ((1, 2, 1, 2, 0, 0, 0, 0), (64, 48), 4, 3, 5, 'tensor', 'rows', 'reward', 0, 0, 0, -1, -1, 'default/tables/off_lines'),
    ((1, 2, 1, 2, 0, 0, 0, 0), (40, 30), 4, 33, 17, 'order', 'rows', 'none', 0, 0, 64, -1, -1, 'full/order/off_lines'),
    ((1, 2, 1, 2, 0, 0, 0, 0), (40, 30), 4, 36, 17, 'order', 'rows16', 'none', 0, 0, 64, -1, -1, 'full/order/residue16'),
    ((1, 2, 1, 2, 0, 0, 0, 0), (40, 30), 4, 33, 5, 'greedy', 'rows', 'none', 0, 0, 64, -1, -1, 'full/policy/off_lines'),
    ((1, 2, 1, 2, 0, 0, 0, 0), (40, 30), 4, 36, 5, 'greedy', 'rows16', 'none', 0, 0, 64, -1, -1, 'full/policy/residue16'),
    ((1, 2, 1, 2, 0, 0, 0, 0), (40, 30), 4, 33, 17, 'tensor', 'rows', 'terminated', 0, 0, 64, -1, -1, 'full/tables/off_lines'),
    ((1, 2, 1, 2, 0, 0, 0, 0), (40, 30), 4, 36, 17, 'tensor', 'rows16', 'terminated', 0, 0, 64, -1, -1, 'full/tables/residue16'),
    ((1, 2, 1, 2, 0, 0, 0, 0), (4, 4), 4, 3, 5, 'greedy', 'rows', 'none', 0, 0, 0, 0, -1, 'occ_forced'),
    ((1, 2, 1, 2, 0, 1, 0, 0), (100, 100), 4, 3, 5, 'tensor', 'rows', 'none', 0, 0, 0, -1, -1, 'default/off_lines'),
    ((1, 2, 1, 2, 0, 1, 0, 0), (40, 30), 4, 33, 17, 'tensor', 'rows', 'none', 0, 0, 64, -1, -1, 'full/off_lines'),
    ((1, 2, 1, 2, 0, 1, 0, 0), (40, 30), 4, 36, 17, 'tensor', 'rows16', 'none', 0, 0, 64, -1, -1, 'full/residue16'),
    ((1, 2, 1, 2, 0, 1, 0, 0), (4, 4), 4, 3, 17, 'tensor', 'rows', 'none', 0, 0, 0, 0, -1, 'occ_forced'),
    ((1, 2, 1, 2, 1, 0, 0, 0), (4, 4), 4, 3, 5, 'greedy_actions_out', 'rows', 'none', 0, 0, 0, -1, -1, 'actions_out'),
    ((1, 2, 1, 2, 1, 0, 0, 0), (4, 4), 4, 3, 17, 'order', 'rows', 'none', 0, 0, 0, -1, -1, 'default/order/off_lines'),
    ((1, 2, 1, 2, 1, 0, 0, 0), (4, 4), 4, 3, 5, 'greedy', 'rows', 'none', 0, 0, 0, -1, -1, 'default/policy/off_lines'),
    ((1, 2, 1, 2, 1, 0, 0, 0), (4, 4), 4, 3, 17, 'tensor', 'rows', 'reward', 0, 0, 0, -1, -1, 'default/tables/off_lines'),
    ((1, 2, 1, 2, 1, 0, 0, 0), (4, 4), 4, 33, 17, 'order', 'rows', 'none', 0, 0, 64, -1, -1, 'full/order/off_lines'),
    ((1, 2, 1, 2, 1, 0, 0, 0), (4, 4), 4, 36, 17, 'order', 'rows16', 'none', 0, 0, 64, -1, -1, 'full/order/residue16'),
    ((1, 2, 1, 2, 1, 0, 0, 0), (4, 4), 4, 33, 5, 'greedy', 'rows', 'none', 0, 0, 64, -1, -1, 'full/policy/off_lines'),
    ((1, 2, 1, 2, 1, 0, 0, 0), (4, 4), 4, 36, 5, 'greedy', 'rows16', 'none', 0, 0, 64, -1, -1, 'full/policy/residue16'),
    ((1, 2, 1, 2, 1, 0, 0, 0), (4, 4), 4, 33, 17, 'tensor', 'rows', 'terminated', 0, 0, 64, -1, -1, 'full/tables/off_lines'),
    ((1, 2, 1, 2, 1, 0, 0, 0), (4, 4), 4, 36, 17, 'tensor', 'rows16', 'terminated', 0, 0, 64, -1, -1, 'full/tables/residue16'),
    ((1, 2, 1, 2, 1, 0, 0, 0), (20, 12), 4, 8193, 5, 'order', 'rows', 'none', 0, 0, 0, 1, -1, 'occ_forced'),
    ((1, 2, 1, 2, 1, 1, 0, 0), (4, 4), 4, 3, 17, 'tensor', 'rows', 'none', 0, 0, 0, -1, -1, 'default/off_lines'),
    ((1, 2, 1, 2, 1, 1, 0, 0), (4, 4), 4, 33, 17, 'tensor', 'rows', 'none', 0, 0, 64, -1, -1, 'full/off_lines'),
    ((1, 2, 1, 2, 1, 1, 0, 0), (4, 4), 4, 36, 17, 'tensor', 'rows16', 'none', 0, 0, 64, -1, -1, 'full/residue16'),
    ((1, 2, 1, 2, 1, 1, 0, 0), (20, 12), 4, 8193, 5, 'tensor', 'rows', 'none', 0, 0, 0, 1, -1, 'occ_forced'),
    ((1, 3, 0, 0, 0, 0, 0, 0), (100, 100), 5, 3, 5, 'order', 'none', 'none', 0, 0, 0, -1, -1, 'default/order'),
    ((1, 3, 0, 0, 0, 0, 0, 0), (100, 100), 5, 3, 5, 'greedy', 'none', 'none', 0, 0, 0, -1, -1, 'default/policy'),
    ((1, 3, 0, 0, 0, 0, 0, 0), (64, 48), 5, 3, 5, 'tensor', 'none', 'reward', 0, 0, 0, -1, -1, 'default/tables'),
    ((1, 3, 0, 0, 0, 0, 0, 0), (40, 30), 5, 17, 17, 'order', 'none', 'none', 0, 0, 64, -1, -1, 'full/order'),
    ((1, 3, 0, 0, 0, 0, 0, 0), (40, 30), 5, 17, 5, 'greedy', 'none', 'none', 0, 0, 64, -1, -1, 'full/policy'),
    ((1, 3, 0, 0, 0, 0, 0, 0), (40, 30), 5, 17, 17, 'tensor', 'none', 'terminated', 0, 0, 64, -1, -1, 'full/tables'),
    ((1, 3, 0, 0, 0, 0, 0, 0), (6, 16), 5, 3, 5, 'greedy', 'none', 'none', 0, 0, 0, 0, -1, 'occ_forced'),
    ((1, 3, 0, 0, 0, 1, 0, 0), (100, 100), 5, 3, 5, 'tensor', 'none', 'none', 0, 0, 0, -1, -1, 'default'),
    ((1, 3, 0, 0, 0, 1, 0, 0), (40, 30), 5, 17, 17, 'tensor', 'none', 'none', 0, 0, 64, -1, -1, 'full'),
    ((1, 3, 0, 0, 0, 1, 0, 0), (6, 16), 5, 3, 17, 'tensor', 'none', 'none', 0, 0, 0, 0, -1, 'occ_forced'),
    ((1, 3, 0, 0, 1, 0, 0, 0), (6, 16), 5, 3, 17, 'order', 'none', 'none', 0, 0, 0, -1, -1, 'default/order'),
    ((1, 3, 0, 0, 1, 0, 0, 0), (6, 16), 5, 3, 5, 'greedy', 'none', 'none', 0, 0, 0, -1, -1, 'default/policy'),
    ((1, 3, 0, 0, 1, 0, 0, 0), (6, 16), 5, 3, 17, 'tensor', 'none', 'reward', 0, 0, 0, -1, -1, 'default/tables'),
    ((1, 3, 0, 0, 1, 0, 0, 0), (6, 16), 5, 17, 17, 'order', 'none', 'none', 0, 0, 64, -1, -1, 'full/order'),
    ((1, 3, 0, 0, 1, 0, 0, 0), (6, 16), 5, 17, 5, 'greedy', 'none', 'none', 0, 0, 64, -1, -1, 'full/policy'),
    ((1, 3, 0, 0, 1, 0, 0, 0), (6, 16), 5, 17, 17, 'tensor', 'none', 'terminated', 0, 0, 64, -1, -1, 'full/tables'),
    ((1, 3, 0, 0, 1, 0, 0, 0), (20, 12), 5, 8193, 5, 'order', 'none', 'none', 0, 0, 0, 1, -1, 'occ_forced'),
    ((1, 3, 0, 0, 1, 1, 0, 0), (6, 16), 5, 3, 17, 'tensor', 'none', 'none', 0, 0, 0, -1, -1, 'default'),
    ((1, 3, 0, 0, 1, 1, 0, 0), (6, 16), 5, 17, 17, 'tensor', 'none', 'none', 0, 0, 64, -1, -1, 'full'),
    ((1, 3, 0, 0, 1, 1, 0, 0), (20, 12), 5, 8193, 5, 'tensor', 'none', 'none', 0, 0, 0, 1, -1, 'occ_forced'),
    ((1, 3, 0, 1, 0, 0, 0, 0), (100, 100), 5, 3, 5, 'order', 'small', 'none', 0, 0, 0, -1, -1, 'default/order'),
    ((1, 3, 0, 1, 0, 0, 0, 0), (100, 100), 5, 3, 5, 'greedy', 'small', 'none', 0, 0, 0, -1, -1, 'default/policy'),
    ((1, 3, 0, 1, 0, 0, 0, 0), (64, 48), 5, 3, 5, 'tensor', 'small', 'reward', 0, 0, 0, -1, -1, 'default/tables'),
    ((1, 3, 0, 1, 0, 0, 0, 0), (40, 30), 5, 17, 17, 'order', 'small', 'none', 0, 0, 64, -1, -1, 'full/order'),
    ((1, 3, 0, 1, 0, 0, 0, 0), (40, 30), 5, 17, 5, 'greedy', 'small', 'none', 0, 0, 64, -1, -1, 'full/policy'),
    ((1, 3, 0, 1, 0, 0, 0, 0), (40, 30), 5, 17, 17, 'tensor', 'small', 'terminated', 0, 0, 64, -1, -1, 'full/tables'),
    ((1, 3, 0, 1, 0, 0, 0, 0), (6, 16), 5, 3, 5, 'greedy', 'small', 'none', 0, 0, 0, 0, -1, 'occ_forced'),
    ((1, 3, 0, 1, 0, 1, 0, 0), (100, 100), 5, 3, 5, 'tensor', 'small', 'none', 0, 0, 0, -1, -1, 'default'),
    ((1, 3, 0, 1, 0, 1, 0, 0), (40, 30), 5, 17, 17, 'tensor', 'small', 'none', 0, 0, 64, -1, -1, 'full'),
    ((1, 3, 0, 1, 0, 1, 0, 0), (6, 16), 5, 3, 17, 'tensor', 'small', 'none', 0, 0, 0, 0, -1, 'occ_forced'),
    ((1, 3, 0, 1, 1, 0, 0, 0), (6, 16), 5, 3, 5, 'greedy_actions_out', 'none', 'none', 0, 0, 0, -1, -1, 'actions_out_only'),
    ((1, 3, 0, 1, 1, 0, 0, 0), (6, 16), 5, 3, 17, 'order', 'small', 'none', 0, 0, 0, -1, -1, 'default/order'),
    ((1, 3, 0, 1, 1, 0, 0, 0), (6, 16), 5, 3, 5, 'greedy', 'small', 'none', 0, 0, 0, -1, -1, 'default/policy'),
    ((1, 3, 0, 1, 1, 0, 0, 0), (6, 16), 5, 3, 17, 'tensor', 'small', 'reward', 0, 0, 0, -1, -1, 'default/tables'),
    ((1, 3, 0, 1, 1, 0, 0, 0), (6, 16), 5, 17, 17, 'order', 'small', 'none', 0, 0, 64, -1, -1, 'full/order'),
    ((1, 3, 0, 1, 1, 0, 0, 0), (6, 16), 5, 17, 5, 'greedy', 'small', 'none', 0, 0, 64, -1, -1, 'full/policy'),
    ((1, 3, 0, 1, 1, 0, 0, 0), (6, 16), 5, 17, 17, 'tensor', 'small', 'terminated', 0, 0, 64, -1, -1, 'full/tables'),
    ((1, 3, 0, 1, 1, 0, 0, 0), (20, 12), 5, 8193, 5, 'order', 'small', 'none', 0, 0, 0, 1, -1, 'occ_forced'),
    ((1, 3, 0, 1, 1, 1, 0, 0), (6, 16), 5, 3, 17, 'tensor', 'small', 'none', 0, 0, 0, -1, -1, 'default'),
    ((1, 3, 0, 1, 1, 1, 0, 0), (6, 16), 5, 17, 17, 'tensor', 'small', 'none', 0, 0, 64, -1, -1, 'full'),
    ((1, 3, 0, 1, 1, 1, 0, 0), (20, 12), 5, 8193, 5, 'tensor', 'small', 'none', 0, 0, 0, 1, -1, 'occ_forced'),
    ((1, 3, 0, 2, 0, 0, 0, 0), (100, 100), 5, 3, 5, 'order', 'rows', 'none', 0, 0, 0, -1, -1, 'default/order/off_lines'),
    ((1, 3, 0, 2, 0, 0, 0, 0), (100, 100), 5, 3, 5, 'greedy', 'rows', 'none', 0, 0, 0, -1, -1, 'default/policy/off_lines'),
    ((1, 3, 0, 2, 0, 0, 0, 0), (64, 48), 5, 3, 5, 'tensor', 'rows', 'reward', 0, 0, 0, -1, -1, 'default/tables/off_lines'),
    ((1, 3, 0, 2, 0, 0, 0, 0), (40, 30), 5, 17, 17, 'order', 'rows', 'none', 0, 0, 64, -1, -1, 'full/order/off_lines'),
    ((1, 3, 0, 2, 0, 0, 0, 0), (40, 30), 5, 17, 5, 'greedy', 'rows', 'none', 0, 0, 64, -1, -1, 'full/policy/off_lines'),
    ((1, 3, 0, 2, 0, 0, 0, 0), (40, 30), 5, 17, 17, 'tensor', 'rows', 'terminated', 0, 0, 64, -1, -1, 'full/tables/off_lines'),
    ((1, 3, 0, 2, 0, 0, 0, 0), (6, 16), 5, 3, 5, 'greedy', 'rows', 'none', 0, 0, 0, 0, -1, 'occ_forced'),
    ((1, 3, 0, 2, 0, 1, 0, 0), (100, 100), 5, 3, 5, 'tensor', 'rows', 'none', 0, 0, 0, -1, -1, 'default/off_lines'),
    ((1, 3, 0, 2, 0, 1, 0, 0), (40, 30), 5, 17, 17, 'tensor', 'rows', 'none', 0, 0, 64, -1, -1, 'full/off_lines'),
    ((1, 3, 0, 2, 0, 1, 0, 0), (6, 16), 5, 3, 17, 'tensor', 'rows', 'none', 0, 0, 0, 0, -1, 'occ_forced'),
    ((1, 3, 0, 2, 1, 0, 0, 0), (6, 16), 5, 3, 5, 'greedy_actions_out', 'rows', 'none', 0, 0, 0, -1, -1, 'actions_out'),
    ((1, 3, 0, 2, 1, 0, 0, 0), (6, 16), 5, 3, 17, 'order', 'rows', 'none', 0, 0, 0, -1, -1, 'default/order/off_lines'),
    ((1, 3, 0, 2, 1, 0, 0, 0), (6, 16), 5, 3, 5, 'greedy', 'rows', 'none', 0, 0, 0, -1, -1, 'default/policy/off_lines'),
    ((1, 3, 0, 2, 1, 0, 0, 0), (6, 16), 5, 3, 17, 'tensor', 'rows', 'reward', 0, 0, 0, -1, -1, 'default/tables/off_lines'),
    ((1, 3, 0, 2, 1, 0, 0, 0), (6, 16), 5, 17, 17, 'order', 'rows', 'none', 0, 0, 64, -1, -1, 'full/order/off_lines'),
    ((1, 3, 0, 2, 1, 0, 0, 0), (6, 16), 5, 17, 5, 'greedy', 'rows', 'none', 0, 0, 64, -1, -1, 'full/policy/off_lines'),
    ((1, 3, 0, 2, 1, 0, 0, 0), (6, 16), 5, 17, 17, 'tensor', 'rows', 'terminated', 0, 0, 64, -1, -1, 'full/tables/off_lines'),
    ((1, 3, 0, 2, 1, 0, 0, 0), (20, 12), 5, 8193, 5, 'order', 'rows', 'none', 0, 0, 0, 1, -1, 'occ_forced'),
    ((1, 3, 0, 2, 1, 1, 0, 0), (6, 16), 5, 3, 17, 'tensor', 'rows', 'none', 0, 0, 0, -1, -1, 'default/off_lines'),
    ((1, 3, 0, 2, 1, 1, 0, 0), (6, 16), 5, 17, 17, 'tensor', 'rows', 'none', 0, 0, 64, -1, -1, 'full/off_lines'),
    ((1, 3, 0, 2, 1, 1, 0, 0), (20, 12), 5, 8193, 5, 'tensor', 'rows', 'none', 0, 0, 0, 1, -1, 'occ_forced'),
    ((1, 3, 0, 3, 0, 0, 0, 0), (64, 48), 7, 8193, 5, 'order', 'rows', 'none', 0, 0, 0, -1, -1, 'default/order'),
    ((1, 3, 0, 3, 0, 0, 0, 0), (64, 48), 7, 8193, 5, 'greedy', 'rows', 'none', 0, 0, 0, -1, -1, 'default/policy'),
    ((1, 3, 0, 3, 0, 0, 0, 0), (40, 30), 7, 8193, 5, 'tensor', 'rows', 'reward', 0, 0, 0, -1, -1, 'default/tables'),
    ((1, 3, 0, 3, 0, 0, 0, 0), (64, 48), 7, 8193, 5, 'order', 'rows', 'none', 0, 0, 64, -1, -1, 'full/order'),
    ((1, 3, 0, 3, 0, 0, 0, 0), (64, 48), 7, 8193, 5, 'greedy', 'rows', 'none', 0, 0, 64, -1, -1, 'full/policy'),
    ((1, 3, 0, 3, 0, 0, 0, 0), (40, 30), 7, 8193, 5, 'tensor', 'rows', 'reward', 0, 0, 64, -1, -1, 'full/tables'),
    ((1, 3, 0, 3, 0, 1, 0, 0), (64, 48), 7, 8193, 5, 'tensor', 'rows', 'none', 0, 0, 0, -1, -1, 'default'),
    ((1, 3, 0, 3, 0, 1, 0, 0), (64, 48), 7, 8193, 5, 'tensor', 'rows', 'none', 0, 0, 64, -1, -1, 'full'),
    ((1, 3, 1, 0, 0, 0, 0, 0), (100, 100), 6, 3, 5, 'order', 'none', 'none', 0, 0, 0, -1, -1, 'default/order'),
    ((1, 3, 1, 0, 0, 0, 0, 0), (100, 100), 6, 3, 5, 'greedy', 'none', 'none', 0, 0, 0, -1, -1, 'default/policy'),
    ((1, 3, 1, 0, 0, 0, 0, 0), (64, 48), 6, 3, 5, 'tensor', 'none', 'reward', 0, 0, 0, -1, -1, 'default/tables'),
    ((1, 3, 1, 0, 0, 0, 0, 0), (40, 30), 6, 17, 17, 'order', 'none', 'none', 0, 0, 64, -1, -1, 'full/order'),
    ((1, 3, 1, 0, 0, 0, 0, 0), (40, 30), 6, 17, 5, 'greedy', 'none', 'none', 0, 0, 64, -1, -1, 'full/policy'),
    ((1, 3, 1, 0, 0, 0, 0, 0), (40, 30), 6, 17, 17, 'tensor', 'none', 'terminated', 0, 0, 64, -1, -1, 'full/tables'),
    ((1, 3, 1, 0, 0, 0, 0, 0), (6, 16), 6, 3, 5, 'greedy', 'none', 'none', 0, 0, 0, 0, -1, 'occ_forced'),
    ((1, 3, 1, 0, 0, 1, 0, 0), (100, 100), 6, 3, 5, 'tensor', 'none', 'none', 0, 0, 0, -1, -1, 'default'),
    ((1, 3, 1, 0, 0, 1, 0, 0), (40, 30), 6, 17, 17, 'tensor', 'none', 'none', 0, 0, 64, -1, -1, 'full'),
    ((1, 3, 1, 0, 0, 1, 0, 0), (6, 16), 6, 3, 17, 'tensor', 'none', 'none', 0, 0, 0, 0, -1, 'occ_forced'),
    ((1, 3, 1, 0, 1, 0, 0, 0), (6, 16), 6, 3, 17, 'order', 'none', 'none', 0, 0, 0, -1, -1, 'default/order'),
    ((1, 3, 1, 0, 1, 0, 0, 0), (6, 16), 6, 3, 5, 'greedy', 'none', 'none', 0, 0, 0, -1, -1, 'default/policy'),
    ((1, 3, 1, 0, 1, 0, 0, 0), (6, 16), 6, 3, 17, 'tensor', 'none', 'reward', 0, 0, 0, -1, -1, 'default/tables'),
    ((1, 3, 1, 0, 1, 0, 0, 0), (6, 16), 6, 17, 17, 'order', 'none', 'none', 0, 0, 64, -1, -1, 'full/order'),
    ((1, 3, 1, 0, 1, 0, 0, 0), (6, 16), 6, 17, 5, 'greedy', 'none', 'none', 0, 0, 64, -1, -1, 'full/policy'),
    ((1, 3, 1, 0, 1, 0, 0, 0), (6, 16), 6, 17, 17, 'tensor', 'none', 'terminated', 0, 0, 64, -1, -1, 'full/tables'),
    ((1, 3, 1, 0, 1, 0, 0, 0), (20, 12), 6, 8193, 5, 'order', 'none', 'none', 0, 0, 0, 1, -1, 'occ_forced'),
    ((1, 3, 1, 0, 1, 1, 0, 0), (6, 16), 6, 3, 17, 'tensor', 'none', 'none', 0, 0, 0, -1, -1, 'default'),
    ((1, 3, 1, 0, 1, 1, 0, 0), (6, 16), 6, 17, 17, 'tensor', 'none', 'none', 0, 0, 64, -1, -1, 'full'),
    ((1, 3, 1, 0, 1, 1, 0, 0), (20, 12), 6, 8193, 5, 'tensor', 'none', 'none', 0, 0, 0, 1, -1, 'occ_forced'),
    ((1, 3, 1, 1, 0, 0, 0, 0), (100, 100), 6, 3, 5, 'order', 'small', 'none', 0, 0, 0, -1, -1, 'default/order'),
    ((1, 3, 1, 1, 0, 0, 0, 0), (100, 100), 6, 3, 5, 'greedy', 'small', 'none', 0, 0, 0, -1, -1, 'default/policy'),
    ((1, 3, 1, 1, 0, 0, 0, 0), (64, 48), 6, 3, 5, 'tensor', 'small', 'reward', 0, 0, 0, -1, -1, 'default/tables'),
    ((1, 3, 1, 1, 0, 0, 0, 0), (40, 30), 6, 17, 17, 'order', 'small', 'none', 0, 0, 64, -1, -1, 'full/order'),
    ((1, 3, 1, 1, 0, 0, 0, 0), (40, 30), 6, 17, 5, 'greedy', 'small', 'none', 0, 0, 64, -1, -1, 'full/policy'),
    ((1, 3, 1, 1, 0, 0, 0, 0), (40, 30), 6, 17, 17, 'tensor', 'small', 'terminated', 0, 0, 64, -1, -1, 'full/tables'),
    ((1, 3, 1, 1, 0, 0, 0, 0), (6, 16), 6, 3, 5, 'greedy', 'small', 'none', 0, 0, 0, 0, -1, 'occ_forced'),
    ((1, 3, 1, 1, 0, 1, 0, 0), (100, 100), 6, 3, 5, 'tensor', 'small', 'none', 0, 0, 0, -1, -1, 'default'),
    ((1, 3, 1, 1, 0, 1, 0, 0), (40, 30), 6, 17, 17, 'tensor', 'small', 'none', 0, 0, 64, -1, -1, 'full'),
    ((1, 3, 1, 1, 0, 1, 0, 0), (6, 16), 6, 3, 17, 'tensor', 'small', 'none', 0, 0, 0, 0, -1, 'occ_forced'),
    ((1, 3, 1, 1, 1, 0, 0, 0), (6, 16), 6, 3, 5, 'greedy_actions_out', 'none', 'none', 0, 0, 0, -1, -1, 'actions_out_only'),
    ((1, 3, 1, 1, 1, 0, 0, 0), (6, 16), 6, 3, 17, 'order', 'small', 'none', 0, 0, 0, -1, -1, 'default/order'),
    ((1, 3, 1, 1, 1, 0, 0, 0), (6, 16), 6, 3, 5, 'greedy', 'small', 'none', 0, 0, 0, -1, -1, 'default/policy'),
    ((1, 3, 1, 1, 1, 0, 0, 0), (6, 16), 6, 3, 17, 'tensor', 'small', 'reward', 0, 0, 0, -1, -1, 'default/tables'),
    ((1, 3, 1, 1, 1, 0, 0, 0), (6, 16), 6, 17, 17, 'order', 'small', 'none', 0, 0, 64, -1, -1, 'full/order'),
    ((1, 3, 1, 1, 1, 0, 0, 0), (6, 16), 6, 17, 5, 'greedy', 'small', 'none', 0, 0, 64, -1, -1, 'full/policy'),
    ((1, 3, 1, 1, 1, 0, 0, 0), (6, 16), 6, 17, 17, 'tensor', 'small', 'terminated', 0, 0, 64, -1, -1, 'full/tables'),
    ((1, 3, 1, 1, 1, 0, 0, 0), (20, 12), 6, 8193, 5, 'order', 'small', 'none', 0, 0, 0, 1, -1, 'occ_forced'),
    ((1, 3, 1, 1, 1, 1, 0, 0), (6, 16), 6, 3, 17, 'tensor', 'small', 'none', 0, 0, 0, -1, -1, 'default'),
    ((1, 3, 1, 1, 1, 1, 0, 0), (6, 16), 6, 17, 17, 'tensor', 'small', 'none', 0, 0, 64, -1, -1, 'full'),
    ((1, 3, 1, 1, 1, 1, 0, 0), (20, 12), 6, 8193, 5, 'tensor', 'small', 'none', 0, 0, 0, 1, -1, 'occ_forced'),
    ((1, 3, 1, 2, 0, 0, 0, 0), (100, 100), 6, 3, 5, 'order', 'rows', 'none', 0, 0, 0, -1, -1, 'default/order/off_lines'),
    ((1, 3, 1, 2, 0, 0, 0, 0), (100, 100), 6, 3, 5, 'greedy', 'rows', 'none', 0, 0, 0, -1, -1, 'default/policy/off_lines'),
    ((1, 3, 1, 2, 0, 0, 0, 0), (64, 48), 6, 3, 5, 'tensor', 'rows', 'reward', 0, 0, 0, -1, -1, 'default/tables/off_lines'),
    ((1, 3, 1, 2, 0, 0, 0, 0), (40, 30), 6, 17, 17, 'order', 'rows', 'none', 0, 0, 64, -1, -1, 'full/order/off_lines'),
    ((1, 3, 1, 2, 0, 0, 0, 0), (40, 30), 6, 8, 17, 'order', 'rows16', 'none', 0, 0, 64, -1, -1, 'full/order/residue16'),
    ((1, 3, 1, 2, 0, 0, 0, 0), (40, 30), 6, 17, 5, 'greedy', 'rows', 'none', 0, 0, 64, -1, -1, 'full/policy/off_lines'),
    ((1, 3, 1, 2, 0, 0, 0, 0), (40, 30), 6, 8, 5, 'greedy', 'rows16', 'none', 0, 0, 64, -1, -1, 'full/policy/residue16'),
    ((1, 3, 1, 2, 0, 0, 0, 0), (40, 30), 6, 17, 17, 'tensor', 'rows', 'terminated', 0, 0, 64, -1, -1, 'full/tables/off_lines'),
    ((1, 3, 1, 2, 0, 0, 0, 0), (40, 30), 6, 8, 17, 'tensor', 'rows16', 'terminated', 0, 0, 64, -1, -1, 'full/tables/residue16'),
    ((1, 3, 1, 2, 0, 0, 0, 0), (6, 16), 6, 3, 5, 'greedy', 'rows', 'none', 0, 0, 0, 0, -1, 'occ_forced'),
    ((1, 3, 1, 2, 0, 1, 0, 0), (100, 100), 6, 3, 5, 'tensor', 'rows', 'none', 0, 0, 0, -1, -1, 'default/off_lines'),
    ((1, 3, 1, 2, 0, 1, 0, 0), (40, 30), 6, 17, 17, 'tensor', 'rows', 'none', 0, 0, 64, -1, -1, 'full/off_lines'),
    ((1, 3, 1, 2, 0, 1, 0, 0), (40, 30), 6, 8, 17, 'tensor', 'rows16', 'none', 0, 0, 64, -1, -1, 'full/residue16'),
    ((1, 3, 1, 2, 0, 1, 0, 0), (6, 16), 6, 3, 17, 'tensor', 'rows', 'none', 0, 0, 0, 0, -1, 'occ_forced'),
    ((1, 3, 1, 2, 1, 0, 0, 0), (6, 16), 6, 3, 5, 'greedy_actions_out', 'rows', 'none', 0, 0, 0, -1, -1, 'actions_out'),
    ((1, 3, 1, 2, 1, 0, 0, 0), (6, 16), 6, 3, 17, 'order', 'rows', 'none', 0, 0, 0, -1, -1, 'default/order/off_lines'),
    ((1, 3, 1, 2, 1, 0, 0, 0), (6, 16), 6, 3, 5, 'greedy', 'rows', 'none', 0, 0, 0, -1, -1, 'default/policy/off_lines'),
    ((1, 3, 1, 2, 1, 0, 0, 0), (6, 16), 6, 3, 17, 'tensor', 'rows', 'reward', 0, 0, 0, -1, -1, 'default/tables/off_lines'),
    ((1, 3, 1, 2, 1, 0, 0, 0), (6, 16), 6, 17, 17, 'order', 'rows', 'none', 0, 0, 64, -1, -1, 'full/order/off_lines'),
    ((1, 3, 1, 2, 1, 0, 0, 0), (6, 16), 6, 8, 17, 'order', 'rows16', 'none', 0, 0, 64, -1, -1, 'full/order/residue16'),
    ((1, 3, 1, 2, 1, 0, 0, 0), (6, 16), 6, 17, 5, 'greedy', 'rows', 'none', 0, 0, 64, -1, -1, 'full/policy/off_lines'),
    ((1, 3, 1, 2, 1, 0, 0, 0), (6, 16), 6, 8, 5, 'greedy', 'rows16', 'none', 0, 0, 64, -1, -1, 'full/policy/residue16'),
    ((1, 3, 1, 2, 1, 0, 0, 0), (6, 16), 6, 17, 17, 'tensor', 'rows', 'terminated', 0, 0, 64, -1, -1, 'full/tables/off_lines'),
    ((1, 3, 1, 2, 1, 0, 0, 0), (6, 16), 6, 8, 17, 'tensor', 'rows16', 'terminated', 0, 0, 64, -1, -1, 'full/tables/residue16'),
    ((1, 3, 1, 2, 1, 0, 0, 0), (20, 12), 6, 8193, 5, 'order', 'rows', 'none', 0, 0, 0, 1, -1, 'occ_forced'),
    ((1, 3, 1, 2, 1, 1, 0, 0), (6, 16), 6, 3, 17, 'tensor', 'rows', 'none', 0, 0, 0, -1, -1, 'default/off_lines'),
    ((1, 3, 1, 2, 1, 1, 0, 0), (6, 16), 6, 17, 17, 'tensor', 'rows', 'none', 0, 0, 64, -1, -1, 'full/off_lines'),
    ((1, 3, 1, 2, 1, 1, 0, 0), (6, 16), 6, 8, 17, 'tensor', 'rows16', 'none', 0, 0, 64, -1, -1, 'full/residue16'),
    ((1, 3, 1, 2, 1, 1, 0, 0), (20, 12), 6, 8193, 5, 'tensor', 'rows', 'none', 0, 0, 0, 1, -1, 'occ_forced'),
    ((1, 4, 0, 0, 0, 0, 0, 0), (100, 100), 9, 3, 5, 'order', 'none', 'none', 0, 0, 0, -1, -1, 'default/order'),
    ((1, 4, 0, 0, 0, 0, 0, 0), (100, 100), 9, 3, 5, 'greedy', 'none', 'none', 0, 0, 0, -1, -1, 'default/policy'),
    ((1, 4, 0, 0, 0, 0, 0, 0), (64, 48), 9, 3, 5, 'tensor', 'none', 'reward', 0, 0, 0, -1, -1, 'default/tables'),
    ((1, 4, 0, 0, 0, 0, 0, 0), (64, 48), 9, 9, 17, 'order', 'none', 'none', 0, 0, 64, -1, -1, 'full/order'),
    ((1, 4, 0, 0, 0, 0, 0, 0), (64, 48), 9, 9, 5, 'greedy', 'none', 'none', 0, 0, 64, -1, -1, 'full/policy'),
    ((1, 4, 0, 0, 0, 0, 0, 0), (64, 48), 9, 9, 17, 'tensor', 'none', 'terminated', 0, 0, 64, -1, -1, 'full/tables'),
    ((1, 4, 0, 0, 0, 0, 0, 0), (6, 16), 9, 3, 5, 'greedy', 'none', 'none', 0, 0, 0, 0, -1, 'occ_forced'),
    ((1, 4, 0, 0, 0, 1, 0, 0), (100, 100), 9, 3, 5, 'tensor', 'none', 'none', 0, 0, 0, -1, -1, 'default'),
    ((1, 4, 0, 0, 0, 1, 0, 0), (64, 48), 9, 9, 17, 'tensor', 'none', 'none', 0, 0, 64, -1, -1, 'full'),
    ((1, 4, 0, 0, 0, 1, 0, 0), (6, 16), 9, 3, 17, 'tensor', 'none', 'none', 0, 0, 0, 0, -1, 'occ_forced'),
    ((1, 4, 0, 0, 1, 0, 0, 0), (6, 16), 9, 3, 17, 'order', 'none', 'none', 0, 0, 0, -1, -1, 'default/order'),
    ((1, 4, 0, 0, 1, 0, 0, 0), (6, 16), 9, 3, 5, 'greedy', 'none', 'none', 0, 0, 0, -1, -1, 'default/policy'),
    ((1, 4, 0, 0, 1, 0, 0, 0), (6, 16), 9, 3, 17, 'tensor', 'none', 'reward', 0, 0, 0, -1, -1, 'default/tables'),
    ((1, 4, 0, 0, 1, 0, 0, 0), (6, 16), 9, 9, 17, 'order', 'none', 'none', 0, 0, 64, -1, -1, 'full/order'),
    ((1, 4, 0, 0, 1, 0, 0, 0), (6, 16), 9, 9, 5, 'greedy', 'none', 'none', 0, 0, 64, -1, -1, 'full/policy'),
    ((1, 4, 0, 0, 1, 0, 0, 0), (6, 16), 9, 9, 17, 'tensor', 'none', 'terminated', 0, 0, 64, -1, -1, 'full/tables'),
    ((1, 4, 0, 0, 1, 0, 0, 0), (32, 16), 9, 3073, 5, 'tensor', 'none', 'reward', 0, 0, 0, 1, -1, 'occ_forced'),
    ((1, 4, 0, 0, 1, 1, 0, 0), (6, 16), 9, 3, 17, 'tensor', 'none', 'none', 0, 0, 0, -1, -1, 'default'),
    ((1, 4, 0, 0, 1, 1, 0, 0), (6, 16), 9, 9, 17, 'tensor', 'none', 'none', 0, 0, 64, -1, -1, 'full'),
    ((1, 4, 0, 0, 1, 1, 0, 0), (32, 16), 13, 3073, 17, 'tensor', 'none', 'none', 0, 0, 0, 1, -1, 'occ_forced'),
    ((1, 4, 0, 1, 0, 0, 0, 0), (100, 100), 9, 3, 5, 'order', 'small', 'none', 0, 0, 0, -1, -1, 'default/order'),
    ((1, 4, 0, 1, 0, 0, 0, 0), (100, 100), 9, 3, 5, 'greedy', 'small', 'none', 0, 0, 0, -1, -1, 'default/policy'),
    ((1, 4, 0, 1, 0, 0, 0, 0), (64, 48), 9, 3, 5, 'tensor', 'small', 'reward', 0, 0, 0, -1, -1, 'default/tables'),
    ((1, 4, 0, 1, 0, 0, 0, 0), (64, 48), 9, 9, 17, 'order', 'small', 'none', 0, 0, 64, -1, -1, 'full/order'),
    ((1, 4, 0, 1, 0, 0, 0, 0), (64, 48), 9, 9, 5, 'greedy', 'small', 'none', 0, 0, 64, -1, -1, 'full/policy'),
    ((1, 4, 0, 1, 0, 0, 0, 0), (64, 48), 9, 9, 17, 'tensor', 'small', 'terminated', 0, 0, 64, -1, -1, 'full/tables'),
    ((1, 4, 0, 1, 0, 0, 0, 0), (6, 16), 9, 3, 5, 'greedy', 'small', 'none', 0, 0, 0, 0, -1, 'occ_forced'),
    ((1, 4, 0, 1, 0, 1, 0, 0), (100, 100), 9, 3, 5, 'tensor', 'small', 'none', 0, 0, 0, -1, -1, 'default'),
    ((1, 4, 0, 1, 0, 1, 0, 0), (64, 48), 9, 9, 17, 'tensor', 'small', 'none', 0, 0, 64, -1, -1, 'full'),
    ((1, 4, 0, 1, 0, 1, 0, 0), (6, 16), 9, 3, 17, 'tensor', 'small', 'none', 0, 0, 0, 0, -1, 'occ_forced'),
    ((1, 4, 0, 1, 1, 0, 0, 0), (6, 16), 9, 3, 5, 'greedy_actions_out', 'none', 'none', 0, 0, 0, -1, -1, 'actions_out_only'),
    ((1, 4, 0, 1, 1, 0, 0, 0), (6, 16), 9, 3, 17, 'order', 'small', 'none', 0, 0, 0, -1, -1, 'default/order'),
    ((1, 4, 0, 1, 1, 0, 0, 0), (6, 16), 9, 3, 5, 'greedy', 'small', 'none', 0, 0, 0, -1, -1, 'default/policy'),
    ((1, 4, 0, 1, 1, 0, 0, 0), (6, 16), 9, 3, 17, 'tensor', 'small', 'reward', 0, 0, 0, -1, -1, 'default/tables'),
    ((1, 4, 0, 1, 1, 0, 0, 0), (6, 16), 9, 9, 17, 'order', 'small', 'none', 0, 0, 64, -1, -1, 'full/order'),
    ((1, 4, 0, 1, 1, 0, 0, 0), (6, 16), 9, 9, 5, 'greedy', 'small', 'none', 0, 0, 64, -1, -1, 'full/policy'),
    ((1, 4, 0, 1, 1, 0, 0, 0), (6, 16), 9, 9, 17, 'tensor', 'small', 'terminated', 0, 0, 64, -1, -1, 'full/tables'),
    ((1, 4, 0, 1, 1, 0, 0, 0), (32, 16), 9, 3073, 5, 'tensor', 'small', 'reward', 0, 0, 0, 1, -1, 'occ_forced'),
    ((1, 4, 0, 1, 1, 1, 0, 0), (6, 16), 9, 3, 17, 'tensor', 'small', 'none', 0, 0, 0, -1, -1, 'default'),
    ((1, 4, 0, 1, 1, 1, 0, 0), (6, 16), 9, 9, 17, 'tensor', 'small', 'none', 0, 0, 64, -1, -1, 'full'),
    ((1, 4, 0, 1, 1, 1, 0, 0), (32, 16), 13, 3073, 17, 'tensor', 'small', 'none', 0, 0, 0, 1, -1, 'occ_forced'),
    ((1, 4, 0, 2, 0, 0, 0, 0), (100, 100), 9, 3, 5, 'order', 'rows', 'none', 0, 0, 0, -1, -1, 'default/order/off_lines'),
    ((1, 4, 0, 2, 0, 0, 0, 0), (100, 100), 9, 3, 5, 'greedy', 'rows', 'none', 0, 0, 0, -1, -1, 'default/policy/off_lines'),
    ((1, 4, 0, 2, 0, 0, 0, 0), (64, 48), 9, 3, 5, 'tensor', 'rows', 'reward', 0, 0, 0, -1, -1, 'default/tables/off_lines'),
    ((1, 4, 0, 2, 0, 0, 0, 0), (64, 48), 9, 16, 17, 'order', 'rows', 'none', 0, 0, 64, -1, -1, 'full/order/off_lines'),
    ((1, 4, 0, 2, 0, 0, 0, 0), (64, 48), 9, 16, 5, 'greedy', 'rows', 'none', 0, 0, 64, -1, -1, 'full/policy/off_lines'),
    ((1, 4, 0, 2, 0, 0, 0, 0), (64, 48), 9, 16, 17, 'tensor', 'rows', 'terminated', 0, 0, 64, -1, -1, 'full/tables/off_lines'),
    ((1, 4, 0, 2, 0, 0, 0, 0), (6, 16), 9, 3, 5, 'greedy', 'rows', 'none', 0, 0, 0, 0, -1, 'occ_forced'),
    ((1, 4, 0, 2, 0, 1, 0, 0), (100, 100), 9, 3, 5, 'tensor', 'rows', 'none', 0, 0, 0, -1, -1, 'default/off_lines'),
    ((1, 4, 0, 2, 0, 1, 0, 0), (64, 48), 9, 16, 17, 'tensor', 'rows', 'none', 0, 0, 64, -1, -1, 'full/off_lines'),
    ((1, 4, 0, 2, 0, 1, 0, 0), (6, 16), 9, 3, 17, 'tensor', 'rows', 'none', 0, 0, 0, 0, -1, 'occ_forced'),
    ((1, 4, 0, 2, 1, 0, 0, 0), (6, 16), 9, 3, 5, 'greedy_actions_out', 'rows', 'none', 0, 0, 0, -1, -1, 'actions_out'),
    ((1, 4, 0, 2, 1, 0, 0, 0), (6, 16), 9, 3, 17, 'order', 'rows', 'none', 0, 0, 0, -1, -1, 'default/order/off_lines'),
    ((1, 4, 0, 2, 1, 0, 0, 0), (6, 16), 9, 3, 5, 'greedy', 'rows', 'none', 0, 0, 0, -1, -1, 'default/policy/off_lines'),
    ((1, 4, 0, 2, 1, 0, 0, 0), (6, 16), 9, 3, 17, 'tensor', 'rows', 'reward', 0, 0, 0, -1, -1, 'default/tables/off_lines'),
    ((1, 4, 0, 2, 1, 0, 0, 0), (6, 16), 9, 16, 17, 'order', 'rows', 'none', 0, 0, 64, -1, -1, 'full/order/off_lines'),
    ((1, 4, 0, 2, 1, 0, 0, 0), (6, 16), 9, 16, 5, 'greedy', 'rows', 'none', 0, 0, 64, -1, -1, 'full/policy/off_lines'),
    ((1, 4, 0, 2, 1, 0, 0, 0), (6, 16), 9, 16, 17, 'tensor', 'rows', 'terminated', 0, 0, 64, -1, -1, 'full/tables/off_lines'),
    ((1, 4, 0, 2, 1, 0, 0, 0), (32, 16), 9, 3073, 5, 'tensor', 'rows', 'reward', 0, 0, 0, 1, -1, 'occ_forced'),
    ((1, 4, 0, 2, 1, 1, 0, 0), (6, 16), 9, 3, 17, 'tensor', 'rows', 'none', 0, 0, 0, -1, -1, 'default/off_lines'),
    ((1, 4, 0, 2, 1, 1, 0, 0), (6, 16), 9, 16, 17, 'tensor', 'rows', 'none', 0, 0, 64, -1, -1, 'full/off_lines'),
    ((1, 4, 0, 2, 1, 1, 0, 0), (32, 16), 13, 4096, 17, 'tensor', 'rows', 'none', 0, 0, 0, 1, -1, 'occ_forced'),
    ((1, 4, 0, 3, 0, 0, 0, 0), (64, 48), 9, 9, 17, 'order', 'rows', 'none', 0, 0, 64, -1, -1, 'full/order'),
    ((1, 4, 0, 3, 0, 0, 0, 0), (64, 48), 9, 9, 5, 'greedy', 'rows', 'none', 0, 0, 64, -1, -1, 'full/policy'),
    ((1, 4, 0, 3, 0, 0, 0, 0), (64, 48), 9, 9, 17, 'tensor', 'rows', 'terminated', 0, 0, 64, -1, -1, 'full/tables'),
    ((1, 4, 0, 3, 0, 0, 0, 0), (6, 16), 9, 9, 5, 'greedy', 'rows', 'none', 0, 0, 64, 0, -1, 'occ_forced'),
    ((1, 4, 0, 3, 0, 1, 0, 0), (64, 48), 9, 9, 17, 'tensor', 'rows', 'none', 0, 0, 64, -1, -1, 'full'),
    ((1, 4, 0, 3, 0, 1, 0, 0), (6, 16), 9, 9, 17, 'tensor', 'rows', 'none', 0, 0, 64, 0, -1, 'occ_forced'),
    ((1, 4, 0, 3, 1, 0, 0, 0), (6, 16), 9, 9, 17, 'order', 'rows', 'none', 0, 0, 64, -1, -1, 'full/order'),
    ((1, 4, 0, 3, 1, 0, 0, 0), (6, 16), 9, 9, 5, 'greedy', 'rows', 'none', 0, 0, 64, -1, -1, 'full/policy'),
    ((1, 4, 0, 3, 1, 0, 0, 0), (6, 16), 9, 9, 17, 'tensor', 'rows', 'terminated', 0, 0, 64, -1, -1, 'full/tables'),
    ((1, 4, 0, 3, 1, 0, 0, 0), (32, 16), 9, 4097, 5, 'tensor', 'rows', 'reward', 0, 0, 0, 1, -1, 'occ_forced'),
    ((1, 4, 0, 3, 1, 1, 0, 0), (6, 16), 9, 9, 17, 'tensor', 'rows', 'none', 0, 0, 64, -1, -1, 'full'),
    ((1, 4, 0, 3, 1, 1, 0, 0), (32, 16), 13, 3073, 17, 'tensor', 'rows', 'none', 0, 0, 0, 1, -1, 'occ_forced'),
    ((1, 4, 1, 0, 0, 0, 0, 0), (100, 100), 10, 3, 5, 'order', 'none', 'none', 0, 0, 0, -1, -1, 'default/order'),
    ((1, 4, 1, 0, 0, 0, 0, 0), (100, 100), 10, 3, 5, 'greedy', 'none', 'none', 0, 0, 0, -1, -1, 'default/policy'),
    ((1, 4, 1, 0, 0, 0, 0, 0), (64, 48), 10, 3, 5, 'tensor', 'none', 'reward', 0, 0, 0, -1, -1, 'default/tables'),
    ((1, 4, 1, 0, 0, 0, 0, 0), (64, 48), 10, 9, 17, 'order', 'none', 'none', 0, 0, 64, -1, -1, 'full/order'),
    ((1, 4, 1, 0, 0, 0, 0, 0), (64, 48), 10, 9, 5, 'greedy', 'none', 'none', 0, 0, 64, -1, -1, 'full/policy'),
    ((1, 4, 1, 0, 0, 0, 0, 0), (64, 48), 10, 9, 17, 'tensor', 'none', 'terminated', 0, 0, 64, -1, -1, 'full/tables'),
    ((1, 4, 1, 0, 0, 0, 0, 0), (6, 16), 10, 3, 5, 'greedy', 'none', 'none', 0, 0, 0, 0, -1, 'occ_forced'),
    ((1, 4, 1, 0, 0, 1, 0, 0), (100, 100), 10, 3, 5, 'tensor', 'none', 'none', 0, 0, 0, -1, -1, 'default'),
    ((1, 4, 1, 0, 0, 1, 0, 0), (64, 48), 10, 9, 17, 'tensor', 'none', 'none', 0, 0, 64, -1, -1, 'full'),
    ((1, 4, 1, 0, 0, 1, 0, 0), (6, 16), 10, 3, 17, 'tensor', 'none', 'none', 0, 0, 0, 0, -1, 'occ_forced'),
    ((1, 4, 1, 0, 1, 0, 0, 0), (6, 16), 10, 3, 17, 'order', 'none', 'none', 0, 0, 0, -1, -1, 'default/order'),
    ((1, 4, 1, 0, 1, 0, 0, 0), (6, 16), 10, 3, 5, 'greedy', 'none', 'none', 0, 0, 0, -1, -1, 'default/policy'),
    ((1, 4, 1, 0, 1, 0, 0, 0), (6, 16), 10, 3, 17, 'tensor', 'none', 'reward', 0, 0, 0, -1, -1, 'default/tables'),
    ((1, 4, 1, 0, 1, 0, 0, 0), (6, 16), 10, 9, 17, 'order', 'none', 'none', 0, 0, 64, -1, -1, 'full/order'),
    ((1, 4, 1, 0, 1, 0, 0, 0), (6, 16), 10, 9, 5, 'greedy', 'none', 'none', 0, 0, 64, -1, -1, 'full/policy'),
    ((1, 4, 1, 0, 1, 0, 0, 0), (6, 16), 10, 9, 17, 'tensor', 'none', 'terminated', 0, 0, 64, -1, -1, 'full/tables'),
    ((1, 4, 1, 0, 1, 0, 0, 0), (32, 16), 10, 3073, 5, 'tensor', 'none', 'reward', 0, 0, 0, 1, -1, 'occ_forced'),
    ((1, 4, 1, 0, 1, 1, 0, 0), (6, 16), 10, 3, 17, 'tensor', 'none', 'none', 0, 0, 0, -1, -1, 'default'),
    ((1, 4, 1, 0, 1, 1, 0, 0), (6, 16), 10, 9, 17, 'tensor', 'none', 'none', 0, 0, 64, -1, -1, 'full'),
    ((1, 4, 1, 0, 1, 1, 0, 0), (32, 16), 12, 3073, 17, 'tensor', 'none', 'none', 0, 0, 0, 1, -1, 'occ_forced'),
    ((1, 4, 1, 1, 0, 0, 0, 0), (100, 100), 10, 3, 5, 'order', 'small', 'none', 0, 0, 0, -1, -1, 'default/order'),
    ((1, 4, 1, 1, 0, 0, 0, 0), (100, 100), 10, 3, 5, 'greedy', 'small', 'none', 0, 0, 0, -1, -1, 'default/policy'),
    ((1, 4, 1, 1, 0, 0, 0, 0), (64, 48), 10, 3, 5, 'tensor', 'small', 'reward', 0, 0, 0, -1, -1, 'default/tables'),
    ((1, 4, 1, 1, 0, 0, 0, 0), (64, 48), 10, 9, 17, 'order', 'small', 'none', 0, 0, 64, -1, -1, 'full/order'),
    ((1, 4, 1, 1, 0, 0, 0, 0), (64, 48), 10, 9, 5, 'greedy', 'small', 'none', 0, 0, 64, -1, -1, 'full/policy'),
    ((1, 4, 1, 1, 0, 0, 0, 0), (64, 48), 10, 9, 17, 'tensor', 'small', 'terminated', 0, 0, 64, -1, -1, 'full/tables'),
    ((1, 4, 1, 1, 0, 0, 0, 0), (6, 16), 10, 3, 5, 'greedy', 'small', 'none', 0, 0, 0, 0, -1, 'occ_forced'),
    ((1, 4, 1, 1, 0, 1, 0, 0), (100, 100), 10, 3, 5, 'tensor', 'small', 'none', 0, 0, 0, -1, -1, 'default'),
    ((1, 4, 1, 1, 0, 1, 0, 0), (64, 48), 10, 9, 17, 'tensor', 'small', 'none', 0, 0, 64, -1, -1, 'full'),
    ((1, 4, 1, 1, 0, 1, 0, 0), (6, 16), 10, 3, 17, 'tensor', 'small', 'none', 0, 0, 0, 0, -1, 'occ_forced'),
    ((1, 4, 1, 1, 1, 0, 0, 0), (6, 16), 10, 3, 5, 'greedy_actions_out', 'none', 'none', 0, 0, 0, -1, -1, 'actions_out_only'),
    ((1, 4, 1, 1, 1, 0, 0, 0), (6, 16), 10, 3, 17, 'order', 'small', 'none', 0, 0, 0, -1, -1, 'default/order'),
    ((1, 4, 1, 1, 1, 0, 0, 0), (6, 16), 10, 3, 5, 'greedy', 'small', 'none', 0, 0, 0, -1, -1, 'default/policy'),
    ((1, 4, 1, 1, 1, 0, 0, 0), (6, 16), 10, 3, 17, 'tensor', 'small', 'reward', 0, 0, 0, -1, -1, 'default/tables'),
    ((1, 4, 1, 1, 1, 0, 0, 0), (6, 16), 10, 9, 17, 'order', 'small', 'none', 0, 0, 64, -1, -1, 'full/order'),
    ((1, 4, 1, 1, 1, 0, 0, 0), (6, 16), 10, 9, 5, 'greedy', 'small', 'none', 0, 0, 64, -1, -1, 'full/policy'),
    ((1, 4, 1, 1, 1, 0, 0, 0), (6, 16), 10, 9, 17, 'tensor', 'small', 'terminated', 0, 0, 64, -1, -1, 'full/tables'),
    ((1, 4, 1, 1, 1, 0, 0, 0), (32, 16), 10, 3073, 5, 'tensor', 'small', 'reward', 0, 0, 0, 1, -1, 'occ_forced'),
    ((1, 4, 1, 1, 1, 1, 0, 0), (6, 16), 10, 3, 17, 'tensor', 'small', 'none', 0, 0, 0, -1, -1, 'default'),
    ((1, 4, 1, 1, 1, 1, 0, 0), (6, 16), 10, 9, 17, 'tensor', 'small', 'none', 0, 0, 64, -1, -1, 'full'),
    ((1, 4, 1, 1, 1, 1, 0, 0), (32, 16), 12, 3073, 17, 'tensor', 'small', 'none', 0, 0, 0, 1, -1, 'occ_forced'),
    ((1, 4, 1, 2, 0, 0, 0, 0), (100, 100), 10, 3, 5, 'order', 'rows', 'none', 0, 0, 0, -1, -1, 'default/order/off_lines'),
    ((1, 4, 1, 2, 0, 0, 0, 0), (100, 100), 16, 3, 5, 'order', 'rows16', 'none', 0, 0, 0, -1, -1, 'default/order/residue16'),
    ((1, 4, 1, 2, 0, 0, 0, 0), (100, 100), 10, 3, 5, 'greedy', 'rows', 'none', 0, 0, 0, -1, -1, 'default/policy/off_lines'),
    ((1, 4, 1, 2, 0, 0, 0, 0), (100, 100), 16, 3, 5, 'greedy', 'rows16', 'none', 0, 0, 0, -1, -1, 'default/policy/residue16'),
    ((1, 4, 1, 2, 0, 0, 0, 0), (64, 48), 10, 3, 5, 'tensor', 'rows', 'reward', 0, 0, 0, -1, -1, 'default/tables/off_lines'),
    ((1, 4, 1, 2, 0, 0, 0, 0), (64, 48), 16, 3, 5, 'tensor', 'rows16', 'reward', 0, 0, 0, -1, -1, 'default/tables/residue16'),
    ((1, 4, 1, 2, 0, 0, 0, 0), (64, 48), 10, 9, 17, 'order', 'rows', 'none', 0, 0, 64, -1, -1, 'full/order/off_lines'),
    ((1, 4, 1, 2, 0, 0, 0, 0), (64, 48), 16, 9, 17, 'order', 'rows16', 'none', 0, 0, 64, -1, -1, 'full/order/residue16'),
    ((1, 4, 1, 2, 0, 0, 0, 0), (64, 48), 10, 9, 5, 'greedy', 'rows', 'none', 0, 0, 64, -1, -1, 'full/policy/off_lines'),
    ((1, 4, 1, 2, 0, 0, 0, 0), (64, 48), 16, 9, 5, 'greedy', 'rows16', 'none', 0, 0, 64, -1, -1, 'full/policy/residue16'),
    ((1, 4, 1, 2, 0, 0, 0, 0), (64, 48), 10, 9, 17, 'tensor', 'rows', 'terminated', 0, 0, 64, -1, -1, 'full/tables/off_lines'),
    ((1, 4, 1, 2, 0, 0, 0, 0), (64, 48), 16, 9, 17, 'tensor', 'rows16', 'terminated', 0, 0, 64, -1, -1, 'full/tables/residue16'),
    ((1, 4, 1, 2, 0, 0, 0, 0), (6, 16), 10, 3, 5, 'greedy', 'rows', 'none', 0, 0, 0, 0, -1, 'occ_forced'),
    ((1, 4, 1, 2, 0, 1, 0, 0), (100, 100), 10, 3, 5, 'tensor', 'rows', 'none', 0, 0, 0, -1, -1, 'default/off_lines'),
    ((1, 4, 1, 2, 0, 1, 0, 0), (100, 100), 16, 3, 5, 'tensor', 'rows16', 'none', 0, 0, 0, -1, -1, 'default/residue16'),
    ((1, 4, 1, 2, 0, 1, 0, 0), (64, 48), 10, 9, 17, 'tensor', 'rows', 'none', 0, 0, 64, -1, -1, 'full/off_lines'),
    ((1, 4, 1, 2, 0, 1, 0, 0), (64, 48), 16, 9, 17, 'tensor', 'rows16', 'none', 0, 0, 64, -1, -1, 'full/residue16'),
    ((1, 4, 1, 2, 0, 1, 0, 0), (6, 16), 10, 3, 17, 'tensor', 'rows', 'none', 0, 0, 0, 0, -1, 'occ_forced'),
    ((1, 4, 1, 2, 1, 0, 0, 0), (6, 16), 10, 3, 5, 'greedy_actions_out', 'rows', 'none', 0, 0, 0, -1, -1, 'actions_out'),
    ((1, 4, 1, 2, 1, 0, 0, 0), (6, 16), 10, 3, 17, 'order', 'rows', 'none', 0, 0, 0, -1, -1, 'default/order/off_lines'),
    ((1, 4, 1, 2, 1, 0, 0, 0), (6, 16), 16, 3, 17, 'order', 'rows16', 'none', 0, 0, 0, -1, -1, 'default/order/residue16'),
    ((1, 4, 1, 2, 1, 0, 0, 0), (6, 16), 10, 3, 5, 'greedy', 'rows', 'none', 0, 0, 0, -1, -1, 'default/policy/off_lines'),
    ((1, 4, 1, 2, 1, 0, 0, 0), (6, 16), 16, 3, 5, 'greedy', 'rows16', 'none', 0, 0, 0, -1, -1, 'default/policy/residue16'),
    ((1, 4, 1, 2, 1, 0, 0, 0), (6, 16), 10, 3, 17, 'tensor', 'rows', 'reward', 0, 0, 0, -1, -1, 'default/tables/off_lines'),
    ((1, 4, 1, 2, 1, 0, 0, 0), (6, 16), 16, 3, 17, 'tensor', 'rows16', 'reward', 0, 0, 0, -1, -1, 'default/tables/residue16'),
    ((1, 4, 1, 2, 1, 0, 0, 0), (6, 16), 10, 9, 17, 'order', 'rows', 'none', 0, 0, 64, -1, -1, 'full/order/off_lines'),
    ((1, 4, 1, 2, 1, 0, 0, 0), (6, 16), 16, 9, 17, 'order', 'rows16', 'none', 0, 0, 64, -1, -1, 'full/order/residue16'),
    ((1, 4, 1, 2, 1, 0, 0, 0), (6, 16), 10, 9, 5, 'greedy', 'rows', 'none', 0, 0, 64, -1, -1, 'full/policy/off_lines'),
    ((1, 4, 1, 2, 1, 0, 0, 0), (6, 16), 16, 9, 5, 'greedy', 'rows16', 'none', 0, 0, 64, -1, -1, 'full/policy/residue16'),
    ((1, 4, 1, 2, 1, 0, 0, 0), (6, 16), 10, 9, 17, 'tensor', 'rows', 'terminated', 0, 0, 64, -1, -1, 'full/tables/off_lines'),
    ((1, 4, 1, 2, 1, 0, 0, 0), (6, 16), 16, 9, 17, 'tensor', 'rows16', 'terminated', 0, 0, 64, -1, -1, 'full/tables/residue16'),
    ((1, 4, 1, 2, 1, 0, 0, 0), (32, 16), 10, 3073, 5, 'tensor', 'rows', 'reward', 0, 0, 0, 1, -1, 'occ_forced'),
    ((1, 4, 1, 2, 1, 1, 0, 0), (6, 16), 10, 3, 17, 'tensor', 'rows', 'none', 0, 0, 0, -1, -1, 'default/off_lines'),
    ((1, 4, 1, 2, 1, 1, 0, 0), (6, 16), 16, 3, 17, 'tensor', 'rows16', 'none', 0, 0, 0, -1, -1, 'default/residue16'),
    ((1, 4, 1, 2, 1, 1, 0, 0), (6, 16), 10, 9, 17, 'tensor', 'rows', 'none', 0, 0, 64, -1, -1, 'full/off_lines'),
    ((1, 4, 1, 2, 1, 1, 0, 0), (6, 16), 16, 9, 17, 'tensor', 'rows16', 'none', 0, 0, 64, -1, -1, 'full/residue16'),
    ((1, 4, 1, 2, 1, 1, 0, 0), (32, 16), 12, 3073, 17, 'tensor', 'rows', 'none', 0, 0, 0, 1, -1, 'occ_forced'),
    ((1, 4, 1, 3, 0, 0, 0, 0), (40, 30), 12, 4097, 5, 'order', 'rows', 'none', 0, 0, 0, -1, -1, 'default/order'),
    ((1, 4, 1, 3, 0, 0, 0, 0), (40, 30), 12, 4097, 5, 'greedy', 'rows', 'none', 0, 0, 0, -1, -1, 'default/policy'),
    ((1, 4, 1, 3, 0, 0, 0, 0), (40, 30), 12, 4097, 5, 'tensor', 'rows', 'terminated', 0, 0, 0, -1, -1, 'default/tables'),
    ((1, 4, 1, 3, 0, 0, 0, 0), (64, 48), 12, 33, 17, 'order', 'rows', 'none', 0, 0, 64, -1, -1, 'full/order'),
    ((1, 4, 1, 3, 0, 0, 0, 0), (64, 48), 12, 33, 5, 'greedy', 'rows', 'none', 0, 0, 64, -1, -1, 'full/policy'),
    ((1, 4, 1, 3, 0, 0, 0, 0), (64, 48), 12, 33, 5, 'tensor', 'rows', 'reward', 0, 0, 64, -1, -1, 'full/tables'),
    ((1, 4, 1, 3, 0, 0, 0, 0), (6, 16), 12, 33, 5, 'greedy', 'rows', 'none', 0, 0, 64, 0, -1, 'occ_forced'),
    ((1, 4, 1, 3, 0, 1, 0, 0), (40, 30), 12, 4097, 5, 'tensor', 'rows', 'none', 0, 0, 0, -1, -1, 'default'),
    ((1, 4, 1, 3, 0, 1, 0, 0), (64, 48), 12, 33, 17, 'tensor', 'rows', 'none', 0, 0, 64, -1, -1, 'full'),
    ((1, 4, 1, 3, 0, 1, 0, 0), (6, 16), 12, 33, 17, 'tensor', 'rows', 'none', 0, 0, 64, 0, -1, 'occ_forced'),
    ((1, 4, 1, 3, 1, 0, 0, 0), (6, 16), 12, 4097, 17, 'order', 'rows', 'none', 0, 0, 0, -1, -1, 'default/order'),
    ((1, 4, 1, 3, 1, 0, 0, 0), (6, 16), 12, 4097, 5, 'greedy', 'rows', 'none', 0, 0, 0, -1, -1, 'default/policy'),
    ((1, 4, 1, 3, 1, 0, 0, 0), (6, 16), 12, 4097, 17, 'tensor', 'rows', 'terminated', 0, 0, 0, -1, -1, 'default/tables'),
    ((1, 4, 1, 3, 1, 0, 0, 0), (6, 16), 12, 33, 17, 'order', 'rows', 'none', 0, 0, 64, -1, -1, 'full/order'),
    ((1, 4, 1, 3, 1, 0, 0, 0), (6, 16), 12, 33, 5, 'greedy', 'rows', 'none', 0, 0, 64, -1, -1, 'full/policy'),
    ((1, 4, 1, 3, 1, 0, 0, 0), (6, 16), 12, 33, 17, 'tensor', 'rows', 'terminated', 0, 0, 64, -1, -1, 'full/tables'),
    ((1, 4, 1, 3, 1, 0, 0, 0), (32, 16), 12, 4097, 5, 'greedy', 'rows', 'none', 0, 0, 0, 1, -1, 'occ_forced'),
    ((1, 4, 1, 3, 1, 1, 0, 0), (6, 16), 12, 4097, 17, 'tensor', 'rows', 'none', 0, 0, 0, -1, -1, 'default'),
    ((1, 4, 1, 3, 1, 1, 0, 0), (6, 16), 12, 33, 17, 'tensor', 'rows', 'none', 0, 0, 64, -1, -1, 'full'),
    ((1, 4, 1, 3, 1, 1, 0, 0), (32, 16), 12, 4097, 17, 'tensor', 'rows', 'none', 0, 0, 0, 1, -1, 'occ_forced'),
    ((1, 5, 0, 0, 0, 0, 0, 0), (100, 100), 17, 3, 5, 'order', 'none', 'none', 0, 0, 0, -1, -1, 'default/order'),
    ((1, 5, 0, 0, 0, 0, 0, 0), (100, 100), 17, 3, 5, 'greedy', 'none', 'none', 0, 0, 0, -1, -1, 'default/policy'),
    ((1, 5, 0, 0, 0, 0, 0, 0), (64, 48), 17, 3, 5, 'tensor', 'none', 'reward', 0, 0, 0, -1, -1, 'default/tables'),
    ((1, 5, 0, 0, 0, 0, 0, 0), (100, 100), 17, 5, 5, 'order', 'none', 'none', 0, 0, 64, -1, -1, 'full/order'),
    ((1, 5, 0, 0, 0, 0, 0, 0), (100, 100), 17, 5, 5, 'greedy', 'none', 'none', 0, 0, 64, -1, -1, 'full/policy'),
    ((1, 5, 0, 0, 0, 0, 0, 0), (64, 48), 23, 33, 5, 'tensor', 'none', 'reward', 0, 0, 64, -1, -1, 'full/tables'),
    ((1, 5, 0, 0, 0, 0, 0, 0), (6, 16), 17, 3, 5, 'greedy', 'none', 'none', 0, 0, 0, 0, -1, 'occ_forced'),
    ((1, 5, 0, 0, 0, 1, 0, 0), (100, 100), 17, 3, 5, 'tensor', 'none', 'none', 0, 0, 0, -1, -1, 'default'),
    ((1, 5, 0, 0, 0, 1, 0, 0), (100, 100), 17, 5, 5, 'tensor', 'none', 'none', 0, 0, 64, -1, -1, 'full'),
    ((1, 5, 0, 0, 0, 1, 0, 0), (6, 16), 17, 3, 17, 'tensor', 'none', 'none', 0, 0, 0, 0, -1, 'occ_forced'),
    ((1, 5, 0, 0, 1, 0, 0, 0), (6, 16), 17, 3, 17, 'order', 'none', 'none', 0, 0, 0, -1, -1, 'default/order'),
    ((1, 5, 0, 0, 1, 0, 0, 0), (6, 16), 17, 3, 5, 'greedy', 'none', 'none', 0, 0, 0, -1, -1, 'default/policy'),
    ((1, 5, 0, 0, 1, 0, 0, 0), (6, 16), 17, 3, 17, 'tensor', 'none', 'reward', 0, 0, 0, -1, -1, 'default/tables'),
    ((1, 5, 0, 0, 1, 0, 0, 0), (6, 16), 17, 5, 17, 'order', 'none', 'none', 0, 0, 64, -1, -1, 'full/order'),
    ((1, 5, 0, 0, 1, 0, 0, 0), (6, 16), 17, 5, 5, 'greedy', 'none', 'none', 0, 0, 64, -1, -1, 'full/policy'),
    ((1, 5, 0, 0, 1, 0, 0, 0), (6, 16), 17, 5, 17, 'tensor', 'none', 'terminated', 0, 0, 64, -1, -1, 'full/tables'),
    ((1, 5, 0, 0, 1, 1, 0, 0), (6, 16), 17, 3, 17, 'tensor', 'none', 'none', 0, 0, 0, -1, -1, 'default'),
    ((1, 5, 0, 0, 1, 1, 0, 0), (6, 16), 17, 5, 17, 'tensor', 'none', 'none', 0, 0, 64, -1, -1, 'full'),
    ((1, 5, 0, 1, 0, 0, 0, 0), (100, 100), 17, 3, 5, 'order', 'small', 'none', 0, 0, 0, -1, -1, 'default/order'),
    ((1, 5, 0, 1, 0, 0, 0, 0), (100, 100), 17, 3, 5, 'greedy', 'small', 'none', 0, 0, 0, -1, -1, 'default/policy'),
    ((1, 5, 0, 1, 0, 0, 0, 0), (64, 48), 17, 3, 5, 'tensor', 'small', 'reward', 0, 0, 0, -1, -1, 'default/tables'),
    ((1, 5, 0, 1, 0, 0, 0, 0), (100, 100), 17, 5, 5, 'order', 'small', 'none', 0, 0, 64, -1, -1, 'full/order'),
    ((1, 5, 0, 1, 0, 0, 0, 0), (100, 100), 17, 5, 5, 'greedy', 'small', 'none', 0, 0, 64, -1, -1, 'full/policy'),
    ((1, 5, 0, 1, 0, 0, 0, 0), (64, 48), 23, 33, 5, 'tensor', 'small', 'reward', 0, 0, 64, -1, -1, 'full/tables'),
    ((1, 5, 0, 1, 0, 0, 0, 0), (6, 16), 17, 3, 5, 'greedy', 'small', 'none', 0, 0, 0, 0, -1, 'occ_forced'),
    ((1, 5, 0, 1, 0, 1, 0, 0), (100, 100), 17, 3, 5, 'tensor', 'small', 'none', 0, 0, 0, -1, -1, 'default'),
    ((1, 5, 0, 1, 0, 1, 0, 0), (100, 100), 17, 5, 5, 'tensor', 'small', 'none', 0, 0, 64, -1, -1, 'full'),
    ((1, 5, 0, 1, 0, 1, 0, 0), (6, 16), 17, 3, 17, 'tensor', 'small', 'none', 0, 0, 0, 0, -1, 'occ_forced'),
    ((1, 5, 0, 1, 1, 0, 0, 0), (6, 16), 17, 3, 5, 'greedy_actions_out', 'none', 'none', 0, 0, 0, -1, -1, 'actions_out_only'),
    ((1, 5, 0, 1, 1, 0, 0, 0), (6, 16), 17, 3, 17, 'order', 'small', 'none', 0, 0, 0, -1, -1, 'default/order'),
    ((1, 5, 0, 1, 1, 0, 0, 0), (6, 16), 17, 3, 5, 'greedy', 'small', 'none', 0, 0, 0, -1, -1, 'default/policy'),
    ((1, 5, 0, 1, 1, 0, 0, 0), (6, 16), 17, 3, 17, 'tensor', 'small', 'reward', 0, 0, 0, -1, -1, 'default/tables'),
    ((1, 5, 0, 1, 1, 0, 0, 0), (6, 16), 17, 5, 17, 'order', 'small', 'none', 0, 0, 64, -1, -1, 'full/order'),
    ((1, 5, 0, 1, 1, 0, 0, 0), (6, 16), 17, 5, 5, 'greedy', 'small', 'none', 0, 0, 64, -1, -1, 'full/policy'),
    ((1, 5, 0, 1, 1, 0, 0, 0), (6, 16), 17, 5, 17, 'tensor', 'small', 'terminated', 0, 0, 64, -1, -1, 'full/tables'),
    ((1, 5, 0, 1, 1, 1, 0, 0), (6, 16), 17, 3, 17, 'tensor', 'small', 'none', 0, 0, 0, -1, -1, 'default'),
    ((1, 5, 0, 1, 1, 1, 0, 0), (6, 16), 17, 5, 17, 'tensor', 'small', 'none', 0, 0, 64, -1, -1, 'full'),
    ((1, 5, 0, 2, 0, 0, 0, 0), (100, 100), 17, 3, 5, 'order', 'rows', 'none', 0, 0, 0, -1, -1, 'default/order/off_lines'),
    ((1, 5, 0, 2, 0, 0, 0, 0), (100, 100), 17, 3, 5, 'greedy', 'rows', 'none', 0, 0, 0, -1, -1, 'default/policy/off_lines'),
    ((1, 5, 0, 2, 0, 0, 0, 0), (64, 48), 17, 3, 5, 'tensor', 'rows', 'reward', 0, 0, 0, -1, -1, 'default/tables/off_lines'),
    ((1, 5, 0, 2, 0, 0, 0, 0), (100, 100), 17, 5, 5, 'order', 'rows', 'none', 0, 0, 64, -1, -1, 'full/order/off_lines'),
    ((1, 5, 0, 2, 0, 0, 0, 0), (100, 100), 17, 5, 5, 'greedy', 'rows', 'none', 0, 0, 64, -1, -1, 'full/policy/off_lines'),
    ((1, 5, 0, 2, 0, 0, 0, 0), (100, 100), 17, 5, 5, 'tensor', 'rows', 'terminated', 0, 0, 64, -1, -1, 'full/tables/off_lines'),
    ((1, 5, 0, 2, 0, 0, 0, 0), (6, 16), 17, 3, 5, 'greedy', 'rows', 'none', 0, 0, 0, 0, -1, 'occ_forced'),
    ((1, 5, 0, 2, 0, 1, 0, 0), (100, 100), 17, 3, 5, 'tensor', 'rows', 'none', 0, 0, 0, -1, -1, 'default/off_lines'),
    ((1, 5, 0, 2, 0, 1, 0, 0), (100, 100), 17, 5, 5, 'tensor', 'rows', 'none', 0, 0, 64, -1, -1, 'full/off_lines'),
    ((1, 5, 0, 2, 0, 1, 0, 0), (6, 16), 17, 3, 17, 'tensor', 'rows', 'none', 0, 0, 0, 0, -1, 'occ_forced'),
    ((1, 5, 0, 2, 1, 0, 0, 0), (6, 16), 17, 3, 5, 'greedy_actions_out', 'rows', 'none', 0, 0, 0, -1, -1, 'actions_out'),
    ((1, 5, 0, 2, 1, 0, 0, 0), (6, 16), 17, 3, 17, 'order', 'rows', 'none', 0, 0, 0, -1, -1, 'default/order/off_lines'),
    ((1, 5, 0, 2, 1, 0, 0, 0), (6, 16), 17, 3, 5, 'greedy', 'rows', 'none', 0, 0, 0, -1, -1, 'default/policy/off_lines'),
    ((1, 5, 0, 2, 1, 0, 0, 0), (6, 16), 17, 3, 17, 'tensor', 'rows', 'reward', 0, 0, 0, -1, -1, 'default/tables/off_lines'),
    ((1, 5, 0, 2, 1, 0, 0, 0), (6, 16), 17, 5, 17, 'order', 'rows', 'none', 0, 0, 64, -1, -1, 'full/order/off_lines'),
    ((1, 5, 0, 2, 1, 0, 0, 0), (6, 16), 17, 5, 5, 'greedy', 'rows', 'none', 0, 0, 64, -1, -1, 'full/policy/off_lines'),
    ((1, 5, 0, 2, 1, 0, 0, 0), (6, 16), 17, 5, 17, 'tensor', 'rows', 'terminated', 0, 0, 64, -1, -1, 'full/tables/off_lines'),
    ((1, 5, 0, 2, 1, 1, 0, 0), (6, 16), 17, 3, 17, 'tensor', 'rows', 'none', 0, 0, 0, -1, -1, 'default/off_lines'),
    ((1, 5, 0, 2, 1, 1, 0, 0), (6, 16), 17, 5, 17, 'tensor', 'rows', 'none', 0, 0, 64, -1, -1, 'full/off_lines'),
    ((1, 5, 0, 3, 0, 0, 0, 0), (100, 100), 25, 3, 5, 'order', 'rows', 'none', 0, 0, 0, -1, -1, 'default/order'),
    ((1, 5, 0, 3, 0, 0, 0, 0), (100, 100), 25, 3, 5, 'greedy', 'rows', 'none', 0, 0, 0, -1, -1, 'default/policy'),
    ((1, 5, 0, 3, 0, 0, 0, 0), (64, 48), 25, 3, 5, 'tensor', 'rows', 'reward', 0, 0, 0, -1, -1, 'default/tables'),
    ((1, 5, 0, 3, 0, 0, 0, 0), (100, 100), 23, 33, 5, 'order', 'rows', 'none', 0, 0, 64, -1, -1, 'full/order'),
    ((1, 5, 0, 3, 0, 0, 0, 0), (100, 100), 23, 33, 5, 'greedy', 'rows', 'none', 0, 0, 64, -1, -1, 'full/policy'),
    ((1, 5, 0, 3, 0, 0, 0, 0), (64, 48), 23, 33, 5, 'tensor', 'rows', 'reward', 0, 0, 64, -1, -1, 'full/tables'),
    ((1, 5, 0, 3, 0, 0, 0, 0), (20, 12), 25, 3, 5, 'greedy', 'rows', 'none', 0, 0, 0, 0, -1, 'occ_forced'),
    ((1, 5, 0, 3, 0, 1, 0, 0), (100, 100), 25, 3, 5, 'tensor', 'rows', 'none', 0, 0, 0, -1, -1, 'default'),
    ((1, 5, 0, 3, 0, 1, 0, 0), (100, 100), 23, 33, 5, 'tensor', 'rows', 'none', 0, 0, 64, -1, -1, 'full'),
    ((1, 5, 0, 3, 0, 1, 0, 0), (20, 12), 25, 3, 17, 'tensor', 'rows', 'none', 0, 0, 0, 0, -1, 'occ_forced'),
    ((1, 5, 0, 3, 1, 0, 0, 0), (20, 12), 25, 3, 17, 'order', 'rows', 'none', 0, 0, 0, -1, -1, 'default/order'),
    ((1, 5, 0, 3, 1, 0, 0, 0), (20, 12), 25, 3, 5, 'greedy', 'rows', 'none', 0, 0, 0, -1, -1, 'default/policy'),
    ((1, 5, 0, 3, 1, 0, 0, 0), (20, 12), 25, 3, 17, 'tensor', 'rows', 'terminated', 0, 0, 0, -1, -1, 'default/tables'),
    ((1, 5, 0, 3, 1, 0, 0, 0), (6, 16), 23, 33, 17, 'order', 'rows', 'none', 0, 0, 64, -1, -1, 'full/order'),
    ((1, 5, 0, 3, 1, 0, 0, 0), (6, 16), 23, 33, 5, 'greedy', 'rows', 'none', 0, 0, 64, -1, -1, 'full/policy'),
    ((1, 5, 0, 3, 1, 0, 0, 0), (6, 16), 23, 33, 17, 'tensor', 'rows', 'terminated', 0, 0, 64, -1, -1, 'full/tables'),
    ((1, 5, 0, 3, 1, 1, 0, 0), (20, 12), 25, 3, 17, 'tensor', 'rows', 'none', 0, 0, 0, -1, -1, 'default'),
    ((1, 5, 0, 3, 1, 1, 0, 0), (6, 16), 23, 33, 17, 'tensor', 'rows', 'none', 0, 0, 64, -1, -1, 'full'),
    ((1, 5, 1, 0, 0, 0, 0, 0), (100, 100), 18, 3, 5, 'order', 'none', 'none', 0, 0, 0, -1, -1, 'default/order'),
    ((1, 5, 1, 0, 0, 0, 0, 0), (100, 100), 18, 3, 5, 'greedy', 'none', 'none', 0, 0, 0, -1, -1, 'default/policy'),
    ((1, 5, 1, 0, 0, 0, 0, 0), (64, 48), 18, 3, 5, 'tensor', 'none', 'reward', 0, 0, 0, -1, -1, 'default/tables'),
    ((1, 5, 1, 0, 0, 0, 0, 0), (100, 100), 18, 5, 5, 'order', 'none', 'none', 0, 0, 64, -1, -1, 'full/order'),
    ((1, 5, 1, 0, 0, 0, 0, 0), (100, 100), 18, 5, 5, 'greedy', 'none', 'none', 0, 0, 64, -1, -1, 'full/policy'),
    ((1, 5, 1, 0, 0, 0, 0, 0), (100, 100), 18, 5, 5, 'tensor', 'none', 'terminated', 0, 0, 64, -1, -1, 'full/tables'),
    ((1, 5, 1, 0, 0, 0, 0, 0), (6, 16), 18, 3, 5, 'greedy', 'none', 'none', 0, 0, 0, 0, -1, 'occ_forced'),
    ((1, 5, 1, 0, 0, 1, 0, 0), (100, 100), 18, 3, 5, 'tensor', 'none', 'none', 0, 0, 0, -1, -1, 'default'),
    ((1, 5, 1, 0, 0, 1, 0, 0), (100, 100), 18, 5, 5, 'tensor', 'none', 'none', 0, 0, 64, -1, -1, 'full'),
    ((1, 5, 1, 0, 0, 1, 0, 0), (6, 16), 18, 3, 17, 'tensor', 'none', 'none', 0, 0, 0, 0, -1, 'occ_forced'),
    ((1, 5, 1, 0, 1, 0, 0, 0), (6, 16), 18, 3, 17, 'order', 'none', 'none', 0, 0, 0, -1, -1, 'default/order'),
    ((1, 5, 1, 0, 1, 0, 0, 0), (6, 16), 18, 3, 5, 'greedy', 'none', 'none', 0, 0, 0, -1, -1, 'default/policy'),
    ((1, 5, 1, 0, 1, 0, 0, 0), (6, 16), 18, 3, 17, 'tensor', 'none', 'reward', 0, 0, 0, -1, -1, 'default/tables'),
    ((1, 5, 1, 0, 1, 0, 0, 0), (6, 16), 18, 5, 17, 'order', 'none', 'none', 0, 0, 64, -1, -1, 'full/order'),
    ((1, 5, 1, 0, 1, 0, 0, 0), (6, 16), 18, 5, 5, 'greedy', 'none', 'none', 0, 0, 64, -1, -1, 'full/policy'),
    ((1, 5, 1, 0, 1, 0, 0, 0), (6, 16), 18, 5, 17, 'tensor', 'none', 'terminated', 0, 0, 64, -1, -1, 'full/tables'),
    ((1, 5, 1, 0, 1, 1, 0, 0), (6, 16), 18, 3, 17, 'tensor', 'none', 'none', 0, 0, 0, -1, -1, 'default'),
    ((1, 5, 1, 0, 1, 1, 0, 0), (6, 16), 18, 5, 17, 'tensor', 'none', 'none', 0, 0, 64, -1, -1, 'full'),
    ((1, 5, 1, 1, 0, 0, 0, 0), (100, 100), 18, 3, 5, 'order', 'small', 'none', 0, 0, 0, -1, -1, 'default/order'),
    ((1, 5, 1, 1, 0, 0, 0, 0), (100, 100), 18, 3, 5, 'greedy', 'small', 'none', 0, 0, 0, -1, -1, 'default/policy'),
    ((1, 5, 1, 1, 0, 0, 0, 0), (64, 48), 18, 3, 5, 'tensor', 'small', 'reward', 0, 0, 0, -1, -1, 'default/tables'),
    ((1, 5, 1, 1, 0, 0, 0, 0), (100, 100), 18, 5, 5, 'order', 'small', 'none', 0, 0, 64, -1, -1, 'full/order'),
    ((1, 5, 1, 1, 0, 0, 0, 0), (100, 100), 18, 5, 5, 'greedy', 'small', 'none', 0, 0, 64, -1, -1, 'full/policy'),
    ((1, 5, 1, 1, 0, 0, 0, 0), (100, 100), 18, 5, 5, 'tensor', 'small', 'terminated', 0, 0, 64, -1, -1, 'full/tables'),
    ((1, 5, 1, 1, 0, 0, 0, 0), (6, 16), 18, 3, 5, 'greedy', 'small', 'none', 0, 0, 0, 0, -1, 'occ_forced'),
    ((1, 5, 1, 1, 0, 1, 0, 0), (100, 100), 18, 3, 5, 'tensor', 'small', 'none', 0, 0, 0, -1, -1, 'default'),
    ((1, 5, 1, 1, 0, 1, 0, 0), (100, 100), 18, 5, 5, 'tensor', 'small', 'none', 0, 0, 64, -1, -1, 'full'),
    ((1, 5, 1, 1, 0, 1, 0, 0), (6, 16), 18, 3, 17, 'tensor', 'small', 'none', 0, 0, 0, 0, -1, 'occ_forced'),
    ((1, 5, 1, 1, 1, 0, 0, 0), (6, 16), 18, 3, 5, 'greedy_actions_out', 'none', 'none', 0, 0, 0, -1, -1, 'actions_out_only'),
    ((1, 5, 1, 1, 1, 0, 0, 0), (6, 16), 18, 3, 17, 'order', 'small', 'none', 0, 0, 0, -1, -1, 'default/order'),
    ((1, 5, 1, 1, 1, 0, 0, 0), (6, 16), 18, 3, 5, 'greedy', 'small', 'none', 0, 0, 0, -1, -1, 'default/policy'),
    ((1, 5, 1, 1, 1, 0, 0, 0), (6, 16), 18, 3, 17, 'tensor', 'small', 'reward', 0, 0, 0, -1, -1, 'default/tables'),
    ((1, 5, 1, 1, 1, 0, 0, 0), (6, 16), 18, 5, 17, 'order', 'small', 'none', 0, 0, 64, -1, -1, 'full/order'),
    ((1, 5, 1, 1, 1, 0, 0, 0), (6, 16), 18, 5, 5, 'greedy', 'small', 'none', 0, 0, 64, -1, -1, 'full/policy'),
    ((1, 5, 1, 1, 1, 0, 0, 0), (6, 16), 18, 5, 17, 'tensor', 'small', 'terminated', 0, 0, 64, -1, -1, 'full/tables'),
    ((1, 5, 1, 1, 1, 1, 0, 0), (6, 16), 18, 3, 17, 'tensor', 'small', 'none', 0, 0, 0, -1, -1, 'default'),
    ((1, 5, 1, 1, 1, 1, 0, 0), (6, 16), 18, 5, 17, 'tensor', 'small', 'none', 0, 0, 64, -1, -1, 'full'),
    ((1, 5, 1, 2, 0, 0, 0, 0), (100, 100), 18, 3, 5, 'order', 'rows', 'none', 0, 0, 0, -1, -1, 'default/order/off_lines'),
    ((1, 5, 1, 2, 0, 0, 0, 0), (100, 100), 32, 3, 5, 'order', 'rows16', 'none', 0, 0, 0, -1, -1, 'default/order/residue16'),
    ((1, 5, 1, 2, 0, 0, 0, 0), (100, 100), 18, 3, 5, 'greedy', 'rows', 'none', 0, 0, 0, -1, -1, 'default/policy/off_lines'),
    ((1, 5, 1, 2, 0, 0, 0, 0), (100, 100), 32, 3, 5, 'greedy', 'rows16', 'none', 0, 0, 0, -1, -1, 'default/policy/residue16'),
    ((1, 5, 1, 2, 0, 0, 0, 0), (64, 48), 18, 3, 5, 'tensor', 'rows', 'reward', 0, 0, 0, -1, -1, 'default/tables/off_lines'),
    ((1, 5, 1, 2, 0, 0, 0, 0), (64, 48), 32, 3, 5, 'tensor', 'rows16', 'reward', 0, 0, 0, -1, -1, 'default/tables/residue16'),
    ((1, 5, 1, 2, 0, 0, 0, 0), (100, 100), 18, 8, 5, 'order', 'rows', 'none', 0, 0, 64, -1, -1, 'full/order/off_lines'),
    ((1, 5, 1, 2, 0, 0, 0, 0), (100, 100), 32, 5, 5, 'order', 'rows16', 'none', 0, 0, 64, -1, -1, 'full/order/residue16'),
    ((1, 5, 1, 2, 0, 0, 0, 0), (100, 100), 18, 8, 5, 'greedy', 'rows', 'none', 0, 0, 64, -1, -1, 'full/policy/off_lines'),
    ((1, 5, 1, 2, 0, 0, 0, 0), (100, 100), 32, 5, 5, 'greedy', 'rows16', 'none', 0, 0, 64, -1, -1, 'full/policy/residue16'),
    ((1, 5, 1, 2, 0, 0, 0, 0), (100, 100), 18, 8, 5, 'tensor', 'rows', 'terminated', 0, 0, 64, -1, -1, 'full/tables/off_lines'),
    ((1, 5, 1, 2, 0, 0, 0, 0), (100, 100), 32, 5, 5, 'tensor', 'rows16', 'terminated', 0, 0, 64, -1, -1, 'full/tables/residue16'),
    ((1, 5, 1, 2, 0, 0, 0, 0), (6, 16), 18, 3, 5, 'greedy', 'rows', 'none', 0, 0, 0, 0, -1, 'occ_forced'),
    ((1, 5, 1, 2, 0, 1, 0, 0), (100, 100), 18, 3, 5, 'tensor', 'rows', 'none', 0, 0, 0, -1, -1, 'default/off_lines'),
    ((1, 5, 1, 2, 0, 1, 0, 0), (100, 100), 32, 3, 5, 'tensor', 'rows16', 'none', 0, 0, 0, -1, -1, 'default/residue16'),
    ((1, 5, 1, 2, 0, 1, 0, 0), (100, 100), 18, 8, 5, 'tensor', 'rows', 'none', 0, 0, 64, -1, -1, 'full/off_lines'),
    ((1, 5, 1, 2, 0, 1, 0, 0), (100, 100), 32, 5, 5, 'tensor', 'rows16', 'none', 0, 0, 64, -1, -1, 'full/residue16'),
    ((1, 5, 1, 2, 0, 1, 0, 0), (6, 16), 18, 3, 17, 'tensor', 'rows', 'none', 0, 0, 0, 0, -1, 'occ_forced'),
    ((1, 5, 1, 2, 1, 0, 0, 0), (6, 16), 18, 3, 5, 'greedy_actions_out', 'rows', 'none', 0, 0, 0, -1, -1, 'actions_out'),
    ((1, 5, 1, 2, 1, 0, 0, 0), (6, 16), 18, 3, 17, 'order', 'rows', 'none', 0, 0, 0, -1, -1, 'default/order/off_lines'),
    ((1, 5, 1, 2, 1, 0, 0, 0), (20, 12), 32, 3, 17, 'order', 'rows16', 'none', 0, 0, 0, -1, -1, 'default/order/residue16'),
    ((1, 5, 1, 2, 1, 0, 0, 0), (6, 16), 18, 3, 5, 'greedy', 'rows', 'none', 0, 0, 0, -1, -1, 'default/policy/off_lines'),
    ((1, 5, 1, 2, 1, 0, 0, 0), (20, 12), 32, 3, 5, 'greedy', 'rows16', 'none', 0, 0, 0, -1, -1, 'default/policy/residue16'),
    ((1, 5, 1, 2, 1, 0, 0, 0), (6, 16), 18, 3, 17, 'tensor', 'rows', 'reward', 0, 0, 0, -1, -1, 'default/tables/off_lines'),
    ((1, 5, 1, 2, 1, 0, 0, 0), (20, 12), 32, 3, 17, 'tensor', 'rows16', 'reward', 0, 0, 0, -1, -1, 'default/tables/residue16'),
    ((1, 5, 1, 2, 1, 0, 0, 0), (6, 16), 18, 8, 17, 'order', 'rows', 'none', 0, 0, 64, -1, -1, 'full/order/off_lines'),
    ((1, 5, 1, 2, 1, 0, 0, 0), (20, 12), 32, 5, 17, 'order', 'rows16', 'none', 0, 0, 64, -1, -1, 'full/order/residue16'),
    ((1, 5, 1, 2, 1, 0, 0, 0), (6, 16), 18, 8, 5, 'greedy', 'rows', 'none', 0, 0, 64, -1, -1, 'full/policy/off_lines'),
    ((1, 5, 1, 2, 1, 0, 0, 0), (20, 12), 32, 5, 5, 'greedy', 'rows16', 'none', 0, 0, 64, -1, -1, 'full/policy/residue16'),
    ((1, 5, 1, 2, 1, 0, 0, 0), (6, 16), 18, 8, 17, 'tensor', 'rows', 'terminated', 0, 0, 64, -1, -1, 'full/tables/off_lines'),
    ((1, 5, 1, 2, 1, 0, 0, 0), (20, 12), 32, 5, 17, 'tensor', 'rows16', 'terminated', 0, 0, 64, -1, -1, 'full/tables/residue16'),
    ((1, 5, 1, 2, 1, 1, 0, 0), (6, 16), 18, 3, 17, 'tensor', 'rows', 'none', 0, 0, 0, -1, -1, 'default/off_lines'),
    ((1, 5, 1, 2, 1, 1, 0, 0), (20, 12), 32, 3, 17, 'tensor', 'rows16', 'none', 0, 0, 0, -1, -1, 'default/residue16'),
    ((1, 5, 1, 2, 1, 1, 0, 0), (6, 16), 18, 8, 17, 'tensor', 'rows', 'none', 0, 0, 64, -1, -1, 'full/off_lines'),
    ((1, 5, 1, 2, 1, 1, 0, 0), (20, 12), 32, 5, 17, 'tensor', 'rows16', 'none', 0, 0, 64, -1, -1, 'full/residue16'),
    ((1, 5, 1, 3, 0, 0, 0, 0), (100, 100), 18, 5, 5, 'order', 'rows', 'none', 0, 0, 64, -1, -1, 'full/order'),
    ((1, 5, 1, 3, 0, 0, 0, 0), (100, 100), 18, 5, 5, 'greedy', 'rows', 'none', 0, 0, 64, -1, -1, 'full/policy'),
    ((1, 5, 1, 3, 0, 0, 0, 0), (100, 100), 18, 5, 5, 'tensor', 'rows', 'terminated', 0, 0, 64, -1, -1, 'full/tables'),
    ((1, 5, 1, 3, 0, 0, 0, 0), (20, 12), 26, 3, 5, 'greedy', 'rows', 'none', 0, 0, 0, 0, -1, 'occ_forced'),
    ((1, 5, 1, 3, 0, 1, 0, 0), (100, 100), 18, 5, 5, 'tensor', 'rows', 'none', 0, 0, 64, -1, -1, 'full'),
    ((1, 5, 1, 3, 0, 1, 0, 0), (20, 12), 26, 3, 17, 'tensor', 'rows', 'none', 0, 0, 0, 0, -1, 'occ_forced'),
    ((1, 5, 1, 3, 1, 0, 0, 0), (6, 16), 18, 5, 17, 'order', 'rows', 'none', 0, 0, 64, -1, -1, 'full/order'),
    ((1, 5, 1, 3, 1, 0, 0, 0), (6, 16), 18, 5, 5, 'greedy', 'rows', 'none', 0, 0, 64, -1, -1, 'full/policy'),
    ((1, 5, 1, 3, 1, 0, 0, 0), (6, 16), 18, 5, 17, 'tensor', 'rows', 'terminated', 0, 0, 64, -1, -1, 'full/tables'),
    ((1, 5, 1, 3, 1, 1, 0, 0), (6, 16), 18, 5, 17, 'tensor', 'rows', 'none', 0, 0, 64, -1, -1, 'full'),
    ((1, 6, 0, 0, 0, 0, 0, 0), (64, 48), 49, 3, 17, 'order', 'none', 'none', 0, 0, 0, -1, -1, 'default/order'),
    ((1, 6, 0, 0, 0, 0, 0, 0), (64, 48), 49, 3, 5, 'greedy', 'none', 'none', 0, 0, 0, -1, -1, 'default/policy'),
    ((1, 6, 0, 0, 0, 0, 0, 0), (64, 48), 33, 3, 5, 'tensor', 'none', 'reward', 0, 0, 0, -1, -1, 'default/tables'),
    ((1, 6, 0, 0, 0, 0, 0, 0), (64, 48), 49, 3, 17, 'order', 'none', 'none', 0, 0, 64, -1, -1, 'full/order'),
    ((1, 6, 0, 0, 0, 0, 0, 0), (64, 48), 49, 3, 5, 'greedy', 'none', 'none', 0, 0, 64, -1, -1, 'full/policy'),
    ((1, 6, 0, 0, 0, 0, 0, 0), (64, 48), 49, 3, 17, 'tensor', 'none', 'terminated', 0, 0, 64, -1, -1, 'full/tables'),
    ((1, 6, 0, 0, 0, 0, 0, 0), (20, 12), 33, 3, 5, 'greedy', 'none', 'none', 0, 0, 0, 0, -1, 'occ_forced'),
    ((1, 6, 0, 0, 0, 1, 0, 0), (64, 48), 49, 3, 17, 'tensor', 'none', 'none', 0, 0, 0, -1, -1, 'default'),
    ((1, 6, 0, 0, 0, 1, 0, 0), (64, 48), 49, 3, 17, 'tensor', 'none', 'none', 0, 0, 64, -1, -1, 'full'),
    ((1, 6, 0, 0, 0, 1, 0, 0), (20, 12), 33, 3, 17, 'tensor', 'none', 'none', 0, 0, 0, 0, -1, 'occ_forced'),
    ((1, 6, 0, 0, 1, 0, 0, 0), (20, 12), 33, 3, 17, 'order', 'none', 'none', 0, 0, 0, -1, -1, 'default/order'),
    ((1, 6, 0, 0, 1, 0, 0, 0), (20, 12), 33, 3, 5, 'greedy', 'none', 'none', 0, 0, 0, -1, -1, 'default/policy'),
    ((1, 6, 0, 0, 1, 0, 0, 0), (20, 12), 33, 3, 17, 'tensor', 'none', 'reward', 0, 0, 0, -1, -1, 'default/tables'),
    ((1, 6, 0, 0, 1, 0, 0, 0), (20, 12), 33, 3, 17, 'order', 'none', 'none', 0, 0, 64, -1, -1, 'full/order'),
    ((1, 6, 0, 0, 1, 0, 0, 0), (20, 12), 33, 3, 5, 'greedy', 'none', 'none', 0, 0, 64, -1, -1, 'full/policy'),
    ((1, 6, 0, 0, 1, 0, 0, 0), (20, 12), 33, 3, 17, 'tensor', 'none', 'terminated', 0, 0, 64, -1, -1, 'full/tables'),
    ((1, 6, 0, 0, 1, 1, 0, 0), (20, 12), 33, 3, 17, 'tensor', 'none', 'none', 0, 0, 0, -1, -1, 'default'),
    ((1, 6, 0, 0, 1, 1, 0, 0), (20, 12), 33, 3, 17, 'tensor', 'none', 'none', 0, 0, 64, -1, -1, 'full'),
    ((1, 6, 0, 1, 0, 0, 0, 0), (64, 48), 49, 3, 17, 'order', 'small', 'none', 0, 0, 0, -1, -1, 'default/order'),
    ((1, 6, 0, 1, 0, 0, 0, 0), (64, 48), 49, 3, 5, 'greedy', 'small', 'none', 0, 0, 0, -1, -1, 'default/policy'),
    ((1, 6, 0, 1, 0, 0, 0, 0), (64, 48), 33, 3, 5, 'tensor', 'small', 'reward', 0, 0, 0, -1, -1, 'default/tables'),
    ((1, 6, 0, 1, 0, 0, 0, 0), (64, 48), 49, 3, 17, 'order', 'small', 'none', 0, 0, 64, -1, -1, 'full/order'),
    ((1, 6, 0, 1, 0, 0, 0, 0), (64, 48), 49, 3, 5, 'greedy', 'small', 'none', 0, 0, 64, -1, -1, 'full/policy'),
    ((1, 6, 0, 1, 0, 0, 0, 0), (64, 48), 49, 3, 17, 'tensor', 'small', 'terminated', 0, 0, 64, -1, -1, 'full/tables'),
    ((1, 6, 0, 1, 0, 0, 0, 0), (20, 12), 33, 3, 5, 'greedy', 'small', 'none', 0, 0, 0, 0, -1, 'occ_forced'),
    ((1, 6, 0, 1, 0, 1, 0, 0), (64, 48), 49, 3, 17, 'tensor', 'small', 'none', 0, 0, 0, -1, -1, 'default'),
    ((1, 6, 0, 1, 0, 1, 0, 0), (64, 48), 49, 3, 17, 'tensor', 'small', 'none', 0, 0, 64, -1, -1, 'full'),
    ((1, 6, 0, 1, 0, 1, 0, 0), (20, 12), 33, 3, 17, 'tensor', 'small', 'none', 0, 0, 0, 0, -1, 'occ_forced'),
    ((1, 6, 0, 1, 1, 0, 0, 0), (20, 12), 33, 3, 5, 'greedy_actions_out', 'none', 'none', 0, 0, 0, -1, -1, 'actions_out_only'),
    ((1, 6, 0, 1, 1, 0, 0, 0), (20, 12), 33, 3, 17, 'order', 'small', 'none', 0, 0, 0, -1, -1, 'default/order'),
    ((1, 6, 0, 1, 1, 0, 0, 0), (20, 12), 33, 3, 5, 'greedy', 'small', 'none', 0, 0, 0, -1, -1, 'default/policy'),
    ((1, 6, 0, 1, 1, 0, 0, 0), (20, 12), 33, 3, 17, 'tensor', 'small', 'reward', 0, 0, 0, -1, -1, 'default/tables'),
    ((1, 6, 0, 1, 1, 0, 0, 0), (20, 12), 33, 3, 17, 'order', 'small', 'none', 0, 0, 64, -1, -1, 'full/order'),
    ((1, 6, 0, 1, 1, 0, 0, 0), (20, 12), 33, 3, 5, 'greedy', 'small', 'none', 0, 0, 64, -1, -1, 'full/policy'),
    ((1, 6, 0, 1, 1, 0, 0, 0), (20, 12), 33, 3, 17, 'tensor', 'small', 'terminated', 0, 0, 64, -1, -1, 'full/tables'),
    ((1, 6, 0, 1, 1, 1, 0, 0), (20, 12), 33, 3, 17, 'tensor', 'small', 'none', 0, 0, 0, -1, -1, 'default'),
    ((1, 6, 0, 1, 1, 1, 0, 0), (20, 12), 33, 3, 17, 'tensor', 'small', 'none', 0, 0, 64, -1, -1, 'full'),
    ((1, 6, 0, 2, 0, 0, 0, 0), (64, 48), 49, 16, 17, 'order', 'rows', 'none', 0, 0, 0, -1, -1, 'default/order/off_lines'),
    ((1, 6, 0, 2, 0, 0, 0, 0), (64, 48), 49, 16, 5, 'greedy', 'rows', 'none', 0, 0, 0, -1, -1, 'default/policy/off_lines'),
    ((1, 6, 0, 2, 0, 0, 0, 0), (64, 48), 33, 16, 5, 'tensor', 'rows', 'reward', 0, 0, 0, -1, -1, 'default/tables/off_lines'),
    ((1, 6, 0, 2, 0, 0, 0, 0), (64, 48), 49, 16, 17, 'order', 'rows', 'none', 0, 0, 64, -1, -1, 'full/order/off_lines'),
    ((1, 6, 0, 2, 0, 0, 0, 0), (64, 48), 49, 16, 5, 'greedy', 'rows', 'none', 0, 0, 64, -1, -1, 'full/policy/off_lines'),
    ((1, 6, 0, 2, 0, 0, 0, 0), (64, 48), 49, 16, 17, 'tensor', 'rows', 'terminated', 0, 0, 64, -1, -1, 'full/tables/off_lines'),
    ((1, 6, 0, 2, 0, 0, 0, 0), (20, 12), 33, 16, 5, 'greedy', 'rows', 'none', 0, 0, 0, 0, -1, 'occ_forced'),
    ((1, 6, 0, 2, 0, 1, 0, 0), (64, 48), 49, 16, 17, 'tensor', 'rows', 'none', 0, 0, 0, -1, -1, 'default/off_lines'),
    ((1, 6, 0, 2, 0, 1, 0, 0), (64, 48), 49, 16, 17, 'tensor', 'rows', 'none', 0, 0, 64, -1, -1, 'full/off_lines'),
    ((1, 6, 0, 2, 0, 1, 0, 0), (20, 12), 33, 16, 17, 'tensor', 'rows', 'none', 0, 0, 0, 0, -1, 'occ_forced'),
    ((1, 6, 0, 2, 1, 0, 0, 0), (20, 12), 33, 16, 17, 'order', 'rows', 'none', 0, 0, 0, -1, -1, 'default/order/off_lines'),
    ((1, 6, 0, 2, 1, 0, 0, 0), (20, 12), 33, 16, 5, 'greedy', 'rows', 'none', 0, 0, 0, -1, -1, 'default/policy/off_lines'),
    ((1, 6, 0, 2, 1, 0, 0, 0), (20, 12), 33, 16, 17, 'tensor', 'rows', 'reward', 0, 0, 0, -1, -1, 'default/tables/off_lines'),
    ((1, 6, 0, 2, 1, 0, 0, 0), (20, 12), 33, 16, 17, 'order', 'rows', 'none', 0, 0, 64, -1, -1, 'full/order/off_lines'),
    ((1, 6, 0, 2, 1, 0, 0, 0), (20, 12), 33, 16, 5, 'greedy', 'rows', 'none', 0, 0, 64, -1, -1, 'full/policy/off_lines'),
    ((1, 6, 0, 2, 1, 0, 0, 0), (20, 12), 33, 16, 17, 'tensor', 'rows', 'terminated', 0, 0, 64, -1, -1, 'full/tables/off_lines'),
    ((1, 6, 0, 2, 1, 1, 0, 0), (20, 12), 33, 16, 17, 'tensor', 'rows', 'none', 0, 0, 0, -1, -1, 'default/off_lines'),
    ((1, 6, 0, 2, 1, 1, 0, 0), (20, 12), 33, 16, 17, 'tensor', 'rows', 'none', 0, 0, 64, -1, -1, 'full/off_lines'),
    ((1, 6, 0, 3, 0, 0, 0, 0), (64, 48), 49, 3, 17, 'order', 'rows', 'none', 0, 0, 0, -1, -1, 'default/order'),
    ((1, 6, 0, 3, 0, 0, 0, 0), (64, 48), 49, 3, 5, 'greedy', 'rows', 'none', 0, 0, 0, -1, -1, 'default/policy'),
    ((1, 6, 0, 3, 0, 0, 0, 0), (64, 48), 33, 3, 5, 'tensor', 'rows', 'reward', 0, 0, 0, -1, -1, 'default/tables'),
    ((1, 6, 0, 3, 0, 0, 0, 0), (64, 48), 49, 3, 17, 'order', 'rows', 'none', 0, 0, 64, -1, -1, 'full/order'),
    ((1, 6, 0, 3, 0, 0, 0, 0), (64, 48), 49, 3, 5, 'greedy', 'rows', 'none', 0, 0, 64, -1, -1, 'full/policy'),
    ((1, 6, 0, 3, 0, 0, 0, 0), (64, 48), 49, 3, 17, 'tensor', 'rows', 'terminated', 0, 0, 64, -1, -1, 'full/tables'),
    ((1, 6, 0, 3, 0, 0, 0, 0), (20, 12), 33, 3, 5, 'greedy', 'rows', 'none', 0, 0, 0, 0, -1, 'occ_forced'),
    ((1, 6, 0, 3, 0, 1, 0, 0), (64, 48), 49, 3, 17, 'tensor', 'rows', 'none', 0, 0, 0, -1, -1, 'default'),
    ((1, 6, 0, 3, 0, 1, 0, 0), (64, 48), 49, 3, 17, 'tensor', 'rows', 'none', 0, 0, 64, -1, -1, 'full'),
    ((1, 6, 0, 3, 0, 1, 0, 0), (20, 12), 33, 3, 17, 'tensor', 'rows', 'none', 0, 0, 0, 0, -1, 'occ_forced'),
    ((1, 6, 0, 3, 1, 0, 0, 0), (20, 12), 33, 3, 5, 'greedy_actions_out', 'rows', 'none', 0, 0, 0, -1, -1, 'actions_out'),
    ((1, 6, 0, 3, 1, 0, 0, 0), (20, 12), 33, 3, 17, 'order', 'rows', 'none', 0, 0, 0, -1, -1, 'default/order'),
    ((1, 6, 0, 3, 1, 0, 0, 0), (20, 12), 33, 3, 5, 'greedy', 'rows', 'none', 0, 0, 0, -1, -1, 'default/policy'),
    ((1, 6, 0, 3, 1, 0, 0, 0), (20, 12), 33, 3, 17, 'tensor', 'rows', 'reward', 0, 0, 0, -1, -1, 'default/tables'),
    ((1, 6, 0, 3, 1, 0, 0, 0), (20, 12), 33, 3, 17, 'order', 'rows', 'none', 0, 0, 64, -1, -1, 'full/order'),
    ((1, 6, 0, 3, 1, 0, 0, 0), (20, 12), 33, 3, 5, 'greedy', 'rows', 'none', 0, 0, 64, -1, -1, 'full/policy'),
    ((1, 6, 0, 3, 1, 0, 0, 0), (20, 12), 33, 3, 17, 'tensor', 'rows', 'terminated', 0, 0, 64, -1, -1, 'full/tables'),
    ((1, 6, 0, 3, 1, 1, 0, 0), (20, 12), 33, 3, 17, 'tensor', 'rows', 'none', 0, 0, 0, -1, -1, 'default'),
    ((1, 6, 0, 3, 1, 1, 0, 0), (20, 12), 33, 3, 17, 'tensor', 'rows', 'none', 0, 0, 64, -1, -1, 'full'),
    ((1, 6, 1, 0, 0, 0, 0, 0), (64, 48), 50, 3, 17, 'order', 'none', 'none', 0, 0, 0, -1, -1, 'default/order'),
    ((1, 6, 1, 0, 0, 0, 0, 0), (64, 48), 50, 3, 5, 'greedy', 'none', 'none', 0, 0, 0, -1, -1, 'default/policy'),
    ((1, 6, 1, 0, 0, 0, 0, 0), (64, 48), 34, 3, 5, 'tensor', 'none', 'reward', 0, 0, 0, -1, -1, 'default/tables'),
    ((1, 6, 1, 0, 0, 0, 0, 0), (64, 48), 50, 3, 17, 'order', 'none', 'none', 0, 0, 64, -1, -1, 'full/order'),
    ((1, 6, 1, 0, 0, 0, 0, 0), (64, 48), 50, 3, 5, 'greedy', 'none', 'none', 0, 0, 64, -1, -1, 'full/policy'),
    ((1, 6, 1, 0, 0, 0, 0, 0), (64, 48), 50, 3, 17, 'tensor', 'none', 'terminated', 0, 0, 64, -1, -1, 'full/tables'),
    ((1, 6, 1, 0, 0, 0, 0, 0), (20, 12), 34, 3, 5, 'greedy', 'none', 'none', 0, 0, 0, 0, -1, 'occ_forced'),
    ((1, 6, 1, 0, 0, 1, 0, 0), (64, 48), 50, 3, 17, 'tensor', 'none', 'none', 0, 0, 0, -1, -1, 'default'),
    ((1, 6, 1, 0, 0, 1, 0, 0), (64, 48), 50, 3, 17, 'tensor', 'none', 'none', 0, 0, 64, -1, -1, 'full'),
    ((1, 6, 1, 0, 0, 1, 0, 0), (20, 12), 34, 3, 17, 'tensor', 'none', 'none', 0, 0, 0, 0, -1, 'occ_forced'),
    ((1, 6, 1, 0, 1, 0, 0, 0), (20, 12), 34, 3, 17, 'order', 'none', 'none', 0, 0, 0, -1, -1, 'default/order'),
    ((1, 6, 1, 0, 1, 0, 0, 0), (20, 12), 34, 3, 5, 'greedy', 'none', 'none', 0, 0, 0, -1, -1, 'default/policy'),
    ((1, 6, 1, 0, 1, 0, 0, 0), (20, 12), 34, 3, 17, 'tensor', 'none', 'reward', 0, 0, 0, -1, -1, 'default/tables'),
    ((1, 6, 1, 0, 1, 0, 0, 0), (20, 12), 34, 3, 17, 'order', 'none', 'none', 0, 0, 64, -1, -1, 'full/order'),
    ((1, 6, 1, 0, 1, 0, 0, 0), (20, 12), 34, 3, 5, 'greedy', 'none', 'none', 0, 0, 64, -1, -1, 'full/policy'),
    ((1, 6, 1, 0, 1, 0, 0, 0), (20, 12), 34, 3, 17, 'tensor', 'none', 'terminated', 0, 0, 64, -1, -1, 'full/tables'),
    ((1, 6, 1, 0, 1, 1, 0, 0), (20, 12), 34, 3, 17, 'tensor', 'none', 'none', 0, 0, 0, -1, -1, 'default'),
    ((1, 6, 1, 0, 1, 1, 0, 0), (20, 12), 34, 3, 17, 'tensor', 'none', 'none', 0, 0, 64, -1, -1, 'full'),
    ((1, 6, 1, 1, 0, 0, 0, 0), (64, 48), 50, 3, 17, 'order', 'small', 'none', 0, 0, 0, -1, -1, 'default/order'),
    ((1, 6, 1, 1, 0, 0, 0, 0), (64, 48), 50, 3, 5, 'greedy', 'small', 'none', 0, 0, 0, -1, -1, 'default/policy'),
    ((1, 6, 1, 1, 0, 0, 0, 0), (64, 48), 34, 3, 5, 'tensor', 'small', 'reward', 0, 0, 0, -1, -1, 'default/tables'),
    ((1, 6, 1, 1, 0, 0, 0, 0), (64, 48), 50, 3, 17, 'order', 'small', 'none', 0, 0, 64, -1, -1, 'full/order'),
    ((1, 6, 1, 1, 0, 0, 0, 0), (64, 48), 50, 3, 5, 'greedy', 'small', 'none', 0, 0, 64, -1, -1, 'full/policy'),
    ((1, 6, 1, 1, 0, 0, 0, 0), (64, 48), 50, 3, 17, 'tensor', 'small', 'terminated', 0, 0, 64, -1, -1, 'full/tables'),
    ((1, 6, 1, 1, 0, 0, 0, 0), (20, 12), 34, 3, 5, 'greedy', 'small', 'none', 0, 0, 0, 0, -1, 'occ_forced'),
    ((1, 6, 1, 1, 0, 1, 0, 0), (64, 48), 50, 3, 17, 'tensor', 'small', 'none', 0, 0, 0, -1, -1, 'default'),
    ((1, 6, 1, 1, 0, 1, 0, 0), (64, 48), 50, 3, 17, 'tensor', 'small', 'none', 0, 0, 64, -1, -1, 'full'),
    ((1, 6, 1, 1, 0, 1, 0, 0), (20, 12), 34, 3, 17, 'tensor', 'small', 'none', 0, 0, 0, 0, -1, 'occ_forced'),
    ((1, 6, 1, 1, 1, 0, 0, 0), (20, 12), 34, 3, 5, 'greedy_actions_out', 'none', 'none', 0, 0, 0, -1, -1, 'actions_out_only'),
    ((1, 6, 1, 1, 1, 0, 0, 0), (20, 12), 34, 3, 17, 'order', 'small', 'none', 0, 0, 0, -1, -1, 'default/order'),
    ((1, 6, 1, 1, 1, 0, 0, 0), (20, 12), 34, 3, 5, 'greedy', 'small', 'none', 0, 0, 0, -1, -1, 'default/policy'),
    ((1, 6, 1, 1, 1, 0, 0, 0), (20, 12), 34, 3, 17, 'tensor', 'small', 'reward', 0, 0, 0, -1, -1, 'default/tables'),
    ((1, 6, 1, 1, 1, 0, 0, 0), (20, 12), 34, 3, 17, 'order', 'small', 'none', 0, 0, 64, -1, -1, 'full/order'),
    ((1, 6, 1, 1, 1, 0, 0, 0), (20, 12), 34, 3, 5, 'greedy', 'small', 'none', 0, 0, 64, -1, -1, 'full/policy'),
    ((1, 6, 1, 1, 1, 0, 0, 0), (20, 12), 34, 3, 17, 'tensor', 'small', 'terminated', 0, 0, 64, -1, -1, 'full/tables'),
    ((1, 6, 1, 1, 1, 1, 0, 0), (20, 12), 34, 3, 17, 'tensor', 'small', 'none', 0, 0, 0, -1, -1, 'default'),
    ((1, 6, 1, 1, 1, 1, 0, 0), (20, 12), 34, 3, 17, 'tensor', 'small', 'none', 0, 0, 64, -1, -1, 'full'),
    ((1, 6, 1, 2, 0, 0, 0, 0), (64, 48), 50, 8, 17, 'order', 'rows', 'none', 0, 0, 0, -1, -1, 'default/order/off_lines'),
    ((1, 6, 1, 2, 0, 0, 0, 0), (64, 48), 64, 3, 17, 'order', 'rows16', 'none', 0, 0, 0, -1, -1, 'default/order/residue16'),
    ((1, 6, 1, 2, 0, 0, 0, 0), (64, 48), 50, 8, 5, 'greedy', 'rows', 'none', 0, 0, 0, -1, -1, 'default/policy/off_lines'),
    ((1, 6, 1, 2, 0, 0, 0, 0), (64, 48), 64, 3, 5, 'greedy', 'rows16', 'none', 0, 0, 0, -1, -1, 'default/policy/residue16'),
    ((1, 6, 1, 2, 0, 0, 0, 0), (64, 48), 34, 3, 5, 'tensor', 'rows', 'reward', 0, 0, 0, -1, -1, 'default/tables/off_lines'),
    ((1, 6, 1, 2, 0, 0, 0, 0), (64, 48), 64, 3, 5, 'tensor', 'rows16', 'reward', 0, 0, 0, -1, -1, 'default/tables/residue16'),
    ((1, 6, 1, 2, 0, 0, 0, 0), (64, 48), 50, 8, 17, 'order', 'rows', 'none', 0, 0, 64, -1, -1, 'full/order/off_lines'),
    ((1, 6, 1, 2, 0, 0, 0, 0), (64, 48), 64, 3, 17, 'order', 'rows16', 'none', 0, 0, 64, -1, -1, 'full/order/residue16'),
    ((1, 6, 1, 2, 0, 0, 0, 0), (64, 48), 50, 8, 5, 'greedy', 'rows', 'none', 0, 0, 64, -1, -1, 'full/policy/off_lines'),
    ((1, 6, 1, 2, 0, 0, 0, 0), (64, 48), 64, 3, 5, 'greedy', 'rows16', 'none', 0, 0, 64, -1, -1, 'full/policy/residue16'),
    ((1, 6, 1, 2, 0, 0, 0, 0), (64, 48), 50, 8, 17, 'tensor', 'rows', 'terminated', 0, 0, 64, -1, -1, 'full/tables/off_lines'),
    ((1, 6, 1, 2, 0, 0, 0, 0), (64, 48), 64, 3, 17, 'tensor', 'rows16', 'terminated', 0, 0, 64, -1, -1, 'full/tables/residue16'),
    ((1, 6, 1, 2, 0, 0, 0, 0), (20, 12), 34, 3, 5, 'greedy', 'rows', 'none', 0, 0, 0, 0, -1, 'occ_forced'),
    ((1, 6, 1, 2, 0, 1, 0, 0), (64, 48), 50, 8, 17, 'tensor', 'rows', 'none', 0, 0, 0, -1, -1, 'default/off_lines'),
    ((1, 6, 1, 2, 0, 1, 0, 0), (64, 48), 64, 3, 17, 'tensor', 'rows16', 'none', 0, 0, 0, -1, -1, 'default/residue16'),
    ((1, 6, 1, 2, 0, 1, 0, 0), (64, 48), 50, 8, 17, 'tensor', 'rows', 'none', 0, 0, 64, -1, -1, 'full/off_lines'),
    ((1, 6, 1, 2, 0, 1, 0, 0), (64, 48), 64, 3, 17, 'tensor', 'rows16', 'none', 0, 0, 64, -1, -1, 'full/residue16'),
    ((1, 6, 1, 2, 0, 1, 0, 0), (20, 12), 34, 3, 17, 'tensor', 'rows', 'none', 0, 0, 0, 0, -1, 'occ_forced'),
    ((1, 6, 1, 2, 1, 0, 0, 0), (20, 12), 34, 3, 5, 'greedy_actions_out', 'rows', 'none', 0, 0, 0, -1, -1, 'actions_out'),
    ((1, 6, 1, 2, 1, 0, 0, 0), (20, 12), 34, 3, 17, 'order', 'rows', 'none', 0, 0, 0, -1, -1, 'default/order/off_lines'),
    ((1, 6, 1, 2, 1, 0, 0, 0), (32, 16), 64, 3, 17, 'order', 'rows16', 'none', 0, 0, 0, -1, -1, 'default/order/residue16'),
    ((1, 6, 1, 2, 1, 0, 0, 0), (20, 12), 34, 3, 5, 'greedy', 'rows', 'none', 0, 0, 0, -1, -1, 'default/policy/off_lines'),
    ((1, 6, 1, 2, 1, 0, 0, 0), (32, 16), 64, 3, 5, 'greedy', 'rows16', 'none', 0, 0, 0, -1, -1, 'default/policy/residue16'),
    ((1, 6, 1, 2, 1, 0, 0, 0), (20, 12), 34, 3, 17, 'tensor', 'rows', 'reward', 0, 0, 0, -1, -1, 'default/tables/off_lines'),
    ((1, 6, 1, 2, 1, 0, 0, 0), (32, 16), 64, 3, 17, 'tensor', 'rows16', 'reward', 0, 0, 0, -1, -1, 'default/tables/residue16'),
    ((1, 6, 1, 2, 1, 0, 0, 0), (20, 12), 34, 3, 17, 'order', 'rows', 'none', 0, 0, 64, -1, -1, 'full/order/off_lines'),
    ((1, 6, 1, 2, 1, 0, 0, 0), (32, 16), 64, 3, 17, 'order', 'rows16', 'none', 0, 0, 64, -1, -1, 'full/order/residue16'),
    ((1, 6, 1, 2, 1, 0, 0, 0), (20, 12), 34, 3, 5, 'greedy', 'rows', 'none', 0, 0, 64, -1, -1, 'full/policy/off_lines'),
    ((1, 6, 1, 2, 1, 0, 0, 0), (32, 16), 64, 3, 5, 'greedy', 'rows16', 'none', 0, 0, 64, -1, -1, 'full/policy/residue16'),
    ((1, 6, 1, 2, 1, 0, 0, 0), (20, 12), 34, 3, 17, 'tensor', 'rows', 'terminated', 0, 0, 64, -1, -1, 'full/tables/off_lines'),
    ((1, 6, 1, 2, 1, 0, 0, 0), (32, 16), 64, 3, 17, 'tensor', 'rows16', 'terminated', 0, 0, 64, -1, -1, 'full/tables/residue16'),
    ((1, 6, 1, 2, 1, 1, 0, 0), (20, 12), 34, 3, 17, 'tensor', 'rows', 'none', 0, 0, 0, -1, -1, 'default/off_lines'),
    ((1, 6, 1, 2, 1, 1, 0, 0), (32, 16), 64, 3, 17, 'tensor', 'rows16', 'none', 0, 0, 0, -1, -1, 'default/residue16'),
    ((1, 6, 1, 2, 1, 1, 0, 0), (20, 12), 34, 3, 17, 'tensor', 'rows', 'none', 0, 0, 64, -1, -1, 'full/off_lines'),
    ((1, 6, 1, 2, 1, 1, 0, 0), (32, 16), 64, 3, 17, 'tensor', 'rows16', 'none', 0, 0, 64, -1, -1, 'full/residue16'),
    ((1, 6, 1, 3, 0, 0, 0, 0), (64, 48), 50, 3, 17, 'order', 'rows', 'none', 0, 0, 0, -1, -1, 'default/order'),
    ((1, 6, 1, 3, 0, 0, 0, 0), (64, 48), 50, 3, 5, 'greedy', 'rows', 'none', 0, 0, 0, -1, -1, 'default/policy'),
    ((1, 6, 1, 3, 0, 0, 0, 0), (64, 48), 50, 3, 5, 'tensor', 'rows', 'reward', 0, 0, 0, -1, -1, 'default/tables'),
    ((1, 6, 1, 3, 0, 0, 0, 0), (64, 48), 50, 3, 17, 'order', 'rows', 'none', 0, 0, 64, -1, -1, 'full/order'),
    ((1, 6, 1, 3, 0, 0, 0, 0), (64, 48), 50, 3, 5, 'greedy', 'rows', 'none', 0, 0, 64, -1, -1, 'full/policy'),
    ((1, 6, 1, 3, 0, 0, 0, 0), (64, 48), 50, 3, 17, 'tensor', 'rows', 'terminated', 0, 0, 64, -1, -1, 'full/tables'),
    ((1, 6, 1, 3, 0, 0, 0, 0), (20, 12), 36, 3, 5, 'greedy', 'rows', 'none', 0, 0, 0, 0, -1, 'occ_forced'),
    ((1, 6, 1, 3, 0, 1, 0, 0), (64, 48), 50, 3, 17, 'tensor', 'rows', 'none', 0, 0, 0, -1, -1, 'default'),
    ((1, 6, 1, 3, 0, 1, 0, 0), (64, 48), 50, 3, 17, 'tensor', 'rows', 'none', 0, 0, 64, -1, -1, 'full'),
    ((1, 6, 1, 3, 0, 1, 0, 0), (20, 12), 36, 3, 17, 'tensor', 'rows', 'none', 0, 0, 0, 0, -1, 'occ_forced'),
    ((1, 6, 1, 3, 1, 0, 0, 0), (20, 12), 50, 3, 17, 'order', 'rows', 'none', 0, 0, 0, -1, -1, 'default/order'),
    ((1, 6, 1, 3, 1, 0, 0, 0), (20, 12), 50, 3, 5, 'greedy', 'rows', 'none', 0, 0, 0, -1, -1, 'default/policy'),
    ((1, 6, 1, 3, 1, 0, 0, 0), (20, 12), 50, 3, 17, 'tensor', 'rows', 'reward', 0, 0, 0, -1, -1, 'default/tables'),
    ((1, 6, 1, 3, 1, 0, 0, 0), (20, 12), 50, 3, 17, 'order', 'rows', 'none', 0, 0, 64, -1, -1, 'full/order'),
    ((1, 6, 1, 3, 1, 0, 0, 0), (20, 12), 50, 3, 5, 'greedy', 'rows', 'none', 0, 0, 64, -1, -1, 'full/policy'),
    ((1, 6, 1, 3, 1, 0, 0, 0), (20, 12), 50, 3, 17, 'tensor', 'rows', 'terminated', 0, 0, 64, -1, -1, 'full/tables'),
    ((1, 6, 1, 3, 1, 1, 0, 0), (20, 12), 50, 3, 17, 'tensor', 'rows', 'none', 0, 0, 0, -1, -1, 'default'),
    ((1, 6, 1, 3, 1, 1, 0, 0), (20, 12), 50, 3, 17, 'tensor', 'rows', 'none', 0, 0, 64, -1, -1, 'full'),
    ((2, 0, 0, 0, 0, 0, 0, 0), (4, 4), 1, 129, 0, 'observe', 'rows', 'none', 0, 0, 0, -1, -1, ''),
    ((2, 1, 1, 0, 0, 0, 0, 0), (4, 4), 2, 65, 0, 'observe', 'rows', 'none', 0, 0, 0, -1, -1, ''),
    ((2, 2, 0, 0, 0, 0, 0, 0), (4, 4), 3, 33, 0, 'observe', 'rows', 'none', 0, 0, 0, -1, -1, ''),
    ((2, 2, 1, 0, 0, 0, 0, 0), (4, 4), 4, 33, 0, 'observe', 'rows', 'none', 0, 0, 0, -1, -1, ''),
    ((2, 3, 0, 0, 0, 0, 0, 0), (6, 16), 5, 17, 0, 'observe', 'rows', 'none', 0, 0, 0, -1, -1, ''),
    ((2, 3, 1, 0, 0, 0, 0, 0), (6, 16), 6, 17, 0, 'observe', 'rows', 'none', 0, 0, 0, -1, -1, ''),
    ((2, 4, 0, 0, 0, 0, 0, 0), (6, 16), 9, 9, 0, 'observe', 'rows', 'none', 0, 0, 0, -1, -1, ''),
    ((2, 4, 1, 0, 0, 0, 0, 0), (6, 16), 10, 9, 0, 'observe', 'rows', 'none', 0, 0, 0, -1, -1, ''),
    ((2, 5, 0, 0, 0, 0, 0, 0), (6, 16), 17, 5, 0, 'observe', 'rows', 'none', 0, 0, 0, -1, -1, ''),
    ((2, 5, 1, 0, 0, 0, 0, 0), (6, 16), 18, 5, 0, 'observe', 'rows', 'none', 0, 0, 0, -1, -1, ''),
    ((2, 6, 0, 0, 0, 0, 0, 0), (20, 12), 33, 3, 0, 'observe', 'rows', 'none', 0, 0, 0, -1, -1, ''),
    ((2, 6, 1, 0, 0, 0, 0, 0), (20, 12), 34, 3, 0, 'observe', 'rows', 'none', 0, 0, 0, -1, -1, ''),
]


def case_dict(case):
    return dict(zip(CASE_FIELDS, case))


def key_of_case(lib, case, per_cu=(2, 2)):
    """The key the pure functions give the LAST launch of a case's call (ccxi_plan + ccxi_plan_call + the key function)."""
    c = case_dict(case)
    pin = plan_in(*c["grid"], c["N"], c["E"], c["lanes"], c["occ_tables"], int(c["tables"] == "reward"), int(c["tables"] == "terminated"))
    k = Key()
    if c["drive"] == "observe":
        assert lib.ccxi_observe_key(C.byref(pin), C.byref(k)) == 0
        return k.tuple()
    call = CallIn(*call_in(c["K"], DRIVE_NAMES[c["drive"]][0], c["masks"], c["reset"], c["step_kernel"]))
    facts = KeyFacts(*OUTPUTS[c["outputs"]])
    assert lib.ccxi_call_key(C.byref(pin), (C.c_int * 2)(*per_cu), C.byref(call), C.byref(facts), -1, C.byref(k)) == 0
    return k.tuple()
