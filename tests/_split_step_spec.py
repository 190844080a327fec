"""The split step as include/ccx.h states it (``ccx_step_begin`` / ``ccx_step_finish``, the paragraph "The SPLIT step"),
restated in plain NumPy on the CPU.  TEST INFRASTRUCTURE ONLY: the reference the split-step kernels are compared with.

Written from that paragraph and the reference lines it cites (collectivecrossing.py:188-259), not from the kernels.  It takes
nothing from the product package except the lowered parameter struct; the parts that already exist in the repository's C
oracle (``oracle.OracleBatch``: the ordered move resolution for well-formed input, the observation rows, the built-in reward
/ termination / truncation rules) are taken from there.  Integer and boolean logic only: f64 rewards are moved as u64 bit
patterns, never computed, so every comparison against this module is exact.

Conventions: state arrays are the SoA of ``ccx_state`` ([E, N] i32 x / y, u8 active / terminated / truncated, [E] i32
step_count / episode).  Slots 0 .. num_boarding - 1 are boarding agents, the rest exiting.
"""

from __future__ import annotations

from dataclasses import dataclass, field

import numpy as np

STATE_KEYS = ("x", "y", "active", "terminated", "truncated", "step_count", "episode")
_DTYPES = dict(x=np.int32, y=np.int32, active=np.uint8, terminated=np.uint8, truncated=np.uint8, step_count=np.int32,
               episode=np.int32)

AF_TERMINATED, AF_TRUNCATED, AF_LIVE, AF_OBS = 0x01, 0x02, 0x04, 0x08
AF_IN_TRAM_AREA, AF_AT_DOOR, AF_ACTIVE, AF_AT_DEST = 0x10, 0x20, 0x40, 0x80
EF_ALL_TERMINATED, EF_ALL_TRUNCATED, EF_RESET = 0x01, 0x02, 0x04


def make_state(E, N, **kw) -> dict:
    """A state dict of the right dtypes: all agents at (0, 0), active, no flag, counters 0 -- overridden by ``kw``."""
    st = dict(x=np.zeros((E, N), np.int32), y=np.zeros((E, N), np.int32), active=np.ones((E, N), np.uint8),
              terminated=np.zeros((E, N), np.uint8), truncated=np.zeros((E, N), np.uint8),
              step_count=np.zeros(E, np.int32), episode=np.zeros(E, np.int32))
    for k, v in kw.items():
        st[k] = np.ascontiguousarray(np.asarray(v, _DTYPES[k]).reshape(st[k].shape))
    return st


def copy_state(st: dict) -> dict:
    return {k: np.array(st[k], _DTYPES[k], copy=True) for k in STATE_KEYS}


# ---------------------------------------------------------------------------------------------------------------------
# geometry (collectivecrossing.py:509-563, 663-683)
# ---------------------------------------------------------------------------------------------------------------------
def cell_ok(p, x, y):
    """_is_valid_position (:509-534) for arrays of cells."""
    ok = (x >= 0) & (x <= p.width) & (y >= 0) & (y <= p.height)
    ok &= (y != p.division_y) | ((p.door_left < x) & (x < p.door_right))
    ok &= (y < p.division_y) | ((p.tram_left < x) & (x < p.tram_right))
    return ok


def dest_row(p, N):
    """[N] destination row of every slot (:663-683)."""
    return np.where(np.arange(N) < p.num_boarding, p.boarding_dest_y, p.exiting_dest_y).astype(np.int32)


def well_formed_orders(order, N):
    """[E] bool: the row is a permutation of 0 .. N-1 (``None`` = slot order = well formed)."""
    order = np.asarray(order)
    return (np.sort(order.astype(np.int64), axis=1) == np.arange(N)[None, :]).all(axis=1)


# ---------------------------------------------------------------------------------------------------------------------
# begin = collectivecrossing.py:188-212
# ---------------------------------------------------------------------------------------------------------------------
def resolve_moves(p, st, actions, order=None):
    """The ordered move resolution, one move rank at a time for all envs at once, stated for ANY order bytes:

    * rank k names slot ``order[e, k]``; a byte >= N names no agent and moves nothing;
    * an agent proposes the neighbour cell of the cell it stood on before the step (action 0 right, 1 up, 2 left, 3 down;
      every other byte -- wait 4, absent 255, 5 .. 254 -- proposes nothing); only ACTIVE agents move (:685-711);
    * the move happens iff the cell is legal (:509-534) and no OTHER ACTIVE agent stands on it at that moment (:536-541,
      activity as before the step: deactivation comes after all moves, :210-212);
    * an agent moves at most once per step: a slot named again after it moved does nothing (a slot named again after it
      was blocked tries again).
    Returns (x, y, moved [E, N] bool)."""
    E, N = st["x"].shape
    a = np.asarray(actions, np.uint8).reshape(E, N).astype(np.int64)
    order = np.broadcast_to(np.arange(N), (E, N)) if order is None else np.asarray(order, np.uint8).reshape(E, N)
    x, y = st["x"].astype(np.int64), st["y"].astype(np.int64)
    act = st["active"] != 0
    nx = x + (a == 0) - (a == 2)
    ny = y + (a == 1) - (a == 3)
    may = act & (a < 4) & cell_ok(p, nx, ny)
    moved = np.zeros((E, N), bool)
    rows = np.arange(E)
    for k in range(N):
        s = order[:, k].astype(np.int64)
        named = s < N
        si = np.where(named, s, 0)
        tx, ty = nx[rows, si], ny[rows, si]
        others = act & (x == tx[:, None]) & (y == ty[:, None])
        others[rows, si] = False
        go = named & may[rows, si] & ~moved[rows, si] & ~others.any(axis=1)
        x[rows, si] = np.where(go, tx, x[rows, si])
        y[rows, si] = np.where(go, ty, y[rows, si])
        moved[rows, si] |= go
    return x.astype(np.int32), y.astype(np.int32), moved


def begin(p, st, actions, order=None, oracle=None):
    """``ccx_step_begin``: step_count += 1, the moves, deactivation on arrival; flags and episode untouched.
    Returns (state, moves, arrivals).  With ``oracle`` (the module ``oracle.oracle``) envs whose order row is a permutation
    take their positions from ``OracleBatch.step``; malformed rows always take the rule of :func:`resolve_moves`."""
    E, N = st["x"].shape
    out = copy_state(st)
    wf = np.ones(E, bool) if order is None else well_formed_orders(order, N)
    x, y, moved = resolve_moves(p, st, actions, order)
    if oracle is not None and wf.any():
        idx = np.nonzero(wf)[0]
        b = oracle.OracleBatch(p, len(idx))
        b.set_state(x=st["x"][idx], y=st["y"][idx], active=st["active"][idx], terminated=st["terminated"][idx],
                    truncated=st["truncated"][idx], step_count=st["step_count"][idx])
        b.step(np.ascontiguousarray(np.asarray(actions, np.uint8).reshape(E, N)[idx]),
               None if order is None else np.ascontiguousarray(np.asarray(order, np.uint8).reshape(E, N)[idx]), want_obs=False)
        moved[idx] = (b.x != st["x"][idx]) | (b.y != st["y"][idx])
        x[idx], y[idx] = b.x, b.y
    dest = y == dest_row(p, N)[None, :]
    arrive = (st["active"] != 0) & dest
    out["x"], out["y"] = x, y
    out["active"] = ((st["active"] != 0) & ~dest).astype(np.uint8)
    out["step_count"] = (st["step_count"] + 1).astype(np.int32)
    return out, int(moved.sum()), int(arrive.sum())


# ---------------------------------------------------------------------------------------------------------------------
# finish = collectivecrossing.py:214-259
# ---------------------------------------------------------------------------------------------------------------------
@dataclass
class Finish:
    reward_bits: np.ndarray      # u64 [E, N]
    agent_flags: np.ndarray      # u8  [E, N]
    env_flags: np.ndarray        # u8  [E]
    term_present: np.ndarray     # u8  [E, N]
    emitted: np.ndarray          # bool [E, N]  (= AF_OBS)
    obs_compact: np.ndarray      # f32 [E, N, 4] of the state begin left
    state: dict                  # the state after finish
    counters: dict = field(default_factory=dict)   # env_steps, agent_steps, live_agent_steps, episodes


def pool_entry(global_env: int, episode: int, pool_size: int, total_envs: int) -> int:
    """ccx_set_reset_pool: entry ``(g + j * stride) mod P`` with ``stride = total_envs mod P, or 1 when P divides
    total_envs``.  Exact integers (Python ints).  THE statement of the cursor: every spec module takes it from here."""
    P = int(pool_size)
    stride = int(total_envs) % P or 1
    return (int(global_env) + int(episode) * stride) % P


def pool_cursor(env_offset, total_envs, pool_size, env, episode):
    """:func:`pool_entry` of env ``env`` of the shard that starts at global env ``env_offset``."""
    return pool_entry(int(env_offset) + int(env), episode, pool_size, total_envs)


def builtin_arrays(oracle, p, st, tables=None):
    """What the handle's built-in rules (incl. installed position-only tables, ``tables`` = (reward pair, terminated pair))
    give on the state begin left: (reward f64, terminated i8, truncated u8), from the C oracle stepped with nobody moving."""
    E, N = st["x"].shape
    b = oracle.OracleBatch(p, E)
    b.set_state(**{k: st[k] for k in ("x", "y", "active", "terminated", "truncated")}, step_count=st["step_count"] - 1)
    if tables is not None:
        b.set_user_tables(reward=tables[0], terminated=tables[1])
    _, rew, af, _ = b.step(np.full((E, N), 255, np.uint8), None, want_obs=False)
    assert (b.x == st["x"]).all() and (b.y == st["y"]).all() and (b.step_count == st["step_count"]).all()
    return rew, (af & 1).astype(np.int8), ((af >> 1) & 1).astype(np.uint8)


def finish(p, st, reward, terminated, truncated, auto_reset=False, pool=None, env_offset=0, total_envs=None) -> Finish:
    """``ccx_step_finish`` with all three caller arrays given (a NULL array of the C call = :func:`builtin_arrays`).
    reward: f64 or u64 bit patterns [E, N]; terminated: i8 (entry absent iff -1, true iff 1); truncated: u8 (true iff != 0,
    counted only where LIVE -- the termination value is NOT masked by LIVE: terminateds[id] exists for done agents too)."""
    E, N = st["x"].shape
    total_envs = E if total_envs is None else total_envs
    rb = np.ascontiguousarray(np.asarray(reward).reshape(E, N))
    rb = rb.view(np.uint64) if rb.dtype == np.float64 else rb.astype(np.uint64)
    t = np.asarray(terminated).reshape(E, N).astype(np.int64)
    u = np.asarray(truncated).reshape(E, N).astype(np.int64)
    term0, trunc0 = st["terminated"] != 0, st["truncated"] != 0
    live = ~term0 & ~trunc0
    t1, present = t == 1, t != -1
    u1 = live & (u != 0)
    all_term = present.any(axis=1) & (t1 | ~present).all(axis=1)         # :256 all(values) if terminateds else False
    all_trunc = live.any(axis=1) & (u1 | ~live).all(axis=1)              # :257
    reset = (all_term | all_trunc) & bool(auto_reset) & (pool is not None and len(pool) > 0)
    emitted = live | (t1 & ~term0) | (u1 & ~trunc0)                      # :229-243
    x, y, act = st["x"], st["y"], st["active"] != 0
    in_tram = (y >= p.division_y) & (p.tram_left <= x) & (x <= p.tram_right)                   # :551-554
    at_door = (y == p.division_y) & ((x == p.door_left - 1) | (x == p.door_right + 1))         # :556-563
    at_dest = y == dest_row(p, N)[None, :]
    af = (t1 * AF_TERMINATED | u1 * AF_TRUNCATED | live * AF_LIVE | emitted * AF_OBS | in_tram * AF_IN_TRAM_AREA |
          at_door * AF_AT_DOOR | act * AF_ACTIVE | at_dest * AF_AT_DEST).astype(np.uint8)
    ef = (all_term * EF_ALL_TERMINATED | all_trunc * EF_ALL_TRUNCATED | reset * EF_RESET).astype(np.uint8)
    typ = np.broadcast_to((np.arange(N) >= p.num_boarding), (E, N))
    compact = np.stack([x, y, typ, act], axis=-1).astype(np.float32)
    new = copy_state(st)
    new["terminated"] = (term0 | t1).astype(np.uint8)
    new["truncated"] = (trunc0 | u1).astype(np.uint8)
    for e in np.nonzero(reset)[0]:
        entry = pool[pool_cursor(env_offset, total_envs, len(pool), e, int(st["episode"][e]) + 1)]
        new["x"][e], new["y"][e] = entry[:, 0], entry[:, 1]
        new["active"][e], new["terminated"][e], new["truncated"][e] = 1, 0, 0
        new["episode"][e] = st["episode"][e] + 1
        new["step_count"][e] = 0
    counters = dict(env_steps=E, agent_steps=E * N, live_agent_steps=int(live.sum()), episodes=int(reset.sum()))
    return Finish(np.where(live, rb, np.uint64(0)), af, ef, present.astype(np.uint8), emitted, compact, new, counters)


def observe(oracle, p, st):
    """DefaultObservation rows [E, N, L] of a state (observations.py:43-94), from the C oracle."""
    E, N = st["x"].shape
    b = oracle.OracleBatch(p, E)
    b.set_state(x=st["x"], y=st["y"], active=st["active"])
    return b.observe()
