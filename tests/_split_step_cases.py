"""Seeded inputs of the split-step tests: configs, states, actions / orders and caller arrays for
``tests/test_gpu_split_step_matrix.py`` (the kernels) and ``tests/test_split_step_spec.py`` (which asserts, on the CPU,
that these inputs reach the edges they are meant to reach).  NumPy only; nothing here touches a GPU."""

from __future__ import annotations

from types import SimpleNamespace

import _split_step_spec as spec
import numpy as np

from collectivecrossing_amd import configs as C
from collectivecrossing_amd.params import lower_config

GRIDS = ((12, 8), (40, 30), (100, 100))
# agent counts: 1, 2, 3 pack 64 / 32 / 16 envs into a wave; 17, 31, 33, 50, 63 give a wave a small-output run that is not a
# multiple of 4 bytes; 64 is the whole-wave lane group; odd counts take the 8-byte row units
AGENT_COUNTS = (1, 2, 3, 5, 7, 8, 11, 16, 17, 31, 32, 33, 50, 63, 64)
# boarding agents of each count: both kinds present where N >= 2, a group of ONE on either side, and all of one kind
NUM_BOARDING = {1: 1, 2: 1, 3: 1, 5: 4, 7: 3, 8: 5, 11: 1, 16: 8, 17: 16, 31: 15, 32: 16, 33: 1, 50: 25, 63: 62, 64: 32}

# f64 bit patterns a caller's reward array may hold: they pass through where LIVE, bit for bit
REWARD_BITS = np.array([
    0x7FF8000000000000, 0x7FF8000000000001, 0xFFF8DEADBEEF1234, 0x7FF0000000000001, 0xFFF4000000000BAD,   # quiet / signalling NaN
    0x0000000000000000, 0x8000000000000000, 0x7FF0000000000000, 0xFFF0000000000000,                       # +-0.0, +-inf
    0x0000000000000001, 0x8000000000000001, 0x7FEFFFFFFFFFFFFF, 0xFFEFFFFFFFFFFFFF,                       # denormal, largest finite
    0x3FF0000000000000, 0xBFE0000000000000, 0x400921FB54442D18, 0xC0C3880000000000], np.uint64)          # 1.0, -0.5, pi, -10000
TERM_BYTES = np.array([-128, -2, -1, 0, 1, 2, 127], np.int8)       # entry absent iff -1, true iff 1
TRUNC_BYTES = np.array([0, 1, 2, 128, 255], np.uint8)              # true iff != 0


def lane_group(n: int) -> int:
    g = 1
    while g < n:
        g *= 2
    return g


def make_config(w, h, n, nb=None, max_steps=6, reward="default", terminated="individual_at_destination"):
    """A config of n agents on a w x h grid.  Counts beyond the config validator's cap for the grid (w h / 4: 24 agents on
    12 x 8) are constructed without validation, as the recorded 64-agent fixture is: the library accepts them."""
    nb = NUM_BOARDING[n] if nb is None else nb
    kw = dict(width=w, height=h, division_y=h // 2, tram_door_left=w // 2 - 3, tram_door_right=w // 2 + 1, tram_length=w - 2,
              num_boarding_agents=nb, num_exiting_agents=n - nb, exiting_destination_area_y=0, boarding_destination_area_y=h,
              reward_config=C.get_reward_config(reward), terminated_config=C.get_terminated_config(terminated),
              truncated_config=C.MaxStepsTruncatedConfig(max_steps=max_steps), strict_reference_limits=False)
    try:
        return C.CollectiveCrossingConfig(**kw)
    except ValueError:
        kw.setdefault("observation_config", C.DefaultObservationConfig())
        kw.setdefault("render_mode", None)
        return C.CollectiveCrossingConfig.model_construct(**kw)


def legal_cells(p) -> np.ndarray:
    """[C, 2] every cell an agent may stand on, by the spec's own rule."""
    ys, xs = np.mgrid[0:p.height + 1, 0:p.width + 1]
    ok = spec.cell_ok(p, xs, ys)
    return np.stack([xs[ok], ys[ok]], axis=1).astype(np.int32)


def place(rng, p, E, N, cells=None) -> np.ndarray:
    """[E, N, 2] distinct legal cells per env (a few hundred distinct placements, drawn from with replacement)."""
    cells = legal_cells(p) if cells is None else cells
    base = min(E, 256)
    pick = np.argsort(rng.random((base, len(cells))), axis=1)[:, :N]
    pos = cells[pick]
    return pos if base == E else pos[rng.integers(0, base, size=E)]


def random_state(rng, p, E, N, flags=True, crowd=False, kind_offset=0) -> dict:
    """Placement + (flags=True) every combination of the pre-step flags.  Crafted envs, by ``(e + kind_offset) % 8``:
    1 = nobody LIVE (every agent terminated or truncated earlier); 3 = slot 0 truncated earlier and not terminated."""
    cells = legal_cells(p)
    if crowd:      # everybody near the door line: the rows next to division_y
        near = np.abs(cells[:, 1] - p.division_y) <= max(1, (N // max(p.width // 2, 1)) + 1)
        if near.sum() >= N:
            cells = cells[near]
    pos = place(rng, p, E, N, cells)
    st = spec.make_state(E, N, x=pos[..., 0], y=pos[..., 1])
    st["step_count"] = rng.integers(0, 5, size=E).astype(np.int32)
    if flags:
        st["terminated"] = (rng.random((E, N)) < 0.25).astype(np.uint8)
        st["truncated"] = (rng.random((E, N)) < 0.25).astype(np.uint8)
        kind = (np.arange(E) + kind_offset) % 8
        k1 = kind == 1
        st["terminated"][k1] = np.where(st["truncated"][k1] != 0, st["terminated"][k1], 1)
        st["truncated"][kind == 3, 0] = 1
        st["terminated"][kind == 3, 0] = 0
        # an agent that stands on its destination row has arrived earlier: it is inactive
        st["active"] = ((st["y"] != spec.dest_row(p, N)[None, :]) & (rng.random((E, N)) < 0.9)).astype(np.uint8)
    return st


def random_actions(rng, E, N, toward_door=None, p=None, st=None):
    """Action bytes of every class: 0-3 moves, 4 wait, 5..254 no move, 255 absent."""
    a = rng.integers(0, 5, size=(E, N)).astype(np.uint8)
    if toward_door is not None:        # everybody steps toward the door column / across the line
        x, y = st["x"], st["y"]
        dc = (p.door_left + p.door_right) // 2
        up = (np.arange(N) < p.num_boarding)[None, :]
        vert = np.where(up, 1, 3)
        horiz = np.where(x < dc, 0, 2)
        a = np.where((x != dc) & (rng.random((E, N)) < 0.7), horiz, vert).astype(np.uint8)
    odd = rng.random((E, N))
    a = np.where(odd < 0.06, rng.integers(5, 255, size=(E, N)), a)
    a = np.where((odd >= 0.06) & (odd < 0.12), 255, a)
    return np.ascontiguousarray(a, np.uint8)


def random_orders(rng, E, N):
    return np.ascontiguousarray(np.argsort(rng.random((E, N)), axis=1), np.uint8)


def caller_arrays(rng, st, kind_offset=0):
    """(reward u64 bits, terminated i8, truncated u8) [E, N] from the value pools.  Crafted envs, by ``(e + kind_offset) % 8``:
    0 = every termination entry is -1; 2 = every agent truncates (any non-zero byte); 3 = slot 0 terminates now (with
    :func:`random_state` it was truncated earlier: a non-LIVE agent that is emitted once more)."""
    E, N = st["x"].shape
    r = REWARD_BITS[rng.integers(0, len(REWARD_BITS), size=(E, N))]
    t = TERM_BYTES[rng.integers(0, len(TERM_BYTES), size=(E, N))]
    # (an env-wide "all terminated" needs every present entry to be 1: make that common enough to happen)
    sure = rng.random(E) < 0.15
    t[sure] = np.where(rng.random((int(sure.sum()), N)) < 0.5, 1, -1).astype(np.int8)
    u = TRUNC_BYTES[rng.integers(0, len(TRUNC_BYTES), size=(E, N))]
    kind = (np.arange(E) + kind_offset) % 8
    t[kind == 0] = -1
    u[kind == 2] = TRUNC_BYTES[1:][rng.integers(0, len(TRUNC_BYTES) - 1, size=(int((kind == 2).sum()), N))]
    t[kind == 3, 0] = 1
    return np.ascontiguousarray(r), np.ascontiguousarray(t, np.int8), np.ascontiguousarray(u, np.uint8)


def make_pool(rng, p, P, N) -> np.ndarray:
    return np.ascontiguousarray(place(rng, p, P, N), np.uint8)


# ---------------------------------------------------------------------------------------------------------------------
# the dense begin family: crafted queues + crowds
# ---------------------------------------------------------------------------------------------------------------------
QUEUE_ENVS = 130       # batch size of the dense begin family on the GPU (and of its adequacy check)


def queue_case(p, N, rng, E=6):
    """Envs for ``begin`` with known conflicts.  A queue of m = min(N - 1, W - 1) agents (slots 0 .. m-1) stands in row 1
    at x = 0 .. m-1 and steps right; the last slot steps onto its destination row in the same step (an arrival).
      env 0: the queue moves head first (order m-1, .., 0): every follower enters the cell an EARLIER rank just left;
      env 1: slot order: every follower is blocked by a LATER rank standing on its target, only the head moves;
      env 2: as env 1 with the action bytes of the waiting agents drawn from 5 .. 254 and 255;
      env 3+: random crowds near the door stepping toward it, random permutation orders.
    Returns (state, actions, order)."""
    W = p.width
    m = max(0, min(N - 1, W - 1))
    st = random_state(rng, p, E, N, flags=False, crowd=True)
    acts = random_actions(rng, E, N, toward_door=True, p=p, st=st)
    order = random_orders(rng, E, N)
    cells = legal_cells(p)
    free = cells[(cells[:, 1] >= 2) & (cells[:, 1] != p.exiting_dest_y) & (cells[:, 1] != p.boarding_dest_y)]
    for e in range(min(3, E)):
        rest = free[np.argsort(rng.random(len(free)))[:N - m]]
        st["x"][e, m:], st["y"][e, m:] = rest[:, 0], rest[:, 1]
        st["x"][e, :m], st["y"][e, :m] = np.arange(m), 1
        acts[e] = 4
        acts[e, :m] = 0
        last = N - 1
        if last >= p.num_boarding:          # exiting: from row 1 down onto row 0
            st["x"][e, last], st["y"][e, last] = W, 1
            acts[e, last] = 3
        else:                               # boarding: from the row below the seats up onto them
            st["x"][e, last], st["y"][e, last] = p.tram_left + 1, p.boarding_dest_y - 1
            acts[e, last] = 1
        ident = np.arange(N)
        order[e] = np.concatenate([ident[:m][::-1], ident[m:]]) if e == 0 else ident
        if e == 2 and N - 1 > m:
            acts[e, m:N - 1] = np.where(rng.random(N - 1 - m) < 0.5, 255, rng.integers(5, 255, size=N - 1 - m))
    st["active"][...] = (st["y"] != spec.dest_row(p, N)[None, :]).astype(np.uint8)
    return st, acts, order


def move_events(p, st, actions, order):
    """Serial replay of the move loop (the rule of ``spec.resolve_moves``, one env at a time) that names what happened:
    counts of moves blocked by a LATER rank, moves into a cell an EARLIER rank left in this step, the longest run of
    consecutive ranks that each entered the cell the rank before them left, arrivals, blocks."""
    E, N = st["x"].shape
    ev = SimpleNamespace(blocked_by_later=0, into_vacated=0, longest_chain=0, arrivals=0, blocked=0, moves=0,
                         arrival_with_block=0)
    dest = spec.dest_row(p, N)
    for e in range(E):
        pos = [(int(st["x"][e, i]), int(st["y"][e, i])) for i in range(N)]
        act = [bool(st["active"][e, i]) for i in range(N)]
        rank_of = {int(s): k for k, s in reversed(list(enumerate(order[e])))}
        vacated, chain, prev_left, blocked_here = {}, 0, None, 0
        for k in range(N):
            s = int(order[e, k])
            a = int(actions[e, s]) if s < N else 255
            if s >= N or not act[s] or a > 3:
                prev_left = None
                chain = 0
                continue
            x, y = pos[s]
            tgt = (x + (a == 0) - (a == 2), y + (a == 1) - (a == 3))
            if not bool(spec.cell_ok(p, np.int64(tgt[0]), np.int64(tgt[1]))):
                prev_left, chain = None, 0
                continue
            holder = [j for j in range(N) if j != s and act[j] and pos[j] == tgt]
            if holder:
                ev.blocked += 1
                blocked_here += 1
                ev.blocked_by_later += int(any(rank_of.get(j, -1) > k for j in holder))
                prev_left, chain = None, 0
                continue
            ev.moves += 1
            if tgt in vacated:
                ev.into_vacated += 1
            chain = chain + 1 if (prev_left is not None and tgt == prev_left) else 0
            ev.longest_chain = max(ev.longest_chain, chain)
            vacated[(x, y)] = k
            prev_left = (x, y)
            pos[s] = tgt
        arr = sum(1 for i in range(N) if act[i] and pos[i][1] == dest[i])
        ev.arrivals += arr
        ev.arrival_with_block += int(arr > 0 and blocked_here > 0)
    return ev


# ---------------------------------------------------------------------------------------------------------------------
# the shape matrix
# ---------------------------------------------------------------------------------------------------------------------
E_CLASSES = ("one", "wave-1", "wave+1", "block-1", "block+1", "hundreds", "thousands")


def class_envs(n: int, cls: str, lanes: int = 64, waves_per_block: int = 4) -> int:
    """Batch size of an E class for a launch shape of ``lanes`` lanes per wave and ``waves_per_block`` waves (tiles) per
    workgroup: one wave holds lanes / G envs (G = the lane group of n agents).  The defaults are the begin kernel's fixed
    shape; the GPU matrix re-derives the wave / workgroup classes from the shape the library picks for finish."""
    ew = max(1, lanes // lane_group(n))
    wg = ew * waves_per_block
    return {"one": 1, "wave-1": max(ew - 1, 2) if ew == 1 else max(ew - 1, 1), "wave+1": ew + 1, "block-1": max(wg - 1, 1),
            "block+1": wg + 1, "hundreds": 301 + 14 * (n % 5), "thousands": 1541 + 2 * (n % 7)}[cls]


def matrix_cases():
    """(n, grid, E class) of the default-shape matrix: every agent count meets every grid and every E class (the grid
    cycles with the class, shifted per count, so that the 45 (count, grid) and the 105 (count, class) pairs all occur)."""
    out = []
    for a, n in enumerate(AGENT_COUNTS):
        for c, cls in enumerate(E_CLASSES):
            out.append((n, GRIDS[(a + c) % 3], cls))
    return out


# explicit launch shapes (lanes_per_wave, waves_per_block) per agent count; ccx_set_launch_shape accepts lanes that are a
# multiple of the lane group G and at most 64, and 0 .. 4 waves per block
def explicit_shapes(n: int):
    G = lane_group(n)
    lanes = sorted({G, min(2 * G, 64), 64})
    return [(l, w) for l in lanes for w in (1, 2, 3, 4)]


def refused_shapes(n: int):
    G = lane_group(n)
    bad = [(128, 1), (64, 5), (64, -1)]          # more than a wave; more than 4 / fewer than 0 waves per block
    if G > 1:
        bad.append((G // 2, 1))                  # fewer lanes than one env needs
    if 48 % G:
        bad.append((48, 2))                      # not a whole number of lane groups
    return bad
