"""Shared by the legal-action mask tests: the fixtures of tests/golden/gen_action_masks.py, an independent NumPy spec of
``ccx_action_masks`` (include/ccx.h: CCX_ACTION_MASKS) and random states for it."""

from __future__ import annotations

import json
from pathlib import Path

import numpy as np

from _fixtures import config_from_dict
from collectivecrossing_amd.params import lower_config

MASKS_DIR = Path(__file__).resolve().parent / "golden" / "action_masks"
MASK_NPZ = sorted(p.stem for p in MASKS_DIR.glob("g15_action_masks_*.npz"))
DIRS = ((1, 0), (0, 1), (-1, 0), (0, -1))          # actions 0..3: right, up, left, down
WAIT_ONLY = 0x10


class MaskFixture:
    def __init__(self, name: str):
        self.name = name
        with np.load(MASKS_DIR / f"{name}.npz") as z:
            self.a = {k: z[k] for k in z.files}
        self.cfg_dict = json.loads(str(self.a["config_json"]))
        self.config = config_from_dict(self.cfg_dict)
        self.params = lower_config(self.config)
        self.S, self.N = self.a["masks"].shape

    def __getitem__(self, k):
        return self.a[k]

    def state(self) -> dict:
        """The S recorded states as a batch of S envs."""
        return {k: self.a[k] for k in ("x", "y", "active", "terminated", "truncated")}


def enterable(oracle, params) -> np.ndarray:
    """bool [H + 3, W + 3], index [y + 1, x + 1]: the cell can be entered as far as the geometry goes -- inside the grid,
    ``_is_valid_position`` and not ``_would_hit_tram_wall`` (collectivecrossing.py:345-369 without the occupancy term)."""
    W, H = params.width, params.height
    t = np.zeros((H + 3, W + 3), bool)
    for y in range(H + 1):
        for x in range(W + 1):
            t[y + 1, x + 1] = oracle.is_valid_position(params, x, y) and not oracle.would_hit_tram_wall(params, x, y)
    return t


def spec_masks(oracle, params, x, y, active, terminated, truncated) -> np.ndarray:
    """u8 [E, N]: the mask bytes, from the geometry predicate of the CPU oracle and an all-pairs occupancy compare."""
    x, y = np.asarray(x, np.int64), np.asarray(y, np.int64)
    act = np.asarray(active) != 0
    done = (np.asarray(terminated) != 0) | (np.asarray(truncated) != 0)
    ok = enterable(oracle, params)
    E, N = x.shape
    other = ~np.eye(N, dtype=bool)[None]                                      # [1, i, b]
    out = np.full((E, N), WAIT_ONLY, np.uint8)
    for a, (dx, dy) in enumerate(DIRS):
        tx, ty = x + dx, y + dy
        taken = ((tx[:, :, None] == x[:, None, :]) & (ty[:, :, None] == y[:, None, :]) & act[:, None, :] & other).any(-1)
        out |= ((ok[ty + 1, tx + 1] & ~taken & ~done).astype(np.uint8) << a).astype(np.uint8)
    return out


def random_states(oracle, params, E: int, seed: int, p_inactive=0.2, p_trunc=0.15, p_term=0.1, crowd=True) -> dict:
    """E random states on enterable cells.  Active agents never share a cell; inactive ones (arrived) may sit on any
    agent's cell; truncated agents keep their `active` flag (they block), terminated ones are inactive or not; with
    `crowd` the agents are drawn around a few centres, so that neighbours are common."""
    rng = np.random.default_rng(seed)
    N = params.num_agents
    ok = enterable(oracle, params)[1:-1, 1:-1]
    cells = np.argwhere(ok)                                                   # (y, x)
    st = dict(x=np.zeros((E, N), np.int32), y=np.zeros((E, N), np.int32), active=np.ones((E, N), np.uint8),
              terminated=np.zeros((E, N), np.uint8), truncated=np.zeros((E, N), np.uint8))
    for e in range(E):
        if crowd:
            c = cells[rng.integers(len(cells))]
            near = cells[np.abs(cells - c).sum(1) <= max(2, int(np.sqrt(N)) + 1)]
            pool = near if len(near) >= N else cells
        else:
            pool = cells
        pick = pool[rng.permutation(len(pool))[:N]] if len(pool) >= N else pool[rng.integers(len(pool), size=N)]
        inactive = rng.random(N) < p_inactive
        if len(pool) < N:
            inactive[:] = True
            inactive[0] = False
        for i in range(N):
            if inactive[i] and i and rng.random() < 0.5:
                pick[i] = pick[rng.integers(i)]                               # an arrived agent on somebody's cell
        st["y"][e], st["x"][e] = pick[:, 0], pick[:, 1]
        st["active"][e] = ~inactive
        st["truncated"][e] = rng.random(N) < p_trunc
        st["terminated"][e] = rng.random(N) < p_term
    return st
