"""NumPy restatement of the CCX_RENDER frame spec (include/ccx.h), integers only.

``render_frame(geom, xs, ys, types, cp)`` draws one frame the way ``ccx_render`` must, bit for bit: every test is
written in half-pixel units, u = 2c + 1 for column c and v = 2cp H - 2r - 1 for row r.
"""

from __future__ import annotations

import numpy as np


def _rgb(hex_: str) -> np.ndarray:
    h = hex_.lstrip("#")
    return np.array([int(h[i:i + 2], 16) for i in (0, 2, 4)], np.int64)


BACKGROUND = _rgb("#f8f9fa")
TRAM = _rgb("#e3f2fd")
WAITING = _rgb("#fff3e0")
EXIT = _rgb("#f44336")
SEATS = _rgb("#2196f3")
WALL = _rgb("#424242")
DOOR = _rgb("#90caf9")
BOARDING_FACE, BOARDING_EDGE = _rgb("#f44336"), _rgb("#8b0000")
EXITING_FACE, EXITING_EDGE = _rgb("#2196f3"), _rgb("#00008b")
GRID = _rgb("#808080")
DISCS = ((4, 77), (3, 128), (2, 204))          # radius k/10, alpha byte


def alpha_byte(alpha: float) -> int:
    return int(np.floor(255 * alpha + 0.5))


def blend(dst: np.ndarray, src: np.ndarray, a: int, where: np.ndarray) -> np.ndarray:
    """out = (a src + (255 - a) dst + 127) // 255 where `where`, dst elsewhere (dst int64 [..., 3])."""
    src = np.broadcast_to(np.asarray(src, np.int64), dst.shape)
    mixed = (a * src + (255 - a) * dst + 127) // 255
    return np.where(where[..., None], mixed, dst)


def geometry(params) -> dict:
    """The fields of ``ccx_params`` (or a ``CcxParams``) the frame needs."""
    g = {k: int(getattr(params, k)) for k in ("width", "height", "division_y", "tram_left", "tram_right",
                                                "door_left", "door_right", "boarding_dest_y", "exiting_dest_y")}
    return g


def wall_thickness(cp: int) -> int:
    return max(1, (cp + 5) // 10)


def static_layers(g: dict, cp: int):
    """Colour after layers 1-7 (int64 [H cp, W cp, 3]) and the grid-line mask (layer 9)."""
    W, H = g["width"], g["height"]
    div, tl, tr, dl, dr = g["division_y"], g["tram_left"], g["tram_right"], g["door_left"], g["door_right"]
    by, ey = g["boarding_dest_y"], g["exiting_dest_y"]
    Hpx, Wpx, S = H * cp, W * cp, 2 * cp
    r = np.arange(Hpx)[:, None]
    c = np.arange(Wpx)[None, :]
    u = 2 * c + 1
    v = S * H - 2 * r - 1

    def rect(x0_2cp, x1_2cp, y0_2cp, y1_2cp):       # bounds already multiplied by 2cp
        return (u >= x0_2cp) & (u < x1_2cp) & (v >= y0_2cp) & (v < y1_2cp)

    img = np.broadcast_to(BACKGROUND, (Hpx, Wpx, 3)).astype(np.int64)
    img = blend(img, TRAM, 179, rect(S * tl, S * (tr + 1), S * div, S * H))
    img = blend(img, WAITING, 179, rect(0, S * W, 0, S * div))
    if ey < div:
        img = blend(img, EXIT, 204, rect(0, S * W, S * ey, S * (ey + 1)))
    if by >= div:
        ys = H - 1 if by == H else by
        img = blend(img, SEATS, 204, rect(S * tl, S * (tr + 1), S * ys, S * (ys + 1)))
    t = wall_thickness(cp)
    cw_l = min(max(cp * tl - t // 2, 0), Wpx - t)
    cw_r = min(max(cp * (tr + 1) - t // 2, 0), Wpx - t)
    rw_h = min(max(cp * (H - div) - t // 2, 0), Hpx - t)
    above = r < cp * (H - div)
    wall = above & (((c >= cw_l) & (c < cw_l + t)) | ((c >= cw_r) & (c < cw_r + t)))
    hrow = (r >= rw_h) & (r < rw_h + t)
    if dl > tl:
        wall = wall | (hrow & (u >= S * tl) & (u < cp * (2 * dl + 1)))
    if dr < tr:
        wall = wall | (hrow & (u >= cp * (2 * dr - 1)) & (u < S * (tr + 1)))
    img = blend(img, WALL, 230, wall)
    if dr - dl - 1 > 0:
        img = blend(img, DOOR, 204, rect(cp * (2 * dl + 1), cp * (2 * dr - 1), S * div, S * (div + 1)))
    if cp >= 4:
        grid = (c % cp == 0) | (c == Wpx - 1) | (r % cp == 0) | (r == Hpx - 1)
    else:
        grid = np.zeros((Hpx, Wpx), bool)
    return img, np.broadcast_to(grid, (Hpx, Wpx))


def draw_agents(img: np.ndarray, g: dict, cp: int, xs, ys, types) -> np.ndarray:
    """Layer 8 on top of `img` (int64 [H cp, W cp, 3]); types 0 boarding / 1 exiting, slot order."""
    W, H = g["width"], g["height"]
    Hpx, Wpx, S = H * cp, W * cp, 2 * cp
    img = img.copy()
    for x, y, typ in zip(xs, ys, types):
        x, y = int(x), int(y)
        if not (0 <= x <= W and 0 <= y <= H):
            continue
        # every disc lies within half a cell of its centre: work on that window only
        r0, r1 = max(cp * (H - y) - cp, 0), min(cp * (H - y) + cp, Hpx)
        c0, c1 = max(cp * x - cp, 0), min(cp * x + cp, Wpx)
        r = np.arange(r0, r1)[:, None]
        c = np.arange(c0, c1)[None, :]
        d25 = 25 * ((2 * c + 1 - S * x) ** 2 + (S * H - 2 * r - 1 - S * y) ** 2)
        face, edge = (EXITING_FACE, EXITING_EDGE) if typ else (BOARDING_FACE, BOARDING_EDGE)
        win = img[r0:r1, c0:c1]
        for k, a in DISCS:
            kc = k * cp
            inside = d25 <= kc * kc
            ring = inside & ((kc <= 10) | (d25 > (kc - 10) ** 2))
            win = blend(win, edge, a, ring)
            win = blend(win, face, a, inside & ~ring)
        img[r0:r1, c0:c1] = win
    return img


def render_frame(g: dict, xs, ys, types, cp: int) -> np.ndarray:
    """One frame, uint8 [H cp, W cp, 3]."""
    img, grid = static_layers(g, cp)
    img = draw_agents(img, g, cp, xs, ys, types)
    img = blend(img, GRID, 179, grid)
    return img.astype(np.uint8)


def render_state(g: dict, x: np.ndarray, y: np.ndarray, num_boarding: int, cp: int, env_ids=None) -> np.ndarray:
    """Frames of a SoA state x, y [E][N] (ccx_render): [R, H cp, W cp, 3]; ids outside [0, E) = static layers only."""
    E, N = x.shape
    ids = range(E) if env_ids is None else [int(e) for e in env_ids]
    types = [0 if a < num_boarding else 1 for a in range(N)]
    img, grid = static_layers(g, cp)
    out = []
    for e in ids:
        frame = draw_agents(img, g, cp, x[e], y[e], types) if 0 <= e < E else img
        out.append(blend(frame, GRID, 179, grid).astype(np.uint8))
    W, H = g["width"], g["height"]
    return np.stack(out) if out else np.zeros((0, H * cp, W * cp, 3), np.uint8)


def render_compact(g: dict, compact: np.ndarray, cp: int) -> np.ndarray:
    """Frames of compact rows f32 [..., N, 4] (ccx_render_compact): [..., H cp, W cp, 3]."""
    lead = compact.shape[:-2]
    rows = compact.reshape(-1, compact.shape[-2], 4)
    img, grid = static_layers(g, cp)
    out = []
    for row in rows:
        keep = (row[:, 0] >= 0) & (row[:, 0] <= g["width"]) & (row[:, 1] >= 0) & (row[:, 1] <= g["height"])
        frame = draw_agents(img, g, cp, row[keep, 0].astype(np.int64), row[keep, 1].astype(np.int64),
                            (row[keep, 2] != 0).astype(np.int64))
        out.append(blend(frame, GRID, 179, grid).astype(np.uint8))
    W, H = g["width"], g["height"]
    return np.stack(out).reshape(*lead, H * cp, W * cp, 3) if out else np.zeros((*lead, H * cp, W * cp, 3), np.uint8)
