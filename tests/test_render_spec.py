"""CPU checks of the CCX_RENDER frame spec (include/ccx.h) through its NumPy restatement (tests/_render_spec.py).

The restatement against the reference's own Agg frames (tests/golden/render, written by gen_render_golden.py: the RGB at
cell centres and inside each agent's innermost disc, where the reference's 7 x 7 neighbourhood is uniform), within 2 per
channel; and the spec's properties: clipping at the frame edge, grid lines over agents, slot order of co-located agents,
walls at cp = 1."""

from pathlib import Path

import numpy as np
import pytest

import _render_spec as spec

GOLDEN = Path(__file__).resolve().parent / "golden" / "render"
FIXTURES = sorted(GOLDEN.glob("*.npz"))
GEOM_KEYS = ("width", "height", "division_y", "tram_left", "tram_right", "door_left", "door_right",
             "boarding_dest_y", "exiting_dest_y")
CP = 50          # 0.08 cells = 4 px: every sampled point lies well inside its region at this cell size


def load_fixture(path):
    z = np.load(path)
    return dict(zip(GEOM_KEYS, (int(v) for v in z["geometry"]))), z


def sample_points(g, z, cp):
    """(row, col, expected rgb) of every usable fixture point in a frame of cell size cp."""
    W, H = g["width"], g["height"]
    pts = []
    for j in range(H):
        for i in range(W):
            if z["cell_ok"][j, i]:
                pts.append((cp * (H - j - 1) + cp // 2, cp * i + cp // 2, z["cell_rgb"][j, i]))
    d = int(round(0.08 * cp))
    for k in range(len(z["x"])):
        r, c = cp * (H - int(z["y"][k])) - d, cp * int(z["x"][k]) + d
        if z["agent_ok"][k] and 0 <= r < H * cp and 0 <= c < W * cp:
            pts.append((r, c, z["agent_rgb"][k]))
    return pts


def test_fixtures_exist():
    assert len(FIXTURES) >= 5


@pytest.mark.parametrize("path", FIXTURES, ids=[p.stem for p in FIXTURES])
def test_restatement_matches_the_reference_frames(path):
    g, z = load_fixture(path)
    frame = spec.render_frame(g, z["x"], z["y"], z["types"], CP)
    pts = sample_points(g, z, CP)
    assert len(pts) >= 0.8 * g["width"] * g["height"]
    got = np.array([frame[r, c] for r, c, _ in pts], np.int64)
    want = np.array([w for _, _, w in pts], np.int64)
    bad = np.abs(got - want).max(axis=1) > 2
    assert not bad.any(), [(pts[i][:2], got[i].tolist(), want[i].tolist()) for i in np.flatnonzero(bad)]


def test_alpha_bytes_and_palette():
    assert [spec.alpha_byte(a) for a in (0.3, 0.5, 0.7, 0.8, 0.9)] == [77, 128, 179, 204, 230]
    bg = spec.BACKGROUND[None, :]
    waiting = spec.blend(bg, spec.WAITING, 179, np.ones(1, bool))[0]
    assert waiting.tolist() == [253, 245, 232]          # the reference's Agg pixel: 252, 244, 231


C2 = dict(width=12, height=8, division_y=4, tram_left=2, tram_right=10, door_left=7, door_right=9,
          boarding_dest_y=8, exiting_dest_y=0)


def _static(g, cp):
    img, grid = spec.static_layers(g, cp)
    return spec.blend(img, spec.GRID, 179, grid).astype(np.uint8)


def test_discs_at_the_frame_edge_are_clipped_to_half():
    cp = 20
    g = dict(C2)
    base = _static(g, cp)
    corner = spec.render_frame(g, [0], [0], [0], cp) != base        # bottom-left corner: a quarter of the discs
    inner = spec.render_frame(g, [3], [2], [0], cp) != base
    edge_x = spec.render_frame(g, [0], [2], [0], cp) != base        # on x = 0: the right half
    n_inner, n_edge, n_corner = (int(m.any(axis=2).sum()) for m in (inner, edge_x, corner))
    assert n_inner > 0
    assert abs(n_edge - n_inner / 2) <= cp and abs(n_corner - n_inner / 4) <= cp
    rows, cols = np.nonzero(edge_x.any(axis=2))
    assert cols.min() == 0 and cols.max() < cp / 2


def test_grid_lines_lie_over_agents():
    cp = 16
    g = dict(C2)
    frame = spec.render_frame(g, [3], [2], [1], cp)
    H = g["height"]
    r, c = cp * (H - 2), 3 * cp                                     # the grid crossing under the agent's centre
    img, _ = spec.static_layers(g, cp)
    under = spec.draw_agents(img, g, cp, [3], [2], [1])
    for rr, cc in ((r, c), (r, c + 2), (r + 2, c)):               # on the lines through the agent's centre
        assert under[rr, cc].tolist() != img[rr, cc].tolist()     # a disc is there ...
        want = spec.blend(under[rr, cc][None, :], spec.GRID, 179, np.ones(1, bool))[0]
        assert frame[rr, cc].tolist() == want.tolist()            # ... and the grid line lies over it
    assert frame[r + 2, c + 2].tolist() == under[r + 2, c + 2].tolist()   # off the lines the disc shows as is


def test_co_located_agents_blend_in_slot_order():
    cp = 20
    g = dict(C2)
    ab = spec.render_frame(g, [4, 4], [1, 1], [0, 1], cp)
    ba = spec.render_frame(g, [4, 4], [1, 1], [1, 0], cp)
    one = spec.render_frame(g, [4], [1], [1], cp)
    assert not np.array_equal(ab, ba)
    # the later slot is on top: its innermost face colour dominates the centre
    r, c = cp * (g["height"] - 1) + 1, 4 * cp + 1
    assert int(ab[r, c, 2]) > int(ba[r, c, 2])
    assert not np.array_equal(ab, one)


def test_cp1_has_no_grid_and_walls_of_one_pixel():
    g = dict(C2)
    img, grid = spec.static_layers(g, 1)
    assert not grid.any()
    frame = spec.render_frame(g, [], [], [], 1)
    assert spec.wall_thickness(1) == 1 and spec.wall_thickness(8) == 1 and spec.wall_thickness(15) == 2
    # the vertical walls: one column each, above division_y
    H, div = g["height"], g["division_y"]
    wall_col = frame[: H - div, g["tram_left"]]
    assert (wall_col[:, 0] < 110).all()
    # the same frame at cp = 2: no grid yet, walls still one pixel
    f2 = spec.render_frame(g, [], [], [], 2)
    dark = (f2[:, :, 0] < 110)
    assert dark[:2 * (H - div), 2 * g["tram_left"]].all()
    assert not dark[2:2 * (H - div), 2 * g["tram_left"] + 1].any()   # (rows 0, 1: the seats row)


def test_frame_shape_and_dtype():
    g = dict(C2)
    f = spec.render_frame(g, [1, 2], [3, 4], [0, 1], 7)
    assert f.shape == (8 * 7, 12 * 7, 3) and f.dtype == np.uint8
    st = spec.render_state(g, np.array([[1, 2]]), np.array([[3, 4]]), 1, 7, env_ids=[0, 5, 0])
    assert st.shape == (3, 56, 84, 3)
    assert np.array_equal(st[0], f) and np.array_equal(st[2], f) and np.array_equal(st[1], spec.render_frame(g, [], [], [], 7))
