"""The NumPy / Python-integer spec of CCX_REPLAY (tests/_replay_spec.py) checked against itself and against the constants
the library states (csrc/ccx_replay.h, collectivecrossing_amd/replay.py): the slot map, the push, the rows, the draw's range
at the edges of its domain and its statistics.  No GPU."""

import re
from pathlib import Path

import numpy as np
import pytest
from _replay_spec import (ARRAYS, EMPTY_ACTION, EMPTY_MASKS, K_REPLAY_STREAM, MASKS_ALL, draw_one, draw_spec, fetch_spec, filled_spec,
                          new_ring, push_spec, rows_spec, sample_index_spec, slot_spec)

from collectivecrossing_amd import replay as lib_replay

CSRC = Path(lib_replay.__file__).parent / "csrc"
SEED = 0x0123_4567_89AB_CDEF


def test_constants_are_the_headers():
    text = (CSRC / "ccx_replay.h").read_text()
    kern = (CSRC / "ccx_kernels.h").read_text()
    assert int(re.search(r"kStream = (0x[0-9A-Fa-f]+)u", text).group(1), 16) == K_REPLAY_STREAM
    assert int(re.search(r"kReplayStream = (0x[0-9A-Fa-f]+)u", kern).group(1), 16) == K_REPLAY_STREAM
    assert int(re.search(r"kEmptyMasks = (0x[0-9A-Fa-f]+)u", text).group(1), 16) == EMPTY_MASKS == lib_replay.EMPTY_MASKS
    assert int(re.search(r"kMasksAll = (0x[0-9A-Fa-f]+)u", text).group(1), 16) == MASKS_ALL
    assert int(re.search(r"kEmptyAction = (\d+)u", text).group(1)) == EMPTY_ACTION == lib_replay.EMPTY_ACTION
    others = (0, 0x5BD1E995, 0x2545F491, 0x68E31DA4, 0xB5297A4D)
    assert K_REPLAY_STREAM not in others


def test_geometry_and_batch_size_limits():
    assert lib_replay._check_geometry(64, 4096, 8) == 64
    assert lib_replay._check_geometry(1, (1 << 31) - 1, 8) == 1
    for steps, E in ((0, 8), (-1, 8), (1.5, 8), ("x", 8), (1, 1 << 31), (1 << 20, 1 << 11)):
        with pytest.raises(ValueError):
            lib_replay._check_geometry(steps, E, 8)
    assert lib_replay._check_batch_size((1 << 31) // 8, 8) == 1 << 28
    assert lib_replay._check_batch_size(1, 3) == 1
    for B, N in ((0, 8), (-4, 8), ((1 << 28) + 1, 8), (2.5, 8), (None, 8), ((1 << 31) // 3 + 1, 3)):
        with pytest.raises(ValueError):
            lib_replay._check_batch_size(B, N)


def test_slot_map_and_filled():
    S, E = 4, 3
    assert [slot_spec(0, s, S, E, 1) for s in range(4)] == [1, 4, 7, 10]
    assert [slot_spec(3, s, S, E, 2) for s in range(3)] == [11, 2, 5]          # a block that wraps inside itself
    assert slot_spec(4 * 10**12 + 1, 2, S, E, 0) == 9
    for head in range(0, 13):
        slots = {slot_spec(head, s, S, E, e) for s in range(S) for e in range(E)}
        assert slots == set(range(S * E))                                        # K == S rewrites every slot once
    assert [filled_spec(h, S, E) for h in (0, 1, 3, 4, 5, 400)] == [0, 3, 9, 12, 12, 12]


def _block(rng, K, E, N, with_final=True, with_masks=True):
    ef = (rng.random((K, E)) < 0.4).astype(np.uint8) * 0x04 | (rng.random((K, E)) < 0.5).astype(np.uint8)
    return dict(obs0_compact=rng.standard_normal((E, N, 4)).astype(np.float32), actions=rng.integers(0, 5, (K, E, N), dtype=np.uint8),
                reward=rng.standard_normal((K, E, N)), agent_flags=rng.integers(0, 256, (K, E, N), dtype=np.uint8), env_flags=ef,
                obs_compact=rng.standard_normal((K, E, N, 4)).astype(np.float32),
                final_compact=rng.standard_normal((K, E, N, 4)).astype(np.float32) if with_final else None,
                masks_next=rng.integers(0, 32, (K, E, N), dtype=np.uint8) if with_masks else None)


def test_push_fields_and_wrap():
    rng = np.random.default_rng(5)
    S, E, N = 4, 3, 2
    ring = new_ring(S, E, N)
    for k in ARRAYS:
        assert ring[k].shape[0] == S * E
    assert (ring["actions"] == 255).all() and (ring["masks_next"] == 0x10).all() and not ring["valid"].any()
    blk = _block(rng, 3, E, N)
    push_spec(ring, **blk)
    assert ring["state"].tolist() == [3, 0, 0, 0]
    assert (ring["actions"][9:] == 255).all() and (ring["obs_c"][9:] == 0).all()             # step 3 of the ring is untouched
    np.testing.assert_array_equal(ring["obs_c"][0:3], blk["obs0_compact"])
    np.testing.assert_array_equal(ring["obs_c"][3:6], blk["obs_compact"][0])
    reset = (blk["env_flags"] & 0x04) != 0
    assert reset.any() and not reset.all()
    for s in range(3):
        for e in range(E):
            at = s * E + e
            want = blk["final_compact"][s, e] if reset[s, e] else blk["obs_compact"][s, e]
            np.testing.assert_array_equal(ring["next_c"][at], want)
            np.testing.assert_array_equal(ring["masks_next"][at], np.full(N, 0x1F) if reset[s, e] else blk["masks_next"][s, e])
    assert set(np.unique(ring["done"][:9])) <= {0, 1} and set(np.unique(ring["valid"][:9])) <= {0, 4}
    blk2 = _block(rng, 2, E, N, with_final=False, with_masks=False)              # head 3: steps 3 and 0 of the ring
    push_spec(ring, **blk2)
    assert ring["state"][0] == 5
    np.testing.assert_array_equal(ring["actions"][9:12], blk2["actions"][0])
    np.testing.assert_array_equal(ring["actions"][0:3], blk2["actions"][1])
    np.testing.assert_array_equal(ring["next_c"][0:3], blk2["obs_compact"][1])  # no final_compact: never the terminal record
    assert (ring["masks_next"][0:3] == 0x1F).all() and (ring["masks_next"][9:12] == 0x1F).all()
    np.testing.assert_array_equal(ring["actions"][3:9], blk["actions"][1:3].reshape(6, N))   # the rest of block one stays


def test_rows_layout():
    consts = (6.0, 4.0, 5.0, 7.0)
    c = np.arange(24, dtype=np.float32).reshape(2, 3, 4) + 100
    rows = rows_spec(c, consts)
    assert rows.shape == (2, 3, 18)
    np.testing.assert_array_equal(rows[1, 2, :6], [c[1, 2, 0], c[1, 2, 1], 6, 4, 5, 7])
    np.testing.assert_array_equal(rows[1, 2, 6:10], c[1, 0])
    np.testing.assert_array_equal(rows[1, 2, 10:14], c[1, 1])
    np.testing.assert_array_equal(rows[1, 2, 14:18], [-1, -1, -1, -1])
    np.testing.assert_array_equal(rows[0, 0, 6:10], [-1, -1, -1, -1])


def test_fetch_copies_records_and_the_empty_one():
    rng = np.random.default_rng(9)
    S, E, N = 2, 3, 3
    ring = new_ring(S, E, N)
    push_spec(ring, **_block(rng, 1, E, N))
    consts = (6.0, 4.0, 5.0, 7.0)
    index = np.array([2, -1, 0, 6, 1 << 40, 4, 2], np.int64)
    mb = fetch_spec(ring, index, consts)
    empty = fetch_spec(new_ring(1, 1, N), np.array([0]), consts)
    for k in ("actions", "reward", "done", "valid", "masks_next"):
        np.testing.assert_array_equal(mb[k][0], ring[k][2])
        np.testing.assert_array_equal(mb[k][6], ring[k][2])
        for b in (1, 3, 4, 5):                                                    # outside the ring, and a slot not pushed yet
            np.testing.assert_array_equal(mb[k][b], empty[k][0])
    np.testing.assert_array_equal(mb["obs"][2], rows_spec(ring["obs_c"][0], consts))
    for b in (1, 3, 4, 5):
        np.testing.assert_array_equal(mb["next_obs"][b], rows_spec(np.zeros((N, 4), np.float32), consts))
    np.testing.assert_array_equal(mb["index"], index)


def test_draw_range_at_the_edges():
    assert (draw_spec(SEED, 0, 0, 100) == -1).all() and draw_one(SEED, 0, 7, 3) == -1
    assert (draw_spec(SEED, 1, 3, 500) == 0).all()
    F = (1 << 31) - 1
    big = draw_spec(SEED, F, 11, 4096)
    assert big.min() >= 0 and big.max() < F and big.max() > F // 2 and big.min() < F // 2 and len(set(big.tolist())) > 4000
    for d in (1 << 32, (1 << 32) + 5, (1 << 40) + 1, (1 << 63) - 1):
        got = draw_spec(SEED, 1000, d, 256)
        assert got.min() >= 0 and got.max() < 1000
        assert [draw_one(SEED, 1000, d, b) for b in range(256)] == got.tolist()
    # the high word of d is part of the key, and so is every other piece of it
    assert draw_spec(SEED, 1000, 5, 256).tolist() != draw_spec(SEED, 1000, (1 << 32) + 5, 256).tolist()
    assert draw_spec(SEED, 1000, 5, 256).tolist() != draw_spec(SEED, 1000, 6, 256).tolist()
    assert draw_spec(SEED, 1000, 5, 256).tolist() != draw_spec(SEED ^ 1, 1000, 5, 256).tolist()
    assert draw_spec(SEED, 1000, 5, 256)[:100].tolist() == draw_spec(SEED, 1000, 5, 100).tolist()     # b is the key, not B


def test_sample_index_advances_draws():
    ring = new_ring(4, 6, 2)
    assert (sample_index_spec(ring, SEED, 10) == -1).all() and ring["state"][1] == 1
    ring["state"][0] = 3
    a = sample_index_spec(ring, SEED, 64)
    assert a.max() < 18 and ring["state"][1] == 2
    np.testing.assert_array_equal(a, draw_spec(SEED, 18, 1, 64))
    ring["state"][0] = 9
    assert sample_index_spec(ring, SEED, 512).max() < 24 and ring["state"][1] == 3


def test_draw_statistics():
    """F = 1000, d = 0..48, B = 4096: 200 704 indices.  Every bucket within 5 binomial standard deviations of its mean, the
    chi-square statistic within 4 standard deviations of its 999 degrees of freedom."""
    F, B = 1000, 4096
    index = np.concatenate([draw_spec(SEED, F, d, B) for d in range(49)])
    n = index.size
    assert n == 200_704 and index.min() >= 0 and index.max() < F
    counts = np.bincount(index, minlength=F).astype(np.float64)
    p = 1.0 / F
    dev = np.abs(counts - n * p) / np.sqrt(n * p * (1 - p))
    chi2 = float(((counts - n * p) ** 2 / (n * p)).sum())
    z = (chi2 - (F - 1)) / np.sqrt(2.0 * (F - 1))
    print(f"largest bucket deviation {dev.max():.2f} sd, chi-square {chi2:.1f} at {F - 1} degrees of freedom, z = {z:.2f}")
    assert dev.max() <= 5.0
    assert abs(z) <= 4.0
