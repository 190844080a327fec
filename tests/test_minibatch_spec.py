"""The spec of CCX_MINIBATCH (tests/_minibatch_spec.py) against an independent statement of the rule of include/ccx.h: the
network one position at a time in Python integers (and its inverse, rounds 5 .. 0), bijections, widths, the cover of an epoch
by its draws with the roll-over into the next, and the uniformity of pi_c(p) over 20 000 epochs (deterministic: the inputs
are fixed).  No GPU."""

import numpy as np
import pytest
from _minibatch_spec import K_MINIBATCH_STREAM, M_LIST, advance_spec, draw_spec, next_spec, perm_spec, rounds_spec, split_spec
from _sample_spec import random_word, random_word_int

SEED = 2024


def _word(seed, epoch, R, r):
    return random_word_int(seed, K_MINIBATCH_STREAM, R, epoch & 0xFFFFFFFF, (epoch >> 32) & 0xFFFFFFFF, r)


def rounds_int(x: int, M: int, seed: int, epoch: int) -> int:
    """The six rounds as include/ccx.h writes them, in Python integers."""
    w = 2
    while 2 ** w < M:
        w += 1
    a = w // 2
    b = w - a
    L, R, wl = x >> b, x & (2 ** b - 1), a
    for r in range(6):
        L, R = R, L ^ (_word(seed, epoch, R, r) & (2 ** wl - 1))
        wl = w - wl
    assert wl == a and L < 2 ** a and R < 2 ** b
    return L * 2 ** b + R


def rounds_back_int(y: int, M: int, seed: int, epoch: int) -> int:
    """Rounds 5 .. 0 undone."""
    w = 2
    while 2 ** w < M:
        w += 1
    a = w // 2
    b = w - a
    L, R, wl = y >> b, y & (2 ** b - 1), a
    for r in range(5, -1, -1):
        wl = w - wl                                                      # the width of L before round r
        L, R = R ^ (_word(seed, epoch, L, r) & (2 ** wl - 1)), L
    return L * 2 ** b + R


def pi_int(p: int, M: int, seed: int, epoch: int):
    x, steps = p, 0
    while True:
        x, steps = rounds_int(x, M, seed, epoch), steps + 1
        if x < M:
            return x, steps


@pytest.mark.parametrize("M", M_LIST)
def test_bijection(M):
    for epoch in (0, 1):
        pi, steps = perm_spec(M, SEED, epoch, want_steps=True)
        assert pi.dtype == np.int64 and np.array_equal(np.sort(pi), np.arange(M)), (M, epoch)
        assert steps.min() >= 1
    print(f"M {M}: longest walk {int(steps.max())}")


@pytest.mark.parametrize("M", [m for m in M_LIST if m <= 1025])
def test_array_spec_equals_the_integer_statement(M):
    for epoch in (0, 3, 2 ** 32, 2 ** 40 + 7):
        pi, steps = perm_spec(M, SEED, epoch, want_steps=True)
        pos = range(M) if M <= 65 else list(range(0, M, max(1, M // 37))) + [M - 1]
        for p in pos:
            assert (int(pi[p]), int(steps[p])) == pi_int(p, M, SEED, epoch), (M, epoch, p)


@pytest.mark.parametrize("M", [1, 2, 5, 15, 16, 17, 257, 1000])
def test_inverse_network_recovers_the_position(M):
    w, _, _ = split_spec(M)
    for epoch in (0, 2 ** 40 + 7):
        for x in range(min(2 ** w, 300)):
            y = rounds_int(x, M, SEED, epoch)
            assert 0 <= y < 2 ** w and rounds_back_int(y, M, SEED, epoch) == x, (M, epoch, x)
        ys = rounds_spec(np.arange(2 ** w), M, SEED, epoch)
        assert np.array_equal(np.sort(ys), np.arange(2 ** w))              # each pass of the rounds is a bijection of [0, 2^w)


def test_two_epochs_and_two_seeds_differ():
    for M in (15, 16, 1000):
        a, b, c = perm_spec(M, SEED, 0), perm_spec(M, SEED, 1), perm_spec(M, SEED + 1, 0)
        assert not np.array_equal(a, b) and not np.array_equal(a, c)
        assert not np.array_equal(perm_spec(M, SEED, 2 ** 32), a)        # the high half of the epoch is a key as well


@pytest.mark.parametrize("M", M_LIST)
def test_width(M):
    w, a, b = split_spec(M)
    assert w >= 2 and a == w // 2 and a + b == w and 2 ** w >= M
    if M > 2:
        assert 2 ** (w - 1) < M <= 2 ** w


@pytest.mark.parametrize("M,B", [(15, 4), (15, 15), (15, 16), (16, 4), (1, 1), (1, 3)])
def test_a_cycle_of_draws_covers_every_record_once(M, B):
    state = np.zeros(4, np.int64)
    per_epoch = -(-M // B)
    for epoch in range(3):                                               # (the roll-over into the next epoch included)
        seen = []
        for d in range(per_epoch):
            assert state.tolist() == [epoch, d * B, 0, 0]
            index = next_spec(M, B, SEED, state)
            assert index.shape == (B,)
            pad = index < 0
            assert (index[pad] == -1).all()
            if d < per_epoch - 1:
                assert not pad.any()
            else:
                assert pad.sum() == per_epoch * B - M and not pad[:B - pad.sum()].any()      # only at the end of the last draw
            seen += index[~pad].tolist()
        assert sorted(seen) == list(range(M)) and seen == perm_spec(M, SEED, epoch).tolist()
        assert state.tolist() == [epoch + 1, 0, 0, 0]


def test_state_outside_its_range():
    for cursor in (-1, -2 ** 63, 15, 16, 2 ** 62, 2 ** 63 - 1):
        state = np.array([7, cursor, 0, 0], np.int64)
        assert (draw_spec(15, 4, SEED, state) == -1).all(), cursor
        advance_spec(state, 4, 15)
        assert state.tolist() == [8, 0, 0, 0]
    state = np.array([-1, 0, 0, 0], np.int64)                            # epoch 2^64 - 1 wraps to 0
    assert np.array_equal(draw_spec(15, 15, SEED, state), perm_spec(15, SEED, 2 ** 64 - 1))
    advance_spec(state, 15, 15)
    assert state.tolist() == [0, 0, 0, 0]


def _pi_over_epochs(M: int, p: int, epochs: np.ndarray) -> np.ndarray:
    """pi_c(p) for an array of epochs c < 2^32, the walk masked per epoch."""
    w, a, b = split_spec(M)
    x = np.full(len(epochs), p, np.uint32)
    walking = np.ones(len(epochs), bool)
    while walking.any():
        c = epochs[walking]
        L, R, wl = x[walking] >> np.uint32(b), x[walking] & np.uint32(2 ** b - 1), a
        for r in range(6):
            L, R = R, L ^ (random_word(SEED, K_MINIBATCH_STREAM, R, c, 0, r) & np.uint32(2 ** wl - 1))
            wl = w - wl
        x[walking] = (L << np.uint32(b)) | R
        walking &= x >= M
    return x.astype(np.int64)


@pytest.mark.parametrize("M,quantile", [(15, 36.12), (60, 98.32)])
def test_uniformity_over_epochs(M, quantile):
    """Chi-square of the histogram of pi_c(p) over epochs 0 .. 19 999 at p = 0, M / 2, M - 1, against the 0.999 quantile for
    M - 1 degrees of freedom."""
    epochs = np.arange(20_000, dtype=np.int64)
    for p in (0, M // 2, M - 1):
        got = _pi_over_epochs(M, p, epochs)
        assert np.array_equal(got[:5], [perm_spec(M, SEED, int(c))[p] for c in range(5)])
        hist = np.bincount(got, minlength=M)
        expected = len(epochs) / M
        chi2 = float(((hist - expected) ** 2 / expected).sum())
        print(f"M {M} p {p}: chi-square {chi2:.1f} (0.999 quantile {quantile})")
        assert hist.sum() == len(epochs) and chi2 < quantile, (M, p, chi2)
