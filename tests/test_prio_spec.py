"""The NumPy / Python-integer spec of CCX_PRIO (tests/_prio_spec.py) checked against itself, against CCX_REPLAY's draw and
against the constants the library states (csrc/ccx_prio.h, csrc/ccx_kernels.h): the identity with the uniform draw when all
leaves are equal, the strata of a stratified draw, the statistics of 200 000 draws, the quantisation's edges, and the
accuracy of the fixed-point power against f64 ``pow`` (the number include/ccx.h and the README quote).  No GPU."""

import re
from pathlib import Path

import numpy as np
import pytest
from _prio_spec import (F32, K_PRIO_STREAM, LEAF_MAX, ONE_FIXED, POW_REL_BOUND, cumsum_spec, draw_spec, exp_spec, index_of_point, log_spec,
                        new_pstate, point_spec, quantise_spec, sample_spec, td_max_spec, update_spec, weight_spec, words_spec)
from _replay_spec import K_REPLAY_STREAM

import collectivecrossing_amd

CSRC = Path(collectivecrossing_amd.__file__).parent / "csrc"
SEED = 0x0123_4567_89AB_CDEF


def test_constants_are_the_headers():
    text = (CSRC / "ccx_prio.h").read_text()
    assert int(re.search(r"kStream = (0x[0-9A-Fa-f]+)u", text).group(1), 16) == K_PRIO_STREAM
    assert int(re.search(r"kOne = (\d+);", text).group(1)) == ONE_FIXED
    kernels = (CSRC / "ccx_kernels.h").read_text()
    assert int(re.search(r"kPrioStream = (0x[0-9A-Fa-f]+)u", kernels).group(1), 16) == K_PRIO_STREAM
    others = {int(v, 16) for v in re.findall(r"k\w+Stream = (0x[0-9A-Fa-f]+)u", kernels)} - {K_PRIO_STREAM}
    assert K_REPLAY_STREAM in others and len(others) == 5 and K_PRIO_STREAM not in others | {0}
    header = (CSRC.parent.parent / "include" / "ccx.h").read_text()
    assert f"{POW_REL_BOUND:.1e}".replace("e-0", "e-") in header and "0x7F4A7C15" in header


@pytest.mark.parametrize("F,c,tail", [(1, 1, 0), (7, 65536, 5), (1000, 3, 24), (96, LEAF_MAX, 0), (4096, 12345, 1)])
def test_equal_leaves_give_the_uniform_draw_of_the_same_words(F, c, tail):
    """floor(floor(x F c / 2^64) / c) == floor(x F / 2^64): the unstratified index is ccx_replay::index_of for the same words."""
    cum = cumsum_spec([c] * F + [0] * tail)
    w0, w1 = words_spec(SEED, 3, 2000)
    xs = [(int(h) << 32) | int(l) for h, l in zip(w0, w1)] + [0, (1 << 64) - 1, 1 << 63]
    for x in xs:
        assert index_of_point(cum, x) == (x * F) >> 64


@pytest.mark.parametrize("B", [1, 2, 63, 257, 4096, (1 << 31) - 1])
def test_a_stratified_point_lies_in_its_stratum(B):
    rng = np.random.default_rng(B % 1000)
    bs = sorted({0, B - 1, B // 2} | {int(v) for v in rng.integers(0, B, size=50)})
    for b in bs:
        for w0, w1 in [(0, 0), (0xFFFFFFFF, 0xFFFFFFFF)] + [tuple(int(v) for v in rng.integers(0, 1 << 32, size=2)) for _ in range(20)]:
            x = point_spec(w0, w1, b, B, True)
            assert (b << 64) // B <= x < -(-((b + 1) << 64) // B) and x < 1 << 64
            # the two 64-bit divisions of the header are the 128-bit one
            t1 = (b << 32) | w0
            q1, r1 = divmod(t1, B)
            q2 = ((r1 << 32) | w1) // B
            assert t1 < 1 << 64 and q1 < 1 << 32 and q2 < 1 << 32 and x == (q1 << 32) | q2
    assert point_spec(5, 7, 3, 9, False) == (5 << 32) | 7


def test_statistics_of_200000_unstratified_draws():
    """1000 leaves of mixed sizes (a factor of 100 between them, a few zeros): every bucket within 4 binomial standard deviations of leaf / T.
    A cap the chosen seed stays inside (checked with the spec alone), not a measurement."""
    rng = np.random.default_rng(11)
    leaf = np.concatenate([rng.integers(20_000, 40_000, 400), rng.integers(60_000, 140_000, 400), rng.integers(200_000, 2_000_000, 190),
                           np.zeros(10, np.int64)])                   # expected counts from 15 to 1500: the binomial cap means something
    rng.shuffle(leaf)
    cum = cumsum_spec(leaf)
    T, n = cum[-1], 200_000
    counts = np.zeros(1000, np.int64)
    for d in range(50):
        w0, w1 = words_spec(SEED, d, 4000)
        idx = [index_of_point(cum, (int(h) << 32) | int(l)) for h, l in zip(w0, w1)]
        counts += np.bincount(idx, minlength=1000)
    p = leaf.astype(np.float64) / T
    sd = np.sqrt(n * p * (1 - p))
    assert counts.sum() == n and (counts[leaf == 0] == 0).all()
    worst = np.max(np.abs(counts - n * p)[leaf > 0] / np.maximum(sd[leaf > 0], 1e-9))
    print(f"worst bucket: {worst:.2f} standard deviations")
    assert (np.abs(counts - n * p) <= 4 * sd + 1e-9).all()


def test_stratified_draws_cover_every_stratum_once():
    leaf = np.array([5, 0, 0, 1, 1 << 30, 7, 0, 3], np.int64)
    cum = cumsum_spec(leaf)
    idx = draw_spec(leaf, SEED, 0, 64, True)
    assert (np.diff(idx) >= 0).all() and (leaf[idx] > 0).all()          # strata are ordered, empty leaves are never drawn
    assert draw_spec(np.zeros(9, np.int64), SEED, 0, 5, True).tolist() == [-1] * 5
    assert index_of_point(cum, 0) == 0 and index_of_point(cum, (1 << 64) - 1) == 7


def test_quantisation_edges():
    q = quantise_spec
    assert q(F32(0.0), 0.6, 1e-6).tolist() == q(F32(1e-30), 0.6, 1e-6).tolist()                        # below 2^-16: clamped
    top = int(F32(float.fromhex("0x1.fffffep+30")))
    assert (1 << 31) * (1 - 1e-5) < int(q(F32(np.inf), 1.0, 1e-6)) == int(q(F32(4e4), 1.0, 1e-6)) <= top      # clamped to 2^15, then to < 2^31
    assert int(q(F32(np.inf), 1.0, 1e-6)) <= LEAF_MAX and int(q(F32(0.0), 1.0, 1e-6)) == 1            # 2^-16 * 2^16
    assert int(q(F32(123.0), 0.0, 1e-6)) == ONE_FIXED and int(q(F32(1.0), 1.0, F32(2.0 ** -30))) == ONE_FIXED
    assert (np.diff(q(np.linspace(0, 100, 2001).astype(F32), 0.6, 1e-6)) >= 0).all()                  # monotone
    td = np.array([[np.nan, -3.0], [np.nan, np.nan], [-np.inf, 2.0], [1e-45, -0.0]], F32)
    assert td_max_spec([td]).tolist() == [3.0, 0.0, np.inf, float(F32(1e-45))]
    leaf, ps = np.array([0, 9, 9, 9], np.int64), new_pstate()
    update_spec(leaf, ps, [0, 1, 1, 7, -1, 3], [np.array([[5.0], [1.0], [2.0], [9.0], [9.0], [np.nan]], F32)], 1.0, 1e-6)
    assert leaf.tolist() == [0, int(q(F32(2.0), 1.0, 1e-6)), 9, int(q(F32(0.0), 1.0, 1e-6))] and ps[0] == leaf[1]


def test_weights():
    w = weight_spec(100, np.array([100, 200, 0, LEAF_MAX]), 0.5)
    assert w[0] == 1.0 and w[2] == 0.0 and not np.signbit(w[2]) and abs(w[1] - 0.5 ** 0.5) < 1e-6
    assert (weight_spec(1, np.array([1, LEAF_MAX]), 0.0) == 1.0).all()
    assert weight_spec(1, np.array([LEAF_MAX]), 7.0)[0] == weight_spec(1, np.array([LEAF_MAX]), 1.0)[0]   # beta is clamped
    ps = new_pstate()
    out = sample_spec(np.array([0, 4, 2, 0, 8], np.int64), ps, SEED, 6, 3, 1.0, True)
    assert ps.tolist() == [ONE_FIXED, 1, 14, 2] and out["weights"].shape == (6, 3)
    assert set(out["index"].tolist()) <= {1, 2, 4} and (out["weights"][out["index"] == 2] == 1.0).all()


def test_power_accuracy_against_f64():
    """max relative error of p = exp_spec(alpha * log_spec(x)) against f64 pow on the same f32 x, x in [2^-31, 2^15]:
    printed, and asserted below the bound the header quotes (the measured maximum doubled)."""
    rng = np.random.default_rng(5)
    x = np.concatenate([np.exp2(rng.uniform(-31, 15, 400_000)), np.exp2(np.arange(-31, 16)), np.exp2(np.arange(-31, 15)) * (1 + 2.0 ** -23),
                        np.exp2(np.arange(-30, 16)) * (1 - 2.0 ** -24), np.linspace(0.5, 2.0, 100_001)]).astype(F32)
    worst = 0.0
    for alpha in (0.3, 0.6, 1.0):
        p = exp_spec(F32(alpha) * log_spec(x)).astype(np.float64)
        ref = np.power(x.astype(np.float64), np.float64(F32(alpha)))
        rel = float(np.max(np.abs(p - ref) / ref))
        print(f"alpha {alpha}: max relative error {rel:.3e}")
        worst = max(worst, rel)
    print(f"maximum {worst:.3e}; doubled {2 * worst:.3e}")
    assert worst <= POW_REL_BOUND and POW_REL_BOUND <= 2.2 * worst
