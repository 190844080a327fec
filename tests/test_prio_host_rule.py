"""The rules of csrc/ccx_prio.h -- the very source the kernels of ccx_prio.hip inline -- compiled for the host (-O2
-ffp-contract=off) and run against the spec (tests/_prio_spec.py): the descent at a small fan-out (4) AND the shipped one, over
leaf arrays with empty stretches, whole empty blocks, a single non-zero leaf and all leaves 2^31 - 1, at every exact boundary
(u = C[i] - 1, u = C[i], u = T - 1) as exact integers -- the deep levels a GPU test cannot afford are reached here through the
small fan-out --; the point of a draw; and the quantisation and the weight bit for bit, NaN / inf / 0 / denormals included.
No GPU."""

import ctypes as C
import shutil
import subprocess
from bisect import bisect_right
from pathlib import Path

import numpy as np
import pytest
from _prio_spec import F32, LEAF_MAX, cumsum_spec, point_spec, quantise_spec, td_max_spec, weight_spec

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "collectivecrossing_amd" / "csrc"


def _compiler():
    for name in ("c++", "clang++"):
        if shutil.which(name):
            return shutil.which(name)
    rocm = Path("/opt/rocm/llvm/bin/clang++")
    return str(rocm) if rocm.exists() else None


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    cxx = _compiler()
    if cxx is None:
        pytest.skip("no host C++ compiler (c++, clang++ or ROCm's clang++)")
    so = tmp_path_factory.mktemp("prio_host_rule") / "libprio_host_rule.so"
    subprocess.run([cxx, "-std=c++17", "-O2", "-ffp-contract=off", "-fPIC", "-shared", f"-I{CSRC}",
                    str(Path(__file__).with_name("prio_host_rule.cpp")), "-o", str(so)], check=True)
    lib = C.CDLL(str(so))
    for name in ("host_prio_shape", "host_prio_quantise", "host_prio_weight"):
        getattr(lib, name).restype = None
    lib.host_prio_descend.restype = C.c_ulonglong
    lib.host_prio_point.restype = C.c_ulonglong
    lib.host_prio_tree_words.restype = C.c_longlong
    lib.host_prio_fan.restype = C.c_int
    return lib


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def _shape(host, R, fan):
    out = np.zeros(19, np.int64)
    host.host_prio_shape(C.c_longlong(R), C.c_int(fan), _p(out))
    return dict(top=int(out[0]), launches=int(out[1]), nodes=int(out[2]), n=out[3:11].tolist(), off=out[11:19].tolist())


def test_the_shape_of_the_tree(host):
    fan = host.host_prio_fan()
    assert fan == 16
    for f in (4, fan):
        for R in (1, 2, f - 1, f, f + 1, f * f - 1, f * f, f * f + 1, f ** 4 - 1, f ** 4, f ** 4 + 1, f ** 4 + f * f + 1, 100_003):
            s = _shape(host, R, f)
            n = [R]
            for _ in range(s["top"]):
                n.append(-(-n[-1] // f))
            assert s["n"][:s["top"] + 1] == n and s["top"] == 2 * s["launches"] + 1 and s["top"] <= 7
            assert s["off"][1:s["top"] + 1] == np.concatenate([[0], np.cumsum(n[1:-1])]).tolist() and s["nodes"] == sum(n[1:])
            assert n[s["top"] - 1] <= f * f or s["launches"] == 3           # what the final workgroup takes
            assert s["launches"] == 1 or n[2 * s["launches"] - 2] > f * f   # no launch more than needed
    s = _shape(host, (1 << 31) - 1, fan)
    assert s["top"] == 7 and s["n"][6] <= 256 and host.host_prio_tree_words(C.c_longlong((1 << 31) - 1)) == 2 * s["nodes"]
    assert host.host_prio_tree_words(C.c_longlong(0)) == 0 and host.host_prio_tree_words(C.c_longlong(1)) == 2 * 3


def _patterns(R, rng):
    yield "all equal", np.full(R, 65536, np.int32)
    one = np.zeros(R, np.int32)
    one[R // 3] = 7
    yield "one non-zero", one
    yield "all 2^31 - 1", np.full(R, LEAF_MAX, np.int32)
    mixed = rng.integers(1, 1 << 20, R).astype(np.int32)
    mixed[rng.random(R) < 0.3] = 0                                       # empty stretches
    for a in range(0, R, 64):                                            # whole empty blocks of 16 (both fan-outs)
        mixed[a:a + 16] = 0
    mixed[R - 1] = 0 if R > 40 else mixed[R - 1]
    yield "empty stretches and blocks", mixed
    last = np.zeros(R, np.int32)
    last[R - 1] = LEAF_MAX
    yield "only the last", last


@pytest.mark.parametrize("fan", [4, 16])
@pytest.mark.parametrize("R", [1, 2, 3, 4, 5, 15, 16, 17, 63, 64, 65, 255, 256, 257, 1023, 1025, 4097, 65535 + 258])
def test_descent_at_every_boundary(host, fan, R):
    rng = np.random.default_rng(R)
    for what, leaf in _patterns(R, rng):
        cum = cumsum_spec(leaf)
        T = cum[-1]
        if T == 0:
            continue
        us = sorted({u for c in cum for u in (c - 1, c) if 0 <= u < T} | {T - 1, 0})
        if len(us) > 6000:                                               # (the large R: every boundary of a slice, and the ends)
            us = sorted(set(us[:1500] + us[-1500:] + us[::len(us) // 1500]))
        u = np.array(us, np.uint64)
        got = np.full(len(us), -7, np.int64)
        mn = C.c_longlong(-7)
        gotT = host.host_prio_descend(_p(leaf), C.c_longlong(R), C.c_int(fan), _p(u), C.c_longlong(len(us)), _p(got), C.byref(mn))
        assert gotT == T and mn.value == min(int(v) for v in leaf if v), what
        want = np.array([bisect_right(cum, x) for x in us], np.int64)
        np.testing.assert_array_equal(got, want, err_msg=f"{what} R {R} fan {fan}")
        assert (leaf[got] > 0).all()


def test_an_empty_tree_draws_nothing(host):
    leaf, u, got, mn = np.zeros(300, np.int32), np.array([0, 5], np.uint64), np.full(2, -7, np.int64), C.c_longlong(-7)
    assert host.host_prio_descend(_p(leaf), C.c_longlong(300), C.c_int(16), _p(u), C.c_longlong(2), _p(got), C.byref(mn)) == 0
    assert got.tolist() == [-1, -1] and mn.value == 0


def test_point_equals_the_spec(host):
    rng = np.random.default_rng(2)
    for B in (1, 2, 63, 64, 257, 4096, (1 << 31) - 1):
        for b in sorted({0, B - 1, B // 2} | {int(v) for v in rng.integers(0, B, size=30)}):
            for w0, w1 in [(0, 0), (0xFFFFFFFF, 0xFFFFFFFF)] + [tuple(int(v) for v in rng.integers(0, 1 << 32, size=2)) for _ in range(10)]:
                for strat in (0, 1):
                    got = host.host_prio_point(C.c_uint32(w0), C.c_uint32(w1), C.c_ulonglong(b), C.c_ulonglong(B), C.c_int(strat))
                    assert got == point_spec(w0, w1, b, B, bool(strat)), (B, b, w0, w1, strat)


def _td_cases(rng, B, N):
    td = (rng.standard_normal((B, N)) * np.exp2(rng.integers(-30, 18, (B, 1)))).astype(F32)
    special = np.array([np.nan, np.inf, -np.inf, 0.0, -0.0, 1e-45, -1e-40, 2.0 ** -16, 2.0 ** 15, 3.4e38, 2.0 ** -17, 1.0], F32)
    td[:len(special), 0] = special
    td[:len(special), 1:] = 0.0
    td[len(special)] = np.nan                                            # a whole row of NaNs
    return td


@pytest.mark.parametrize("alpha,eps", [(0.0, 1e-6), (0.6, 1e-6), (1.0, 1e-6), (0.3, 1e-3), (1.0, 2.0 ** -40), (0.6, 1e30)])
@pytest.mark.parametrize("count", [1, 3])
def test_quantisation_bit_for_bit(host, alpha, eps, count):
    rng = np.random.default_rng(int(alpha * 10) + count)
    B, N = 3000, 3
    tds = [_td_cases(rng, B, N) for _ in range(count)]
    table = (C.c_void_p * count)(*(t.ctypes.data for t in tds))
    got = np.full(B, -7, np.int32)
    host.host_prio_quantise(table, C.c_int(count), C.c_longlong(B), C.c_int(N), C.c_float(alpha), C.c_float(eps), _p(got))
    want = quantise_spec(td_max_spec(tds), alpha, eps)
    np.testing.assert_array_equal(got.astype(np.int64), want)
    assert got.min() >= 1 and got.max() <= LEAF_MAX


@pytest.mark.parametrize("beta", [0.0, 0.4, 1.0, -3.0, 7.0])
def test_weight_bit_for_bit(host, beta):
    rng = np.random.default_rng(7)
    for min_leaf in (1, 65536, 12345, LEAF_MAX):
        ld = np.concatenate([[min_leaf, 0, LEAF_MAX, min_leaf + 1 if min_leaf < LEAF_MAX else LEAF_MAX],
                             rng.integers(min_leaf, LEAF_MAX, 2000, endpoint=True)]).astype(np.int32)
        got = np.full(len(ld), -7, F32)
        host.host_prio_weight(C.c_longlong(min_leaf), _p(ld), C.c_longlong(len(ld)), C.c_float(beta), _p(got))
        want = weight_spec(min_leaf, ld, beta)
        np.testing.assert_array_equal(got.view(np.uint32), want.view(np.uint32))
        assert got[0] == 1.0 and got[1] == 0.0 and not np.signbit(got[1])
