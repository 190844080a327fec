"""The rules of csrc/ccx_replay.h -- the very source the kernels of ccx_replay.hip inline -- compiled for the host (-O2
-ffp-contract=off) and run against the spec (tests/_replay_spec.py) as exact integers: the slot map for heads around multiples
of S and blocks that wrap inside themselves, the number of filled records, the draw at the edges of its domain (F = 1, F =
2^31 - 1, d >= 2^32, F = 0) and over the statistics test's launches, the high half of the 128-bit product, and the empty
record.  No GPU."""

import ctypes as C
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest
from _replay_spec import EMPTY_ACTION, EMPTY_MASKS, MASKS_ALL, draw_spec, filled_spec, slot_spec

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "collectivecrossing_amd" / "csrc"
SEED = 0x0123_4567_89AB_CDEF


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
    so = tmp_path_factory.mktemp("replay_host_rule") / "libreplay_host_rule.so"
    subprocess.run([cxx, "-std=c++17", "-O2", "-ffp-contract=off", "-fPIC", "-shared", f"-I{CSRC}",
                    str(Path(__file__).with_name("replay_host_rule.cpp")), "-o", str(so)], check=True)
    lib = C.CDLL(str(so))
    for name in ("host_replay_slots", "host_replay_draw", "host_replay_empty"):
        getattr(lib, name).restype = None
    lib.host_replay_filled.restype = C.c_ulonglong
    lib.host_replay_mulhi64.restype = C.c_ulonglong
    lib.host_replay_in_ring.restype = C.c_int
    return lib


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


@pytest.mark.parametrize("S,E", [(4, 24), (1, 5), (7, 3), (64, 2)])
def test_slot_map_equals_the_spec(host, S, E):
    heads = sorted({h for m in (0, 1, 2, 5, 1000) for h in (m * S - 1, m * S, m * S + 1, m * S + S // 2) if h >= 0} | {(1 << 40) + 3})
    for head in heads:
        for K in sorted({1, max(1, S // 2), max(1, S - 1), S}):            # K > S - head mod S: the block wraps inside itself
            got = np.full((K, E), -7, np.int64)
            host.host_replay_slots(C.c_longlong(head), C.c_longlong(K), C.c_longlong(S), C.c_longlong(E), _p(got))
            want = np.array([[slot_spec(head, s, S, E, e) for e in range(E)] for s in range(K)], np.int64)
            np.testing.assert_array_equal(got, want, err_msg=f"head {head} K {K}")
            assert len(set(got.reshape(-1).tolist())) == K * E and got.min() >= 0 and got.max() < S * E
        assert host.host_replay_filled(C.c_longlong(head), C.c_longlong(S), C.c_longlong(E)) == filled_spec(head, S, E)


def _draw(host, F, d, B, seed=SEED):
    got = np.full(B, -7, np.int64)
    host.host_replay_draw(C.c_ulonglong(seed), C.c_ulonglong(F), C.c_ulonglong(d), C.c_longlong(B), _p(got))
    return got


@pytest.mark.parametrize("F,d", [(0, 0), (0, 9), (1, 3), ((1 << 31) - 1, 11), (1000, 1 << 32), (1000, (1 << 32) + 5),
                                 (1000, (1 << 40) + 1), (1000, (1 << 63) - 1), (96, 0), (24, 1)])
def test_draw_equals_the_spec_at_the_edges(host, F, d):
    got = _draw(host, F, d, 4096)
    np.testing.assert_array_equal(got, draw_spec(SEED, F, d, 4096))
    assert (got == -1).all() if F == 0 else (got.min() >= 0 and got.max() < F)


def test_draw_equals_the_spec_over_the_statistics_launches(host):
    for d in range(49):
        np.testing.assert_array_equal(_draw(host, 1000, d, 4096), draw_spec(SEED, 1000, d, 4096), err_msg=f"d {d}")
    np.testing.assert_array_equal(_draw(host, 1000, 5, 300, seed=77), draw_spec(77, 1000, 5, 300))


def test_mulhi64_is_the_high_half(host):
    rng = np.random.default_rng(3)
    cases = [(0, 0), (1, 1), ((1 << 64) - 1, (1 << 64) - 1), ((1 << 64) - 1, 1), ((1 << 63), 2), ((1 << 32) - 1, (1 << 32) + 1),
             ((1 << 64) - 1, (1 << 31) - 1)]
    cases += [(int(a), int(b)) for a, b in rng.integers(0, 1 << 64, size=(500, 2), dtype=np.uint64)]
    cases += [(int(a), int(b)) for a, b in zip(rng.integers(0, 1 << 64, size=500, dtype=np.uint64), rng.integers(0, 1 << 31, size=500))]
    for a, b in cases:
        assert host.host_replay_mulhi64(C.c_ulonglong(a), C.c_ulonglong(b)) == (a * b) >> 64, (a, b)


def test_in_ring_and_the_empty_record(host):
    R = 96
    for i, want in ((-1, 0), (0, 1), (R - 1, 1), (R, 0), (1 << 40, 0), (-(1 << 62), 0)):
        assert host.host_replay_in_ring(C.c_longlong(i), C.c_longlong(R)) == want, i
    out = np.full(7, -7, np.int64)
    host.host_replay_empty(_p(out))
    assert out.tolist() == [EMPTY_ACTION, 0, 0, EMPTY_MASKS, MASKS_ALL, 4, 0]       # (reward: the bits of +0.0)
