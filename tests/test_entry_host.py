"""The host helpers of csrc/ccx_entry.h -- the header every `extern "C"` entry takes its alignment test and its step from
run-time flags to template parameters from -- compiled with a plain host C++17 compiler (no HIP include) and driven through
ctypes: with_flags runs its functor exactly once with exactly the given combination, for 1 to 4 flags; misaligned sees every
offset below the alignment at every position of a pack, passes aligned pointers, and ignores a null.  No GPU."""

import ctypes as C
import itertools
import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "collectivecrossing_amd" / "csrc"
BASE = 0x7F12_3456_7000                                                    # a 4096-byte aligned address (never dereferenced)


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
    so = tmp_path_factory.mktemp("entry_host") / "libentry_host.so"
    subprocess.run([cxx, "-std=c++17", "-O2", "-Wall", "-Werror", "-fPIC", "-shared", f"-I{CSRC}",
                    str(Path(__file__).with_name("entry_host.cpp")), "-o", str(so)], check=True)
    lib = C.CDLL(str(so))
    lib.host_with_flags.restype = None
    lib.host_with_flags.argtypes = [C.c_int, C.c_uint, C.POINTER(C.c_int)]
    lib.host_with_flags_excluding_both_false.restype = C.c_int
    lib.host_with_flags_excluding_both_false.argtypes = [C.c_int, C.c_int]
    lib.host_misaligned1.restype = C.c_int
    lib.host_misaligned1.argtypes = [C.c_uint, C.c_size_t]
    lib.host_misaligned3.restype = C.c_int
    lib.host_misaligned3.argtypes = [C.c_uint] + [C.c_size_t] * 3
    return lib


@pytest.mark.parametrize("n", [1, 2, 3, 4])
def test_with_flags_runs_once_with_the_given_combination(host, n):
    for bits in range(1 << n):
        out = (C.c_int * 4)(-7, -7, -7, -7)
        host.host_with_flags(n, bits, out)
        assert list(out) == [1, bits, n, 10 + n], (n, bits)                # one call, that combination, n arguments, f's value


def test_with_flags_hands_the_flags_over_as_types(host):
    for a, b in itertools.product((0, 1), repeat=2):
        assert host.host_with_flags_excluding_both_false(a, b) == (1 if (a or b) else 0), (a, b)


@pytest.mark.parametrize("align", [4, 8, 16])
def test_misaligned_sees_every_offset_at_every_position(host, align):
    assert host.host_misaligned1(align, BASE) == 0
    assert host.host_misaligned3(align, BASE, BASE + align, BASE + 5 * align) == 0
    for off in range(1, align):
        assert host.host_misaligned1(align, BASE + off) == 1, off
        for pos in range(3):
            ptrs = [BASE, BASE + align, BASE + 5 * align]
            ptrs[pos] += off
            assert host.host_misaligned3(align, *ptrs) == 1, (off, pos)
            # the other two null: the one misaligned pointer is still seen
            alone = [0, 0, 0]
            alone[pos] = ptrs[pos]
            assert host.host_misaligned3(align, *alone) == 1, (off, pos)


@pytest.mark.parametrize("align", [4, 8, 16])
def test_a_null_among_the_pointers_changes_nothing(host, align):
    assert host.host_misaligned1(align, 0) == 0
    assert host.host_misaligned3(align, 0, 0, 0) == 0
    for nulls in itertools.product((False, True), repeat=3):
        aligned = [0 if z else BASE + (k + 1) * align for k, z in enumerate(nulls)]
        assert host.host_misaligned3(align, *aligned) == 0, nulls
        for pos in range(3):
            if nulls[pos]:
                continue
            bad = list(aligned)
            bad[pos] += align // 2                                         # misaligned at `align`, whatever stands beside it
            assert host.host_misaligned3(align, *bad) == 1, (nulls, pos)
    # an alignment the pointer does meet is not mistaken for one it does not
    assert host.host_misaligned1(4, BASE + 4) == 0 and host.host_misaligned1(8, BASE + 4) == 1
    assert host.host_misaligned1(8, BASE + 8) == 0 and host.host_misaligned1(16, BASE + 8) == 1
