"""The rules of csrc/ccx_dueling.h -- the very source the kernels of ccx_dueling.hip, ccx_mlp.hip and ccx_sides.hip inline --
compiled for the host (-O2 -ffp-contract=off) and run against the NumPy spec (tests/_dueling_spec.py) bit for bit, on random
rows and on rows with +-0, +-inf, NaN and subnormals.  The same source with its own ``main``, built with
-fsanitize=address,undefined, runs as a program of its own.  No GPU."""

import ctypes as C
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest
from _dueling_spec import dueling_backward_spec, dueling_spec, make_dueling_rows
from _mlp_spec import bits32c

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "collectivecrossing_amd" / "csrc"
SOURCE = Path(__file__).with_name("dueling_host_rule.cpp")


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
    so = tmp_path_factory.mktemp("dueling_host_rule") / "libdueling_host_rule.so"
    subprocess.run([cxx, "-std=c++17", "-O2", "-ffp-contract=off", "-fPIC", "-shared", f"-I{CSRC}", str(SOURCE), "-o", str(so)],
                   check=True)
    lib = C.CDLL(str(so))
    lib.host_dueling_forward.restype = lib.host_dueling_backward.restype = None
    return lib


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def _both(host, va, g):
    M = len(va)
    q, gva = np.full((M, 5), 7.0, np.float32), np.full((M, 6), 7.0, np.float32)
    host.host_dueling_forward(C.c_longlong(M), _p(va), _p(q))
    host.host_dueling_backward(C.c_longlong(M), _p(g), _p(gva))
    return q, gva


@pytest.mark.parametrize("M", (1, 63, 1000, 20_000))
def test_random_rows_equal_the_spec(host, M):
    va, g = make_dueling_rows(M, seed=M)
    q, gva = _both(host, va, g)
    np.testing.assert_array_equal(bits32c(q), bits32c(dueling_spec(va)))
    np.testing.assert_array_equal(bits32c(gva), bits32c(dueling_backward_spec(g)))
    assert np.isfinite(q).all() and np.isfinite(gva).all()


def test_special_values_equal_the_spec(host):
    va, g = make_dueling_rows(200, seed=5, special=True)
    q, gva = _both(host, va, g)
    want_q, want_g = dueling_spec(va), dueling_backward_spec(g)
    np.testing.assert_array_equal(bits32c(q), bits32c(want_q))           # (NaN payloads canonicalised on both sides)
    np.testing.assert_array_equal(bits32c(gva), bits32c(want_g))
    assert np.isnan(q).any() and np.isinf(q).any() and np.isnan(gva).any() and np.isinf(gva).any()
    zero = ~g.view(np.uint32).any(-1)
    assert zero.any() and not gva[zero].view(np.uint32).any()            # five +0.0 in, six +0.0 out
    tiny = np.abs(gva) < np.float32(1.1754944e-38)
    assert (tiny & (gva != 0)).any()                                     # subnormals are kept


def test_the_rule_under_address_and_undefined_behaviour_sanitizers(tmp_path):
    """The same source as a program of its own (its own ``main``), built with the sanitizers and run as a subprocess: every
    array has exactly the rows' size, so an element outside it ends the program."""
    cxx = _compiler()
    if cxx is None:
        pytest.skip("no host C++ compiler (c++, clang++ or ROCm's clang++)")
    exe = tmp_path / "dueling_host_rule_san"
    plain = [cxx, "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-DDUELING_HOST_MAIN", f"-I{CSRC}", str(SOURCE), "-o", str(exe)]
    subprocess.run(plain, check=True)                                    # (the program itself compiles: a failure below is the runtime's)
    build = subprocess.run(plain + ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"], capture_output=True, text=True)
    if build.returncode:
        pytest.skip("the compiler has no sanitizer runtime: " + build.stderr.strip()[-200:])
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    print(run.stdout.strip())
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-4000:]
    assert "rows combined" in run.stdout
