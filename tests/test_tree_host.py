"""csrc/ccx_tree.h -- the one statement of the fixed f64 reduction tree -- compiled for the host BY ITSELF (-O2
-ffp-contract=off, tests/tree_host.cpp includes nothing else) and run against the NumPy spec's two spellings of the tree
(tests/_ppo_loss_spec.py: tree_sum, the array form, and tree_sum_loop, one addition at a time) bit for bit.  The sizes sit at
the edges of a group (64), of a block (256), of the final wave's 64 places (16384 terms = 64 partials) and in the second
round of a final place (16385, 16389: 65 partials).  No GPU."""

import ctypes as C
import re
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest
from _ppo_loss_spec import block_partials, final_sum, tree_sum, tree_sum_loop

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "collectivecrossing_amd" / "csrc"
SOURCE = Path(__file__).with_name("tree_host.cpp")
ROWS = (1, 63, 64, 65, 255, 256, 257, 16384, 16385, 16389)


def _compiler():
    for name in ("c++", "clang++"):
        if shutil.which(name):
            return shutil.which(name)
    rocm = Path("/opt/rocm/llvm/bin/clang++")
    return str(rocm) if rocm.exists() else None


@pytest.fixture(scope="module")
def cxx():
    found = _compiler()
    if found is None:
        pytest.skip("no host C++ compiler (c++, clang++ or ROCm's clang++)")
    return found


@pytest.fixture(scope="module")
def host(cxx, tmp_path_factory):
    so = tmp_path_factory.mktemp("tree_host") / "libtree_host.so"
    subprocess.run([cxx, "-std=c++17", "-O2", "-ffp-contract=off", "-fPIC", "-shared", f"-I{CSRC}", str(SOURCE), "-o", str(so)],
                   check=True)
    lib = C.CDLL(str(so))
    for name in ("tree_sum_host", "tree_block_host", "tree_final_host"):
        getattr(lib, name).restype = C.c_double
    lib.tree_blocks_of.restype = C.c_longlong
    return lib


def _terms(M):
    """Mixed sign, magnitudes over 2^-29 .. 2^29: almost every addition rounds, so another order gives other bits."""
    rng = np.random.default_rng(1000 + M)
    return rng.standard_normal(M) * np.exp(rng.uniform(-20, 20, M))


def _bits(x):
    return np.asarray(x, np.float64).view(np.uint64)


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def test_the_header_pulls_in_no_rule(cxx):
    """The project headers the unit depends on are ccx_tree.h alone, and its own includes are the fixed-width types and, for the
    device compiler only, the runtime."""
    out = subprocess.run([cxx, "-std=c++17", f"-I{CSRC}", "-MM", str(SOURCE)], check=True, capture_output=True, text=True).stdout
    deps = {Path(d).name for d in out.replace("\\\n", " ").split(":", 1)[1].split()}
    assert deps == {"tree_host.cpp", "ccx_tree.h"}
    includes = re.findall(r'^\s*#\s*include\s*([<"][^>"]+[>"])', (CSRC / "ccx_tree.h").read_text(), re.M)
    assert sorted(includes) == ["<hip/hip_runtime.h>", "<stdint.h>"]


@pytest.mark.parametrize("M", ROWS)
def test_sum_host_equals_both_spellings_of_the_spec(host, M):
    terms = _terms(M)
    got = host.tree_sum_host(C.c_longlong(M), _p(terms))
    assert _bits(got) == _bits(tree_sum(terms))
    assert _bits(got) == _bits(tree_sum_loop(terms))
    assert host.tree_blocks_of(C.c_longlong(M)) == -(-M // 256)


@pytest.mark.parametrize("M", ROWS)
def test_the_pieces_compose_to_the_sum(host, M):
    """block_host per block (the last one short: the missing terms are +0.0), then final_host, is sum_host and the spec's."""
    terms = _terms(M)
    B = -(-M // 256)
    P = np.array([host.tree_block_host(C.c_int(min(256, M - 256 * b)), _p(terms[256 * b:])) for b in range(B)], np.float64)
    np.testing.assert_array_equal(_bits(P), _bits(block_partials(terms)))
    got = host.tree_final_host(C.c_longlong(B), _p(P))
    assert _bits(got) == _bits(final_sum(P)) == _bits(host.tree_sum_host(C.c_longlong(M), _p(terms)))
