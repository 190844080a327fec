"""The rules of csrc/ccx_c51.h -- the very source the kernels of ccx_c51.hip inline -- compiled for the host (-O2
-ffp-contract=off) and run against the NumPy spec (tests/_c51_spec.py) bit for bit, on random rows and on rows with +-0,
+-inf, NaN and subnormals.  The same source with its own ``main``, built with -fsanitize=address,undefined, runs as a program of
its own.  No GPU."""

import ctypes as C
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest
from _c51_spec import ATOMS, C51_VARIANTS, c51_args, c51_loss_backward_spec, c51_loss_spec, make_c51_case, q_values_spec
from _mlp_spec import bits32c

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "collectivecrossing_amd" / "csrc"
SOURCE = Path(__file__).with_name("c51_host_rule.cpp")
VMIN, VMAX = -10.0, 10.0


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
    so = tmp_path_factory.mktemp("c51_host_rule") / "libc51_host_rule.so"
    subprocess.run([cxx, "-std=c++17", "-O2", "-ffp-contract=off", "-fPIC", "-shared", f"-I{CSRC}", str(SOURCE), "-o", str(so)],
                   check=True)
    lib = C.CDLL(str(so))
    lib.host_c51_q_values.restype = lib.host_c51_loss.restype = lib.host_c51_backward.restype = None
    return lib


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def run_host(host, kw, gamma=0.99, vmin=VMIN, vmax=VMAX, grad_loss=None):
    """(q, stats, row_loss, proj, grad_logits) of the host build on the arrays of ``kw`` (c51_args)."""
    lg = kw["logits"]
    M, _, A = lg.shape
    q = np.full((M, 5), 7.0, np.float32)
    stats, row_loss = np.full(8, 7.0, np.float32), np.full(M, 7.0, np.float32)
    proj, grad = np.full((M, A), 7.0, np.float32), np.full((M, 5, A), 7.0, np.float32)
    f = C.c_float
    host.host_c51_q_values(C.c_longlong(M), A, f(vmin), f(vmax), _p(lg), _p(q))
    host.host_c51_loss(C.c_longlong(M), A, f(vmin), f(vmax), _p(lg), _p(kw["actions"]), _p(kw["reward"]), _p(kw["done"]),
                       _p(kw["next_target"]), _p(kw["next_online"]), _p(kw["masks_next"]), _p(kw["valid"]), _p(kw["weights"]),
                       _p(kw["discount"]), f(gamma), _p(stats), _p(row_loss), _p(proj))
    gl = None if grad_loss is None else np.array([grad_loss], np.float32)
    host.host_c51_backward(C.c_longlong(M), A, _p(lg), _p(kw["actions"]), _p(proj), _p(kw["valid"]), _p(kw["weights"]), _p(stats),
                           _p(gl), _p(grad))
    return q, stats, row_loss, proj, grad


def _compare(host, kw, gamma=0.99, grad_loss=None, vmin=VMIN, vmax=VMAX):
    q, stats, row_loss, proj, grad = run_host(host, kw, gamma, vmin, vmax, grad_loss)
    rest = {k: v for k, v in kw.items() if k != "discount"}
    want_stats, want_rl, want_proj = c51_loss_spec(**rest, gamma=gamma, discount=kw["discount"], vmin=vmin, vmax=vmax)
    want_grad = c51_loss_backward_spec(kw["logits"], kw["actions"], want_proj, kw["valid"], kw["weights"], want_stats, grad_loss)
    np.testing.assert_array_equal(bits32c(q), bits32c(q_values_spec(kw["logits"], vmin, vmax)))
    np.testing.assert_array_equal(bits32c(stats), bits32c(want_stats))
    np.testing.assert_array_equal(bits32c(row_loss), bits32c(want_rl))
    np.testing.assert_array_equal(bits32c(proj), bits32c(want_proj))
    np.testing.assert_array_equal(bits32c(grad), bits32c(want_grad))
    return stats, row_loss, proj, grad


@pytest.mark.parametrize("A", ATOMS)
def test_random_rows_equal_the_spec(host, A):
    case = make_c51_case(700, A, seed=A, special=False)
    for variant in C51_VARIANTS:
        stats, row_loss, proj, grad = _compare(host, c51_args(case, *variant), gamma=0.97, grad_loss=-1.75)
        assert np.isfinite(stats).all() and stats[6] > 100 and np.isfinite(proj).all() and np.isfinite(grad).all()
        assert (row_loss >= 0).all()


@pytest.mark.parametrize("A", (2, 51, 64))
def test_special_values_equal_the_spec(host, A):
    case = make_c51_case(1000, A, seed=5 + A, special=True)
    for variant in C51_VARIANTS:
        kw = c51_args(case, *variant)
        stats, row_loss, proj, grad = _compare(host, kw)
        assert np.isfinite(stats).all(), "NaN in rows that do not count, or in done rows' next state, reached a sum"
        gone = (kw["actions"] > 4) | ((kw["valid"] == 0) if kw["valid"] is not None else False)
        assert gone.any() and not row_loss[gone].view(np.uint32).any() and not proj[gone].view(np.uint32).any()
        assert not grad[gone].view(np.uint32).any()                      # +0.0, the sign bit included


def test_non_finite_inputs_of_a_counting_row_are_loud(host):
    A = 51
    case = make_c51_case(64, A, seed=3, special=False)
    kw = c51_args(case, masked=False, double=True, with_valid=False, with_weights=False, with_discount=True)
    kw["actions"][:] = 2
    kw["done"][:] = 0
    kw["discount"][:] = np.float32(0.99)
    kw["reward"][:] = 0.5
    for k in ("logits", "next_target", "next_online"):
        kw[k] = np.nan_to_num(kw[k], nan=0.25)
    kstar = c51_loss_spec(**kw, details=True)[3]["kstar"]
    kw["reward"][0], kw["reward"][1], kw["reward"][2] = np.nan, np.inf, -np.inf
    kw["discount"][3], kw["discount"][4] = np.nan, np.inf
    kw["logits"][5, 2, 7], kw["logits"][6, 2, 0], kw["logits"][7, 2, 50] = np.nan, np.inf, -np.inf
    kw["next_target"][8, kstar[8], 9], kw["next_target"][9, kstar[9], 1] = np.nan, -np.inf
    stats, row_loss, proj, grad = _compare(host, kw)
    assert not np.isfinite(row_loss[:10]).any() and np.isfinite(row_loss[10:]).all()
    assert not np.isfinite(stats[0])


def test_the_rule_under_address_and_undefined_behaviour_sanitizers(tmp_path):
    """The same source as a program of its own (its own ``main``), built with the sanitizers and run as a subprocess: every
    array has exactly the rows' size, so an element outside it ends the program."""
    cxx = _compiler()
    if cxx is None:
        pytest.skip("no host C++ compiler (c++, clang++ or ROCm's clang++)")
    exe = tmp_path / "c51_host_rule_san"
    plain = [cxx, "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-DC51_HOST_MAIN", f"-I{CSRC}", str(SOURCE), "-o", str(exe)]
    subprocess.run(plain, check=True)                                    # (the program itself compiles: a failure below is the runtime's)
    build = subprocess.run(plain + ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"], capture_output=True, text=True)
    if build.returncode:
        pytest.skip("the compiler has no sanitizer runtime: " + build.stderr.strip()[-200:])
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    print(run.stdout.strip())
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-4000:]
    assert "rows projected" in run.stdout
