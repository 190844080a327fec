"""The per-row rules of csrc/ccx_softmax.h -- the very source the kernels of ccx_sample.hip and ccx_evaluate.hip inline --
compiled for the host (-O2 -ffp-contract=off) and run against the NumPy specs bit for bit: CCX_EVALUATE forward and backward
in every mask / gradient combination, and steps 2-6 of CCX_SAMPLE.  No GPU."""

import ctypes as C
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest
from _evaluate_spec import case_args, evaluate_backward_spec, evaluate_spec, make_evaluate_case
from _sample_spec import bits32, make_sample_case, sample_spec

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
    so = tmp_path_factory.mktemp("host_rule") / "libevaluate_host_rule.so"
    subprocess.run([cxx, "-std=c++17", "-O2", "-ffp-contract=off", "-fPIC", "-shared", f"-I{CSRC}",
                    str(Path(__file__).with_name("evaluate_host_rule.cpp")), "-o", str(so)], check=True)
    lib = C.CDLL(str(so))
    for name in ("host_evaluate", "host_evaluate_backward", "host_steps_2_to_6"):
        getattr(lib, name).restype = None
    return lib


@pytest.fixture(scope="module")
def case():
    return make_evaluate_case(96, 8, seed=5)


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


@pytest.mark.parametrize("masked", (True, False))
def test_forward_equals_the_spec(host, case, masked):
    logits, actions, masks, _, _ = case_args(case, masked)
    logits = np.ascontiguousarray(logits)
    M = case["M"]
    for want_entropy in (True, False):
        logp, entropy = np.full(M, np.nan, np.float32), np.full(M, np.nan, np.float32) if want_entropy else None
        host.host_evaluate(C.c_longlong(M), _p(logits), _p(actions), _p(masks), _p(logp), _p(entropy))
        want = evaluate_spec(logits, actions, masks, want_entropy)
        np.testing.assert_array_equal(bits32(logp), bits32(want[0]))
        if want_entropy:
            np.testing.assert_array_equal(bits32(entropy), bits32(want[1]))
    assert (actions == 255).any() and (actions < 5).any() and ((actions > 4) & (actions < 255)).any()
    assert np.isneginf(want[0]).any() and np.isnan(logits).any()


@pytest.mark.parametrize("masked", (True, False))
@pytest.mark.parametrize("which", (3, 1, 2))
def test_backward_equals_the_spec(host, case, masked, which):
    logits, actions, masks, glp, gent = case_args(case, masked)
    logits = np.ascontiguousarray(logits)
    glp, gent = glp if which & 1 else None, gent if which & 2 else None
    grad = np.full((case["M"], 5), np.nan, np.float32)
    host.host_evaluate_backward(C.c_longlong(case["M"]), _p(logits), _p(actions), _p(masks), _p(glp), _p(gent), _p(grad))
    np.testing.assert_array_equal(bits32(grad), bits32(evaluate_backward_spec(logits, actions, masks, glp, gent)))
    assert np.isfinite(grad).all()                                       # the NaN / inf gradients sit where the rule selects


@pytest.mark.parametrize("masked", (True, False))
def test_steps_2_to_6_equal_sample_spec(host, masked):
    E, N = 96, 8
    c = make_sample_case(E, N, seed=11)
    logits = np.ascontiguousarray((c["logits_masked"] if masked else c["logits"]).reshape(E * N, 5))
    masks = np.ascontiguousarray(c["masks"].reshape(E * N)) if masked else None
    *_, det = sample_spec(logits.reshape(E, N, 5), None if masks is None else masks.reshape(E, N), c["terminated"], c["truncated"],
                          c["step_count"], c["episode"], details=True)
    M = E * N
    legal, deg = np.full((M, 5), 7, np.uint8), np.full(M, 7, np.uint8)
    d, w, cs = (np.full((M, 5), np.nan, np.float32) for _ in range(3))
    host.host_steps_2_to_6(C.c_longlong(M), _p(logits), _p(masks), _p(legal), _p(deg), _p(d), _p(w), _p(cs))
    np.testing.assert_array_equal(legal.astype(bool), det["legal"].reshape(M, 5))
    np.testing.assert_array_equal(deg.astype(bool), det["degenerate"].reshape(M))
    for got, name in ((d, "d"), (w, "w"), (cs, "c")):
        np.testing.assert_array_equal(bits32(got), bits32(det[name].reshape(M, 5)), err_msg=name)
    np.testing.assert_array_equal(bits32(cs[:, 4]), bits32(det["S"].reshape(M)))
