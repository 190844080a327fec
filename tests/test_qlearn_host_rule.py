"""The rules of csrc/ccx_qlearn.h -- the very source the kernels of ccx_qlearn.hip inline -- compiled for the host (-O2
-ffp-contract=off) and run against the NumPy spec (tests/_qlearn_spec.py) bit for bit: the epsilon-greedy actions (greedy,
three rates, masked or not), the forward ``stats`` and ``td_error`` and the backward, for every NULL combination of the
optional inputs, double-Q off included, and with no row that counts.  No GPU."""

import ctypes as C
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest
from _qlearn_spec import (TD_VARIANTS, make_q_case, make_td_case, q_actions_scalar, q_actions_spec, td_args, td_loss_backward_spec,
                          td_loss_spec)
from _sample_spec import bits32

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "collectivecrossing_amd" / "csrc"
ROWS = (1, 63, 257, 1023, 16389)                                         # 16389: B = 65, a place of the final wave adds twice
SEED = 0x0123_4567_89AB_CDEF
GAMMA, DELTA = 0.97, 1.0


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
    so = tmp_path_factory.mktemp("qlearn_host_rule") / "libqlearn_host_rule.so"
    subprocess.run([cxx, "-std=c++17", "-O2", "-ffp-contract=off", "-fPIC", "-shared", f"-I{CSRC}",
                    str(Path(__file__).with_name("qlearn_host_rule.cpp")), "-o", str(so)], check=True)
    lib = C.CDLL(str(so))
    for name in ("host_q_actions", "host_td_loss", "host_td_loss_backward"):
        getattr(lib, name).restype = None
    return lib


@pytest.fixture(scope="module")
def case():
    return make_td_case(max(ROWS), seed=41, huber_delta=DELTA)


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _td_ptrs(kw):
    return [_p(kw[k]) for k in ("q", "actions", "reward", "done", "q_next_target", "q_next_online", "masks_next", "valid", "weights")]


def _forward(host, M, kw, gamma=GAMMA, delta=DELTA, want_td=True):
    stats = np.full(8, np.nan, np.float32)
    td = np.full(M, np.nan, np.float32) if want_td else None
    host.host_td_loss(C.c_longlong(M), *_td_ptrs(kw), C.c_float(gamma), C.c_float(delta), _p(stats), _p(td))
    return stats, td


def _backward(host, M, kw, stats, grad_loss, gamma=GAMMA, delta=DELTA):
    gq = np.full((M, 5), np.nan, np.float32)
    host.host_td_loss_backward(C.c_longlong(M), *_td_ptrs(kw), C.c_float(gamma), C.c_float(delta), _p(stats), _p(grad_loss), _p(gq))
    return gq


@pytest.mark.parametrize("E,N", [(21, 3), (9, 8), (130, 50)])
def test_q_actions_equal_the_spec(host, E, N):
    case = make_q_case(E, N, seed=E * 100 + N)
    state = (case["terminated"], case["truncated"], case["step_count"], case["episode"])
    offset = (1 << 40) + 12_345
    for masked in (True, False):
        q, masks = (case["q_masked"], case["masks"]) if masked else (case["q"], None)
        q = np.ascontiguousarray(q)
        for eps in (None, 0.0, 0.25, 1.0, float("nan")):
            acts, expl = np.full((E, N), 0xEE, np.uint8), np.full((E, N), 0xEE, np.uint8)
            rate = None if eps is None else np.array([eps], np.float32)
            host.host_q_actions(C.c_longlong(E), C.c_int(N), _p(q), _p(masks), *(_p(np.ascontiguousarray(s)) for s in state),
                                C.c_ulonglong(offset), C.c_ulonglong(SEED), _p(rate), _p(acts), _p(expl))
            want = q_actions_spec(q, masks, *state, env_offset=offset, seed=SEED, epsilon=eps)
            np.testing.assert_array_equal(acts, want[0], err_msg=f"actions masked {masked} eps {eps}")
            np.testing.assert_array_equal(expl, want[1], err_msg=f"explored masked {masked} eps {eps}")
            if E * N < 100:                                              # the header's steps one slot at a time
                one = q_actions_scalar(q, masks, *state, env_offset=offset, seed=SEED, epsilon=eps)
                np.testing.assert_array_equal(want[0], one[0])
                np.testing.assert_array_equal(want[1], one[1])
            dead = (case["terminated"] | case["truncated"]) != 0
            assert (acts[dead] == 255).all() and not expl[dead].any() and (acts[~dead] <= 4).all()
            if masked:
                live = ~dead
                assert ((((case["masks"][live] & 0x1F) | 0x10) >> acts[live]) & 1).all()      # legal under its mask


@pytest.mark.parametrize("M", ROWS)
def test_forward_and_backward_equal_the_spec(host, case, M):
    gloss = np.array([-1.75], np.float32)
    for variant in TD_VARIANTS:
        tag = f"M {M} masked {variant[0]} double {variant[1]} valid {variant[2]} weights {variant[3]}"
        kw = td_args(case, *variant, M=M)
        stats, td = _forward(host, M, kw)
        want_stats, want_td = td_loss_spec(**kw, gamma=GAMMA, huber_delta=DELTA)
        np.testing.assert_array_equal(bits32(stats), bits32(want_stats), err_msg="stats " + tag)
        np.testing.assert_array_equal(bits32(td), bits32(want_td), err_msg="td_error " + tag)
        assert np.isfinite(stats).all() and np.isfinite(td).all()
        assert (stats[6] >= 1 and (stats[7] >= 1 or M < 63)) or M == 1
        np.testing.assert_array_equal(bits32(_forward(host, M, kw, want_td=False)[0]), bits32(want_stats))
        for gl in (None, gloss):
            gq = _backward(host, M, kw, stats, gl)
            want = td_loss_backward_spec(**kw, gamma=GAMMA, huber_delta=DELTA, stats=want_stats, grad_loss=None if gl is None else gl[0])
            np.testing.assert_array_equal(bits32(gq), bits32(want), err_msg="grad_q " + tag)
            assert np.isfinite(gq).all()


def test_other_hyper_parameters(host, case):
    M = 1023
    for gamma, delta in ((0.0, 0.5), (1.0, float("inf")), (0.5, 3.0)):
        kw = td_args(case, True, True, True, True, M=M)
        stats, td = _forward(host, M, kw, gamma, delta)
        want_stats, want_td = td_loss_spec(**kw, gamma=gamma, huber_delta=delta)
        np.testing.assert_array_equal(bits32(stats), bits32(want_stats), err_msg=f"gamma {gamma} delta {delta}")
        np.testing.assert_array_equal(bits32(td), bits32(want_td))
        gq = _backward(host, M, kw, stats, None, gamma, delta)
        np.testing.assert_array_equal(bits32(gq), bits32(td_loss_backward_spec(**kw, gamma=gamma, huber_delta=delta, stats=want_stats)))


def test_no_row_counts(host, case):
    M = 300
    kw = td_args(case, True, True, True, True, M=M)
    kw["valid"] = np.zeros(M, np.uint8)
    stats, td = _forward(host, M, kw)
    assert not bits32(stats).any() and not bits32(td).any()             # +0.0f throughout (bad rows need a valid byte too)
    gq = _backward(host, M, kw, stats, None)
    assert not bits32(gq).any()
