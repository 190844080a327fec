"""The rule of csrc/ccx_adam.h -- the very source the kernels of ccx_adam.hip inline -- compiled for the host (-O2
-ffp-contract=off) and run against the NumPy spec (tests/_adam_spec.py) bit for bit: parameters, m, v, the 64 state bytes and
stats over three consecutive steps, with clipping active and inactive, weight decay on and off, the rate by value and from
``lr_dev``, a NaN and an inf gradient (a skipped step followed by a normal one) and beta1 = 0.  No GPU."""

import ctypes as C
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest
from _adam_spec import TWO_HEADS, adam_step_spec, bits32, make_adam_case, new_state, state_bytes, sum_of_squares

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "collectivecrossing_amd" / "csrc"
SETS = {"two heads": TWO_HEADS, "one element": (1,), "ragged": (257, 1, 64, 255), "B = 65": (16389,), "32 x 1": (1,) * 32}


class Row(C.Structure):
    _fields_ = [("param", C.c_void_p), ("grad", C.c_void_p), ("m", C.c_void_p), ("v", C.c_void_p), ("numel", C.c_longlong)]


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
    so = tmp_path_factory.mktemp("adam_host_rule") / "libadam_host_rule.so"
    subprocess.run([cxx, "-std=c++17", "-O2", "-ffp-contract=off", "-fPIC", "-shared", f"-I{CSRC}",
                    str(Path(__file__).with_name("adam_host_rule.cpp")), "-o", str(so)], check=True)
    lib = C.CDLL(str(so))
    lib.host_adam_step.restype = None
    lib.host_adam_blocks.restype = C.c_longlong
    lib.host_adam_locate.restype = None
    return lib


def _table(params, grads, ms, vs):
    tab = (Row * len(params))()
    for r, p, g, m, v in zip(tab, params, grads, ms, vs):
        r.param, r.grad, r.m, r.v, r.numel = p.ctypes.data, g.ctypes.data, m.ctypes.data, v.ctypes.data, p.size
    return tab


def _host_step(host, params, grads, ms, vs, state, lr, lr_dev, hyper):
    stats = np.full(4, np.nan, np.float32)
    f = lambda x: C.c_float(float(x))  # noqa: E731
    host.host_adam_step(C.c_int(len(params)), _table(params, grads, ms, vs), f(lr),
                        None if lr_dev is None else lr_dev.ctypes.data_as(C.c_void_p), f(hyper["beta1"]), f(hyper["beta2"]),
                        f(hyper["eps"]), f(hyper["weight_decay"]), f(hyper["max_grad_norm"]), state.ctypes.data_as(C.c_void_p),
                        stats.ctypes.data_as(C.c_void_p))
    return stats


def _run_both(host, numels, grad_steps, params, lrs, hyper, use_lr_dev=False):
    """Three (or more) steps on both sides; compares everything after every step.  Returns the stats of every step."""
    hp = [p.copy() for p in params]
    hm, hv = [np.zeros_like(p) for p in hp], [np.zeros_like(p) for p in hp]
    hstate = state_bytes(new_state())
    sp = [p.copy() for p in params]
    sm, sv = [np.zeros_like(p) for p in sp], [np.zeros_like(p) for p in sp]
    sstate = new_state()
    all_stats = []
    for s, (grads, lr) in enumerate(zip(grad_steps, lrs)):
        before = [g.copy() for g in grads]
        lr_dev = np.array([lr], np.float32) if use_lr_dev else None
        got = _host_step(host, hp, grads, hm, hv, hstate, 123.0 if use_lr_dev else lr, lr_dev, hyper)   # by value: not read then
        want = adam_step_spec(sp, grads, sm, sv, sstate, lr, **hyper)
        tag = f"step {s}"
        np.testing.assert_array_equal(bits32(got), bits32(want), err_msg="stats, " + tag)
        np.testing.assert_array_equal(hstate, state_bytes(sstate), err_msg="state, " + tag)
        for k in range(len(numels)):
            np.testing.assert_array_equal(bits32(hp[k]), bits32(sp[k]), err_msg=f"param {k}, {tag}")
            np.testing.assert_array_equal(bits32(hm[k]), bits32(sm[k]), err_msg=f"m {k}, {tag}")
            np.testing.assert_array_equal(bits32(hv[k]), bits32(sv[k]), err_msg=f"v {k}, {tag}")
            np.testing.assert_array_equal(bits32(grads[k]), bits32(before[k]), err_msg=f"grad {k} is read only, {tag}")
        all_stats.append(want)
    return all_stats, sp, sstate


HYPER = dict(beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.0, max_grad_norm=0.0)


@pytest.mark.parametrize("name", list(SETS))
def test_three_steps_equal_the_spec(host, name):
    numels = SETS[name]
    params, grad_steps = make_adam_case(numels, seed=len(name))
    gn = float(np.sqrt(sum_of_squares(grad_steps[0])))
    for tag, extra in (("plain", {}), ("clip above", dict(max_grad_norm=gn * 4 + 1)), ("clip active", dict(max_grad_norm=gn / 3)),
                       ("decay", dict(weight_decay=0.01)), ("decay and clip", dict(weight_decay=0.1, max_grad_norm=gn / 3)),
                       ("beta1 = 0", dict(beta1=0.0)), ("beta2 = 0", dict(beta2=0.0, max_grad_norm=gn / 3))):
        hyper = {**HYPER, **extra}
        stats, sp, state = _run_both(host, numels, grad_steps, params, (3e-4, 1e-2, 0.0), hyper)
        assert state["step"] == 3 and state["skipped"] == 0
        assert all(np.isfinite(p).all() for p in sp), tag
        if tag == "clip active":
            assert stats[0][1] < 1.0
        if tag in ("plain", "clip above"):
            assert stats[0][1] == 1.0
        _run_both(host, numels, grad_steps, params, (3e-4, 1e-2, 0.0), hyper, use_lr_dev=True)


@pytest.mark.parametrize("bad", (np.nan, np.inf, -np.inf))
def test_a_skipped_step_changes_nothing_and_the_next_continues(host, bad):
    numels = TWO_HEADS
    params, grad_steps = make_adam_case(numels, seed=5, steps=4)
    grad_steps[1][-1][-1] = bad                                          # the last place of the last tensor's tail
    grad_steps[2][0][3] = bad
    for extra in ({}, dict(max_grad_norm=0.5, weight_decay=0.01)):
        stats, sp, state = _run_both(host, numels, grad_steps, params, (3e-4,) * 4, {**HYPER, **extra})
        assert [s[2] for s in stats] == [0.0, 1.0, 1.0, 0.0]
        assert state["step"] == 2 and state["skipped"] == 2
        assert all(np.isfinite(p).all() for p in sp)


def test_a_norm_beyond_f32_is_a_skip(host):
    params = [np.ones(300, np.float32)]
    grads = [[np.full(300, 3e38, np.float32)], [np.full(300, 1e-3, np.float32)]]
    stats, sp, state = _run_both(host, (300,), grads, params, (1e-3, 1e-3), {**HYPER, "max_grad_norm": 1.0})
    assert np.isinf(stats[0][0]) and stats[0][2] == 1.0 and state["step"] == 1 and state["skipped"] == 1


def test_blocks_never_straddle_two_tensors(host):
    numels = (257, 1, 64, 255, 256, 1023)
    dummy = [np.zeros(n, np.float32) for n in numels]
    tab = _table(dummy, dummy, dummy, dummy)
    B = host.host_adam_blocks(C.c_int(len(numels)), tab)
    assert B == sum(-(-n // 256) for n in numels)
    t_of, b_in = np.full(B, -1, np.int32), np.full(B, -1, np.int64)
    host.host_adam_locate(C.c_int(len(numels)), tab, t_of.ctypes.data_as(C.c_void_p), b_in.ctypes.data_as(C.c_void_p))
    want_t = np.concatenate([np.full(-(-n // 256), k) for k, n in enumerate(numels)])
    want_b = np.concatenate([np.arange(-(-n // 256)) for n in numels])
    np.testing.assert_array_equal(t_of, want_t)
    np.testing.assert_array_equal(b_in, want_b)
