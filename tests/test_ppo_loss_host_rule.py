"""The per-row rule, the reduction tree and the final values of csrc/ccx_ppo.h -- the very source the kernels of
ccx_ppo_loss.hip inline -- compiled for the host (-O2 -ffp-contract=off) and run against the NumPy spec
(tests/_ppo_loss_spec.py) bit for bit: forward, backward with each gradient output alone, the moments and the bare tree, with
and without masks, valid and norm.  No GPU."""

import ctypes as C
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest
from _ppo_loss_spec import (case_args, clean_case, make_ppo_case, masked_moments_spec, ppo_loss_backward_spec, ppo_loss_spec,
                            tree_sum)
from _sample_spec import bits32, exp_spec

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "collectivecrossing_amd" / "csrc"
ROWS = (1, 63, 257, 1023, 16389)                                         # 16389: B = 65, a place of the final wave adds twice
HYPER = dict(clip=0.2, vf_coef=0.5, ent_coef=0.01, adv_eps=1e-8)


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
    so = tmp_path_factory.mktemp("ppo_host_rule") / "libppo_loss_host_rule.so"
    subprocess.run([cxx, "-std=c++17", "-O2", "-ffp-contract=off", "-fPIC", "-shared", f"-I{CSRC}",
                    str(Path(__file__).with_name("ppo_loss_host_rule.cpp")), "-o", str(so)], check=True)
    lib = C.CDLL(str(so))
    for name in ("host_ppo_loss", "host_ppo_loss_backward", "host_masked_moments"):
        getattr(lib, name).restype = None
    lib.host_tree.restype = C.c_double
    lib.host_exp_spec.restype = C.c_float
    lib.host_exp_spec.argtypes = [C.c_float]
    return lib


@pytest.fixture(scope="module")
def case():
    return make_ppo_case(max(ROWS), seed=31, density=0.7)


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _f(*xs):
    return [C.c_float(float(x)) for x in xs]


def _call_forward(host, M, kw, norm, hyper=HYPER):
    stats = np.full(8, np.nan, np.float32)
    host.host_ppo_loss(C.c_longlong(M), _p(kw["logits"]), _p(kw["actions"]), _p(kw["masks"]), _p(kw["logp_old"]),
                       _p(kw["advantages"]), _p(kw["returns"]), _p(kw["values"]), _p(kw["valid"]), _p(norm),
                       *_f(hyper["clip"], hyper["vf_coef"], hyper["ent_coef"], hyper["adv_eps"]), _p(stats))
    return stats


def _variants(case, M):
    norm = np.array([0.125, 0.75], np.float32)
    for masked in (True, False):
        for with_valid in (True, False):
            kw = case_args(case, masked, True, M) if with_valid else clean_case(case, masked, M)
            for nm in (norm, None):
                yield f"M {M} masked {masked} valid {with_valid} norm {nm is not None}", kw, nm


@pytest.mark.parametrize("M", ROWS)
def test_forward_and_backward_equal_the_spec(host, case, M):
    for tag, kw, norm in _variants(case, M):
        stats = _call_forward(host, M, kw, norm)
        want = ppo_loss_spec(**kw, norm=norm, **HYPER)
        np.testing.assert_array_equal(bits32(stats), bits32(want), err_msg="stats " + tag)
        gloss = np.array([-1.75], np.float32)
        for which, gl_in in ((3, gloss), (1, None), (2, gloss)):
            gl = np.full((M, 5), np.nan, np.float32) if which & 1 else None
            gv = np.full(M, np.nan, np.float32) if which & 2 else None
            host.host_ppo_loss_backward(C.c_longlong(M), _p(kw["logits"]), _p(kw["actions"]), _p(kw["masks"]), _p(kw["logp_old"]),
                                        _p(kw["advantages"]), _p(kw["returns"]), _p(kw["values"]), _p(kw["valid"]), _p(norm),
                                        *_f(HYPER["clip"], HYPER["vf_coef"], HYPER["ent_coef"], HYPER["adv_eps"]), _p(stats),
                                        _p(gl_in), _p(gl), _p(gv))
            wl, wv = ppo_loss_backward_spec(**kw, norm=norm, **HYPER, stats=want, grad_loss=None if gl_in is None else gl_in[0],
                                            want_logits=bool(which & 1), want_values=bool(which & 2))
            if which & 1:
                np.testing.assert_array_equal(bits32(gl), bits32(wl), err_msg=f"grad_logits {which} " + tag)
                assert np.isfinite(gl).all()
            if which & 2:
                np.testing.assert_array_equal(bits32(gv), bits32(wv), err_msg=f"grad_values {which} " + tag)
                assert np.isfinite(gv).all()


def test_no_row_counts(host, case):
    M = 300
    kw = case_args(case, True, True, M)
    kw["valid"] = np.zeros(M, np.uint8)
    stats = _call_forward(host, M, kw, None)
    assert not bits32(stats).any()                                       # eight times +0.0f
    gl, gv = np.full((M, 5), np.nan, np.float32), np.full(M, np.nan, np.float32)
    host.host_ppo_loss_backward(C.c_longlong(M), _p(kw["logits"]), _p(kw["actions"]), _p(kw["masks"]), _p(kw["logp_old"]),
                                _p(kw["advantages"]), _p(kw["returns"]), _p(kw["values"]), _p(kw["valid"]), None,
                                *_f(0.2, 0.5, 0.01, 1e-8), _p(stats), None, _p(gl), _p(gv))
    assert not bits32(gl).any() and not bits32(gv).any()


@pytest.mark.parametrize("M", ROWS)
def test_moments_and_the_bare_tree_equal_the_spec(host, case, M):
    rng = np.random.default_rng(M)
    x = (rng.standard_normal(M) * 3 + 1).astype(np.float32)
    for valid in (None, case["valid"][:M].copy(), np.zeros(M, np.uint8), (np.arange(M) == M // 2).astype(np.uint8)):
        xx = x.copy()
        if valid is not None:
            xx[valid == 0] = np.nan
        out = np.full(4, np.nan, np.float32)
        host.host_masked_moments(C.c_longlong(M), _p(xx), _p(valid), _p(out))
        np.testing.assert_array_equal(bits32(out), bits32(masked_moments_spec(xx, valid)))
    terms = rng.standard_normal(M) * np.exp(rng.uniform(-20, 20, M))
    got = host.host_tree(C.c_longlong(M), _p(terms))
    assert np.float64(got).view(np.uint64) == np.float64(tree_sum(terms)).view(np.uint64)


def test_exp_spec_on_the_positive_half(host):
    xs = np.concatenate([np.linspace(0, 80, 4001), [80.0, 79.99999, 1e-30, 0.0]]).astype(np.float32)
    got = np.array([host.host_exp_spec(C.c_float(float(x))) for x in xs], np.float32)
    np.testing.assert_array_equal(bits32(got), bits32(exp_spec(xs)))
    assert np.isfinite(got).all() and got[-1] == 1.0
