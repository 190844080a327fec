"""The host-compiled rules of csrc/ccx_mlp.h and csrc/ccx_mlp_grad.h (tests/mlp_host_rule.cpp, tests/mlp_backward_host_rule.cpp:
-O2 -ffp-contract=off) behind ctypes.  TEST INFRASTRUCTURE ONLY.  tests/test_mlp_host_rule.py and
tests/test_mlp_backward_host_rule.py show them equal to the NumPy specs bit for bit on every shape of
tests/_mlp_shape_classes.py; with that shown, tests/test_gpu_mlp_shapes.py takes them as its reference where the NumPy
spec's Python loops are too slow.  The same libraries export the launch-shape functions of the two headers."""

from __future__ import annotations

import ctypes as C
import shutil
import subprocess
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "collectivecrossing_amd" / "csrc"
F32 = np.float32


def compiler():
    for name in ("c++", "clang++"):
        if shutil.which(name):
            return shutil.which(name)
    rocm = Path("/opt/rocm/llvm/bin/clang++")
    return str(rocm) if rocm.exists() else None


def ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _load(cxx, directory, stem):
    so = Path(directory) / f"lib{stem}.so"
    subprocess.run([cxx, "-std=c++17", "-O2", "-ffp-contract=off", "-fPIC", "-shared", f"-I{CSRC}",
                    str(Path(__file__).with_name(f"{stem}.cpp")), "-o", str(so)], check=True)
    return C.CDLL(str(so))


def load_forward(cxx, directory):
    lib = _load(cxx, directory, "mlp_host_rule")
    lib.host_mlp.restype = C.c_int
    lib.host_activations.restype = None
    lib.host_lds_floats.restype = C.c_longlong
    return lib


def load_backward(cxx, directory):
    lib = _load(cxx, directory, "mlp_backward_host_rule")
    lib.host_mlp_backward.restype = C.c_int
    lib.host_mlp_backward_workspace_bytes.restype = C.c_longlong
    lib.host_sub_rows.restype = C.c_int
    lib.host_grad_grid_y.restype = C.c_int
    return lib


def host_forward(lib, x, w1t, b1, w2, b2, activation, with_hidden=True):
    """(y f32 [M, O], hidden f32 [M, H] or None) by ccx_mlp::mlp_row; the outputs start as NaN."""
    x, w1t, b1, w2, b2 = (np.ascontiguousarray(v, F32) for v in (x, w1t, b1, w2, b2))
    (M, L), H, O = x.shape, w1t.shape[1], w2.shape[0]
    y = np.full((M, O), np.nan, F32)
    hid = np.full((M, H), np.nan, F32) if with_hidden else None
    rc = lib.host_mlp(C.c_longlong(M), L, H, O, activation, ptr(x), ptr(w1t), ptr(b1), ptr(w2), ptr(b2), ptr(y), ptr(hid))
    assert rc == 0, (L, H, O, activation)
    return y, hid


def host_backward(lib, x, hidden, grad_y, w2, activation):
    """dict(w1t, b1, w2, b2, ga) by ccx_mlp_grad::backward_host; the outputs start as NaN."""
    x, hidden, grad_y, w2 = (np.ascontiguousarray(v, F32) for v in (x, hidden, grad_y, w2))
    (M, L), H, O = x.shape, hidden.shape[1], w2.shape[0]
    assert hidden.shape[0] == M and grad_y.shape == (M, O) and w2.shape == (O, H)
    got = dict(w1t=np.full((L, H), np.nan, F32), b1=np.full(H, np.nan, F32), w2=np.full((O, H), np.nan, F32), b2=np.full(O, np.nan, F32),
               ga=np.full((M, H), np.nan, F32))
    rc = lib.host_mlp_backward(C.c_longlong(M), L, H, O, activation, ptr(x), ptr(hidden), ptr(grad_y), ptr(w2), ptr(got["w1t"]),
                               ptr(got["b1"]), ptr(got["w2"]), ptr(got["b2"]), ptr(got["ga"]))
    assert rc == 0, (M, L, H, O, activation)
    return got


def sub_rows(lib, L, H, O, per_row=0):
    """(R, bytes) of ccx_mlp_grad::sub_rows: per_row = 0 the adjacent-rows kernel, 8 the picked-rows kernel."""
    b = C.c_longlong(-1)
    R = lib.host_sub_rows(L, H, O, per_row, C.byref(b))
    return R, b.value
