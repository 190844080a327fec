"""The host-compiled rules of csrc/ccx_mlp_deep.h (tests/mlp_deep_host_rule.cpp: -O2 -ffp-contract=off) behind ctypes.  TEST
INFRASTRUCTURE ONLY.  tests/test_mlp_deep_host_rule.py shows them equal to the NumPy spec (tests/_mlp_deep_spec.py) bit for
bit; with that shown, the GPU tests take them as their reference where the NumPy spec's Python loops are too slow.  The
same library exports the launch-shape functions of the header."""

from __future__ import annotations

import ctypes as C
import subprocess
from pathlib import Path
from typing import NamedTuple

import numpy as np
from _mlp_deep_spec import NAMES
from _mlp_host_rule import CSRC, compiler, ptr  # noqa: F401

F32 = np.float32
SOURCE = Path(__file__).with_name("mlp_deep_host_rule.cpp")


def load(cxx, directory):
    so = Path(directory) / "libmlp_deep_host_rule.so"
    subprocess.run([cxx, "-std=c++17", "-O2", "-ffp-contract=off", "-fPIC", "-shared", f"-I{CSRC}", str(SOURCE), "-o", str(so)], check=True)
    lib = C.CDLL(str(so))
    for name in ("host_deep", "host_narrow", "host_deep_backward", "host_narrow_backward", "host_deep_shape"):
        getattr(lib, name).restype = C.c_int
    lib.host_deep_workspace_bytes.restype = C.c_longlong
    return lib


def host_forward(lib, x, w1t, b1, w2t, b2, w3, b3, activation, with_hidden=True):
    """(y, hidden1, hidden2) by ccx_deep::deep_row (the hiddens None without ``with_hidden``); the outputs start as NaN."""
    x, w1t, b1, w2t, b2, w3, b3 = (np.ascontiguousarray(v, F32) for v in (x, w1t, b1, w2t, b2, w3, b3))
    (M, L), H1, H2, O = x.shape, w1t.shape[1], w2t.shape[1], w3.shape[0]
    y = np.full((M, O), np.nan, F32)
    h1 = np.full((M, H1), np.nan, F32) if with_hidden else None
    h2 = np.full((M, H2), np.nan, F32) if with_hidden else None
    rc = lib.host_deep(C.c_longlong(M), L, H1, H2, O, activation, *(ptr(v) for v in (x, w1t, b1, w2t, b2, w3, b3, y, h1, h2)))
    assert rc == 0, (L, H1, H2, O, activation)
    return y, h1, h2


def host_narrow(lib, x, w1t, b1, w2, b2, activation):
    """(y, hidden) by ccx_mlp::mlp_row."""
    x, w1t, b1, w2, b2 = (np.ascontiguousarray(v, F32) for v in (x, w1t, b1, w2, b2))
    (M, L), H, O = x.shape, w1t.shape[1], w2.shape[0]
    y, hid = np.full((M, O), np.nan, F32), np.full((M, H), np.nan, F32)
    rc = lib.host_narrow(C.c_longlong(M), L, H, O, activation, *(ptr(v) for v in (x, w1t, b1, w2, b2, y, hid)))
    assert rc == 0, (L, H, O, activation)
    return y, hid


def host_backward(lib, x, hidden1, hidden2, grad_y, w2t, w3, activation):
    """dict(w1t, b1, w2t, b2, w3, b3, ga1, ga2) by ccx_deep::backward_host; the outputs start as NaN."""
    x, hidden1, hidden2, grad_y, w2t, w3 = (np.ascontiguousarray(v, F32) for v in (x, hidden1, hidden2, grad_y, w2t, w3))
    (M, L), (H1, H2), O = x.shape, w2t.shape, w3.shape[0]
    assert hidden1.shape == (M, H1) and hidden2.shape == (M, H2) and grad_y.shape == (M, O) and w3.shape == (O, H2)
    shapes = ((L, H1), (H1,), (H1, H2), (H2,), (O, H2), (O,), (M, H1), (M, H2))
    got = {n: np.full(s, np.nan, F32) for n, s in zip(NAMES + ("ga1", "ga2"), shapes)}
    rc = lib.host_deep_backward(C.c_longlong(M), L, H1, H2, O, activation, *(ptr(v) for v in (x, hidden1, hidden2, grad_y, w2t, w3)),
                                *(ptr(got[n]) for n in NAMES + ("ga1", "ga2")))
    assert rc == 0, (M, L, H1, H2, O, activation)
    return got


def host_narrow_backward(lib, x, hidden, grad_y, w2, activation):
    """dict(w1t, b1, w2, b2, ga) by ccx_mlp_grad::backward_host (general in O)."""
    x, hidden, grad_y, w2 = (np.ascontiguousarray(v, F32) for v in (x, hidden, grad_y, w2))
    (M, L), H, O = x.shape, hidden.shape[1], w2.shape[0]
    got = dict(w1t=np.full((L, H), np.nan, F32), b1=np.full(H, np.nan, F32), w2=np.full((O, H), np.nan, F32), b2=np.full(O, np.nan, F32),
               ga=np.full((M, H), np.nan, F32))
    rc = lib.host_narrow_backward(C.c_longlong(M), L, H, O, activation, ptr(x), ptr(hidden), ptr(grad_y), ptr(w2),
                                  *(ptr(got[n]) for n in ("w1t", "b1", "w2", "b2", "ga")))
    assert rc == 0, (M, L, H, O, activation)
    return got


class LaunchShape(NamedTuple):
    forward_bytes: int                 # dynamic LDS of a forward workgroup
    fused_bytes: int                   # .. of the fused kernels (the tile's y kept)
    waves: int                         # waves of a forward workgroup
    sub_rows: int                      # rows of a sub-tile of the backward's blocks kernel
    grad_bytes: int                    # its dynamic LDS
    slices1: int
    slices2: int
    slices3: int


def launch_shape(lib, L, H1, H2, O):
    out = (C.c_longlong * 8)()
    rc = lib.host_deep_shape(L, H1, H2, O, out)
    assert rc == 0, (L, H1, H2, O, rc)
    return LaunchShape(*[int(v) for v in out])
