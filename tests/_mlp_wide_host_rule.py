"""The host-compiled rules of csrc/ccx_mlp_wide.h (tests/mlp_wide_host_rule.cpp: -O2 -ffp-contract=off) behind ctypes.  TEST
INFRASTRUCTURE ONLY.  tests/test_mlp_wide_host_rule.py shows them equal to the NumPy specs bit for bit; with that shown, the
GPU tests take them as their reference where the NumPy specs' Python loops are too slow.  The same library exports the
launch-shape functions of the header (tests/test_mlp_wide_shape_classes.py)."""

from __future__ import annotations

import ctypes as C
import subprocess
from pathlib import Path
from typing import NamedTuple

import numpy as np
from _mlp_host_rule import CSRC, compiler, ptr  # noqa: F401

F32 = np.float32
SOURCE = Path(__file__).with_name("mlp_wide_host_rule.cpp")


def load(cxx, directory):
    so = Path(directory) / "libmlp_wide_host_rule.so"
    subprocess.run([cxx, "-std=c++17", "-O2", "-ffp-contract=off", "-fPIC", "-shared", f"-I{CSRC}", str(SOURCE), "-o", str(so)], check=True)
    lib = C.CDLL(str(so))
    for name in ("host_wide", "host_narrow", "host_wide_backward", "host_narrow_backward", "host_wide_shape"):
        getattr(lib, name).restype = C.c_int
    lib.host_wide_workspace_bytes.restype = C.c_longlong
    return lib


def host_forward(lib, x, w1t, b1, w2, b2, activation, with_hidden=True, narrow=False):
    """(y f32 [M, O], hidden f32 [M, H] or None) by ccx_wide::wide_row (``narrow``: ccx_mlp::mlp_row); the outputs start as NaN."""
    x, w1t, b1, w2, b2 = (np.ascontiguousarray(v, F32) for v in (x, w1t, b1, w2, b2))
    (M, L), H, O = x.shape, w1t.shape[1], w2.shape[0]
    y = np.full((M, O), np.nan, F32)
    hid = np.full((M, H), np.nan, F32) if with_hidden else None
    fn = lib.host_narrow if narrow else lib.host_wide
    rc = fn(C.c_longlong(M), L, H, O, activation, ptr(x), ptr(w1t), ptr(b1), ptr(w2), ptr(b2), ptr(y), ptr(hid))
    assert rc == 0, (L, H, O, activation)
    return y, hid


def host_backward(lib, x, hidden, grad_y, w2, activation, narrow=False):
    """dict(w1t, b1, w2, b2, ga[, ga_slabs]) by ccx_wide::backward_host (``narrow``: ccx_mlp_grad::backward_host)."""
    x, hidden, grad_y, w2 = (np.ascontiguousarray(v, F32) for v in (x, hidden, grad_y, w2))
    (M, L), H, O = x.shape, hidden.shape[1], w2.shape[0]
    assert hidden.shape[0] == M and grad_y.shape == (M, O) and w2.shape == (O, H)
    got = dict(w1t=np.full((L, H), np.nan, F32), b1=np.full(H, np.nan, F32), w2=np.full((O, H), np.nan, F32), b2=np.full(O, np.nan, F32),
               ga=np.full((M, H), np.nan, F32))
    args = [C.c_longlong(M), L, H, O, activation, ptr(x), ptr(hidden), ptr(grad_y), ptr(w2), ptr(got["w1t"]), ptr(got["b1"]),
            ptr(got["w2"]), ptr(got["b2"]), ptr(got["ga"])]
    if narrow:
        rc = lib.host_narrow_backward(*args)
    else:
        got["ga_slabs"] = np.full((M, H), np.nan, F32)
        rc = lib.host_wide_backward(*args, ptr(got["ga_slabs"]))
    assert rc == 0, (M, L, H, O, activation)
    return got


class LaunchShape(NamedTuple):
    chunk: int                         # outputs of a chunk of the forward's layer 2
    chunks: int                        # chunks per tile
    forward_bytes: int                 # dynamic LDS of a forward workgroup
    slab: int                          # outputs of a w2 slab of the backward
    slabs: int
    rows1: int                         # rows of a sub-tile, slices of [x | 1]^T ga
    bytes1: int
    rows2: int                         # .. slices of grad_y^T [hidden | 1]
    bytes2: int
    slices1: int
    grid_y: int


def launch_shape(lib, L, H, O):
    out = (C.c_longlong * 11)()
    rc = lib.host_wide_shape(L, H, O, out)
    assert rc == 0, (L, H, O, rc)
    return LaunchShape(*[int(v) for v in out])
