"""The rules of csrc/ccx_mlp_wide.h -- the very source the kernels of ccx_mlp_wide.hip inline -- compiled for the host (-O2
-ffp-contract=off) and run against the NumPy specs of CCX_MLP (tests/_mlp_spec.py, tests/_mlp_backward_spec.py: general in O)
bit for bit, on rows with +-0, +-inf, NaN and subnormals; for O <= 8 against ccx_mlp::mlp_row and
ccx_mlp_grad::backward_host, which they must equal; the gh chain cut into slabs against the uncut one.  The same source with
its own ``main``, built with -fsanitize=address,undefined, runs as a program of its own.  No GPU."""

import ctypes as C
import subprocess

import numpy as np
import pytest
from _mlp_backward_spec import NAMES, make_mlp_backward_case, mlp_backward_spec
from _mlp_shape_classes import NUMPY_SPEC_BELOW
from _mlp_spec import RELU, TANH, bits32c, make_mlp_case, mlp_spec
from _mlp_wide_host_rule import CSRC, SOURCE, compiler, host_backward, host_forward, launch_shape, load, ptr

OUTPUTS = (1, 8, 9, 17, 255, 319, 320)
HIDDEN = (16, 64, 256)
# (L, H, O, activation): every H with every O, the activations alternating, two row lengths
CASES = tuple((7 if (i + j) % 2 else 38, H, O, TANH if (i + j) % 2 else RELU) for i, H in enumerate(HIDDEN) for j, O in enumerate(OUTPUTS))


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    cxx = compiler()
    if cxx is None:
        pytest.skip("no host C++ compiler (c++, clang++ or ROCm's clang++)")
    return load(cxx, tmp_path_factory.mktemp("mlp_wide_host_rule"))


@pytest.mark.parametrize("L, H, O, act", CASES)
def test_forward_equals_the_spec(host, L, H, O, act):
    c = make_mlp_case(97, L, H, O, seed=H + O, adversarial=True)          # rows with NaN, +-inf, +-0 and subnormals
    p = (c["x"], c["w1t"], c["b1"], c["w2"], c["b2"], act)
    want_y, want_h = mlp_spec(*p)
    y, hid = host_forward(host, *p)
    np.testing.assert_array_equal(bits32c(y), bits32c(want_y))
    np.testing.assert_array_equal(bits32c(hid), bits32c(want_h))
    assert np.isnan(want_y).any() and np.isfinite(want_y).any() and (np.abs(want_h) == 1.0).any() == (act == TANH)
    y2, none = host_forward(host, *p, with_hidden=False)
    assert none is None
    np.testing.assert_array_equal(bits32c(y2), bits32c(y))
    if O <= 8:                                                            # CCX_MLP's own row function: the same bits
        ny, nh = host_forward(host, *p, narrow=True)
        np.testing.assert_array_equal(bits32c(ny), bits32c(y))
        np.testing.assert_array_equal(bits32c(nh), bits32c(hid))


def _elements(L, H, O):
    return (L + 1) * H + O * (H + 1)


@pytest.mark.parametrize("L, H, O, act", CASES)
def test_backward_equals_the_spec(host, L, H, O, act):
    L = 7                                                                 # (the NumPy spec walks every element: keep them few)
    M = 258 if _elements(L, H, O) < NUMPY_SPEC_BELOW else 9               # two blocks, the second of two rows; nine rows above
    c = make_mlp_backward_case(M, L, H, O, act, seed=H + O + 1)
    want = mlp_backward_spec(c["x"], c["hidden"], c["grad_y"], c["w2"], act)
    got = host_backward(host, c["x"], c["hidden"], c["grad_y"], c["w2"], act)
    for name in NAMES + ("ga",):
        np.testing.assert_array_equal(bits32c(got[name]), bits32c(want[name]), err_msg=name)
        assert np.isfinite(want[name]).all() and want[name].any(), name
    np.testing.assert_array_equal(bits32c(got["ga_slabs"]), bits32c(want["ga"]))      # the chain cut into slabs: the same bits
    assert (launch_shape(host, L, H, O).slabs > 1) == (O * H > 4096)
    if O <= 8:                                                            # CCX_MLP's own backward: the same bits
        narrow = host_backward(host, c["x"], c["hidden"], c["grad_y"], c["w2"], act, narrow=True)
        for name in NAMES + ("ga",):
            np.testing.assert_array_equal(bits32c(narrow[name]), bits32c(got[name]), err_msg=name)


@pytest.mark.parametrize("act", (TANH, RELU))
def test_slabs_keep_signed_zeros_and_special_values(host, act):
    """The chain that is continued slab by slab starts from -0.0f: a first product of -0.0f, +0.0f, an infinity or a NaN
    comes out as gh_unit leaves it."""
    H, O, M = 64, 255, 12
    rng = np.random.default_rng(7)
    w2 = rng.standard_normal((O, H)).astype(np.float32)
    gy = rng.standard_normal((M, O)).astype(np.float32)
    hidden = rng.uniform(-0.9, 0.9, (M, H)).astype(np.float32)
    gy[0, :] = 0.0
    gy[1, :] = -0.0                                                       # every product a zero: the signs decide
    w2[:, 5] = -0.0
    gy[2, 0], gy[3, 0], gy[4, 64], gy[5, 254] = np.inf, np.nan, -np.inf, np.nan
    gy[6, :] = 1e-42
    x = rng.standard_normal((M, 7)).astype(np.float32)
    with np.errstate(all="ignore"):
        want = mlp_backward_spec(x, hidden, gy, w2, act)
    got = host_backward(host, x, hidden, gy, w2, act)
    np.testing.assert_array_equal(bits32c(got["ga_slabs"]), bits32c(want["ga"]))
    np.testing.assert_array_equal(bits32c(got["ga"]), bits32c(want["ga"]))
    assert (want["ga"].view(np.uint32) == 0x80000000).any() and np.isnan(want["ga"]).any()


def test_workspace_bytes_and_refusals(host):
    ws = host.host_wide_workspace_bytes
    for rows in (1, 256, 257, 131072, 2**40):
        for L, H, O in ((38, 64, 255), (1, 16, 1), (512, 256, 320), (38, 64, 5)):
            assert ws(C.c_longlong(rows), L, H, O) == -(-rows // 256) * (L * H + H + O * H + O) * 8, (rows, L, H, O)
    for rows, L, H, O in ((0, 38, 64, 5), (8, 0, 64, 5), (8, 513, 64, 5), (8, 38, 24, 5), (8, 38, 272, 5), (8, 38, 64, 0), (8, 38, 64, 321)):
        assert ws(C.c_longlong(rows), L, H, O) == 0, (rows, L, H, O)
    z = np.zeros(8, np.float32)
    for rows, L, H, O, act in ((0, 4, 16, 1, 0), (4, 0, 16, 1, 0), (4, 4, 24, 1, 0), (4, 4, 16, 321, 0), (4, 4, 16, 1, 2)):
        assert host.host_wide(C.c_longlong(rows), L, H, O, act, *([ptr(z)] * 7)) == -1, (rows, L, H, O, act)
        assert host.host_wide_backward(C.c_longlong(rows), L, H, O, act, *([ptr(z)] * 10)) == -1, (rows, L, H, O, act)


def test_the_rule_under_address_and_undefined_behaviour_sanitizers(tmp_path):
    """The same source as a program of its own (its own ``main``), built with the sanitizers and run as a subprocess: every
    array has exactly its size, so an element outside it ends the program."""
    cxx = compiler()
    if cxx is None:
        pytest.skip("no host C++ compiler (c++, clang++ or ROCm's clang++)")
    exe = tmp_path / "mlp_wide_host_rule_san"
    plain = [cxx, "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-DMLP_WIDE_HOST_MAIN", f"-I{CSRC}", str(SOURCE), "-o", str(exe)]
    subprocess.run(plain, check=True)                                    # (the program itself compiles: a failure below is the runtime's)
    build = subprocess.run(plain + ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"], capture_output=True, text=True)
    if build.returncode:
        pytest.skip("the compiler has no sanitizer runtime: " + build.stderr.strip()[-200:])
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    print(run.stdout.strip())
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-4000:]
    assert "rows through the wide rule" in run.stdout
