"""The rules of csrc/ccx_mlp_deep.h -- the very source the kernels of ccx_mlp_deep.hip inline -- compiled for the host (-O2
-ffp-contract=off) and run against the NumPy spec of CCX_MLP_DEEP (tests/_mlp_deep_spec.py) bit for bit, on random rows and
on rows with +-0, +-inf, NaN and subnormals; against ccx_mlp::mlp_row and ccx_mlp_grad::backward_host through the
identities of the rule; the workspace size, the refusals, and the forward's LDS bytes over the catalogue and the corners of
the legal range (a CU has 160 KB).  The same source with its own ``main``, built with -fsanitize=address,undefined, runs as a
program of its own.  No GPU."""

import ctypes as C
import subprocess

import numpy as np
import pytest
from _mlp_deep_host_rule import (CSRC, SOURCE, compiler, host_backward, host_forward, host_narrow, host_narrow_backward, launch_shape,
                                 load, ptr)
from _mlp_deep_spec import (CATALOGUE, NAMES, RELU, TANH, bits32c, deep_backward_spec, deep_spec, make_deep_backward_case,
                            make_deep_case)

HIDDEN = ((16, 16), (16, 256), (256, 16), (64, 48))
CASES = tuple((7 if i % 2 else 38, H1, H2, (5, 1, 8, 6)[i], TANH if i % 2 else RELU) for i, (H1, H2) in enumerate(HIDDEN))
CASES += tuple((L, H1, H2, O, RELU if act == TANH else TANH) for L, H1, H2, O, act in CASES)


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    cxx = compiler()
    if cxx is None:
        pytest.skip("no host C++ compiler (c++, clang++ or ROCm's clang++)")
    return load(cxx, tmp_path_factory.mktemp("mlp_deep_host_rule"))


@pytest.mark.parametrize("L, H1, H2, O, act", CASES)
def test_forward_equals_the_spec(host, L, H1, H2, O, act):
    c = make_deep_case(97, L, H1, H2, O, seed=H1 + H2 + O, adversarial=True)   # rows with NaN, +-inf, +-0 and subnormals
    p = tuple(c[n] for n in NAMES)
    want = deep_spec(c["x"], *p, act)
    got = host_forward(host, c["x"], *p, act)
    for g, w in zip(got, want):
        np.testing.assert_array_equal(bits32c(g), bits32c(w))
    assert np.isnan(want[0]).any() and np.isfinite(want[0]).any() and (np.abs(want[1]) == 1.0).any() == (act == TANH)
    y2, none1, none2 = host_forward(host, c["x"], *p, act, with_hidden=False)
    assert none1 is None and none2 is None
    np.testing.assert_array_equal(bits32c(y2), bits32c(got[0]))
    # the identity: CCX_MLP's own row function on hidden1
    _, nh1 = host_narrow(host, c["x"], c["w1t"], c["b1"], np.zeros((1, H1), np.float32), np.zeros(1, np.float32), act)
    ny, nh2 = host_narrow(host, nh1, c["w2t"], c["b2"], c["w3"], c["b3"], act)
    for g, w in zip(got, (ny, nh1, nh2)):
        np.testing.assert_array_equal(bits32c(g), bits32c(w))


@pytest.mark.parametrize("L, H1, H2, O, act", CASES)
def test_backward_equals_the_spec(host, L, H1, H2, O, act):
    L = 7                                                                 # (the NumPy spec walks every element: keep them few)
    c = make_deep_backward_case(258, L, H1, H2, O, act, seed=H1 + O + 1)  # two blocks, the second of two rows
    args = (c["x"], c["hidden1"], c["hidden2"], c["grad_y"], c["w2t"], c["w3"], act)
    want = deep_backward_spec(*args)
    got = host_backward(host, *args)
    for name in NAMES + ("ga1", "ga2"):
        np.testing.assert_array_equal(bits32c(got[name]), bits32c(want[name]), err_msg=name)
        assert np.isfinite(want[name]).all() and want[name].any(), name
    # the identities: CCX_MLP's own backward on the last two layers, and with O := H2 on the first
    last = host_narrow_backward(host, c["hidden1"], c["hidden2"], c["grad_y"], c["w3"], act)
    for mine, theirs in (("w2t", "w1t"), ("b2", "b1"), ("w3", "w2"), ("b3", "b2"), ("ga2", "ga")):
        np.testing.assert_array_equal(bits32c(got[mine]), bits32c(last[theirs]), err_msg=mine)
    first = host_narrow_backward(host, c["x"], c["hidden1"], got["ga2"], np.ascontiguousarray(c["w2t"].T), act)
    for mine, theirs in (("w1t", "w1t"), ("b1", "b1"), ("ga1", "ga")):
        np.testing.assert_array_equal(bits32c(got[mine]), bits32c(first[theirs]), err_msg=mine)


def test_special_values_in_the_backward(host):
    """+-0, +-inf, NaN and subnormals in grad_y and the hiddens: where a NaN stands and every other bit are the spec's."""
    L, H1, H2, O, M = 5, 16, 32, 5, 14
    for act in (TANH, RELU):
        rng = np.random.default_rng(9 + act)
        x = rng.standard_normal((M, L)).astype(np.float32)
        h1 = rng.uniform(-0.9, 0.9, (M, H1)).astype(np.float32)
        h2 = rng.uniform(-0.9, 0.9, (M, H2)).astype(np.float32)
        w2t = rng.standard_normal((H1, H2)).astype(np.float32)
        w3 = rng.standard_normal((O, H2)).astype(np.float32)
        gy = rng.standard_normal((M, O)).astype(np.float32)
        gy[0, :], gy[1, :], gy[6, :] = 0.0, -0.0, 1e-42
        w3[:, 5], w2t[3, :] = -0.0, -0.0
        gy[2, 0], gy[3, 1], gy[4, 4] = np.inf, np.nan, -np.inf
        h2[7, 0], h2[8, 1], h1[9, 2], h1[10, 3], h1[11, 4] = np.nan, 0.0, -0.0, np.nan, 1e-41
        with np.errstate(all="ignore"):
            want = deep_backward_spec(x, h1, h2, gy, w2t, w3, act)
        got = host_backward(host, x, h1, h2, gy, w2t, w3, act)
        for name in NAMES + ("ga1", "ga2"):
            np.testing.assert_array_equal(bits32c(got[name]), bits32c(want[name]), err_msg=name)
        assert np.isnan(want["ga1"]).any() and (want["ga2"].view(np.uint32) == 0x80000000).any()


def test_workspace_bytes_and_refusals(host):
    ws = host.host_deep_workspace_bytes
    for rows in (1, 256, 257, 524288, 2**40):
        for L, H1, H2, O in CATALOGUE + ((38, 256, 256, 5),):
            want = -(-rows // 256) * (L * H1 + H1 + H1 * H2 + H2 + O * H2 + O) * 8
            assert ws(C.c_longlong(rows), L, H1, H2, O) == want, (rows, L, H1, H2, O)
    assert ws(C.c_longlong(524288), 38, 256, 256, 5) == 1_262_567_424     # what include/ccx.h and the README quote
    bad = ((0, 38, 64, 64, 5), (8, 0, 64, 64, 5), (8, 513, 64, 64, 5), (8, 38, 24, 64, 5), (8, 38, 64, 24, 5), (8, 38, 272, 64, 5),
           (8, 38, 64, 272, 5), (8, 38, 0, 64, 5), (8, 38, 64, 64, 0), (8, 38, 64, 64, 9))
    for rows, L, H1, H2, O in bad:
        assert ws(C.c_longlong(rows), L, H1, H2, O) == 0, (rows, L, H1, H2, O)
    z = np.zeros(8, np.float32)
    for rows, L, H1, H2, O in bad:
        assert host.host_deep(C.c_longlong(rows), L, H1, H2, O, 0, *([ptr(z)] * 10)) == -1, (rows, L, H1, H2, O)
        assert host.host_deep_backward(C.c_longlong(rows), L, H1, H2, O, 0, *([ptr(z)] * 14)) == -1, (rows, L, H1, H2, O)
    assert host.host_deep(C.c_longlong(4), 4, 16, 16, 1, 2, *([ptr(z)] * 10)) == -1


def test_forward_lds_bytes_of_the_catalogue_and_of_every_legal_shape(host):
    """The forward's dynamic LDS, recomputed here from the mapping (the x tile, overlaid by h1, overlaid by the partials)
    and compared with the header's own function; every legal shape stays within a CU's 160 KB and within 16 waves."""
    def want(L, H1, H2, O, draw):
        return 4 * max(64 * (L | 1), 64 * (H1 | 1), (H2 // 16 + draw) * 64 * O)

    for L, H1, H2, O in CATALOGUE:
        s = launch_shape(host, L, H1, H2, O)
        assert (s.forward_bytes, s.fused_bytes) == (want(L, H1, H2, O, 0), want(L, H1, H2, O, 1)), (L, H1, H2, O)
        assert s.waves == max(H1, H2) // 16
    assert launch_shape(host, 262, 256, 256, 8).forward_bytes == 67328 > 65536          # the opt-in above 64 KB
    assert launch_shape(host, 512, 16, 256, 1).forward_bytes == 131328
    assert launch_shape(host, 38, 64, 64, 5).forward_bytes == 16640 == 64 * 65 * 4       # h1, wider than x here
    worst = 0
    for L in (1, 2, 255, 256, 511, 512):
        for H1 in range(16, 257, 16):
            for H2 in (16, 128, 256):
                for O in (1, 5, 8):
                    s = launch_shape(host, L, H1, H2, O)
                    assert s.fused_bytes == want(L, H1, H2, O, 1) >= s.forward_bytes == want(L, H1, H2, O, 0)
                    assert s.grad_bytes <= 160 * 1024 and s.sub_rows in (8, 16, 32, 64) and 1 <= s.waves <= 16
                    worst = max(worst, s.fused_bytes)
    assert worst == 131328 <= 160 * 1024


def test_the_rule_under_address_and_undefined_behaviour_sanitizers(tmp_path):
    """The same source as a program of its own (its own ``main``), built with the sanitizers and run as a subprocess: every
    array has exactly its size, so an element outside it ends the program."""
    cxx = compiler()
    if cxx is None:
        pytest.skip("no host C++ compiler (c++, clang++ or ROCm's clang++)")
    exe = tmp_path / "mlp_deep_host_rule_san"
    plain = [cxx, "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-DMLP_DEEP_HOST_MAIN", f"-I{CSRC}", str(SOURCE), "-o", str(exe)]
    subprocess.run(plain, check=True)                                    # (the program itself compiles: a failure below is the runtime's)
    build = subprocess.run(plain + ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"], capture_output=True, text=True)
    if build.returncode:
        pytest.skip("the compiler has no sanitizer runtime: " + build.stderr.strip()[-200:])
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    print(run.stdout.strip())
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-4000:]
    assert "rows through the deep rule" in run.stdout
