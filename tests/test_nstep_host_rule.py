"""The rules of csrc/ccx_nstep.h -- the very source the kernels of ccx_nstep.hip inline -- compiled for the host (-O2
-ffp-contract=off) and run against the spec (tests/_nstep_spec.py) bit for bit: the cut bytes of a push and of a manual cut,
the availability, the walk (m_env, the span, done, valid, the record the window ends on) and the f64 chain with its f32
discount, on the synthetic ring at every head state and on random rings.  The same source with its own ``main``, built with
-fsanitize=address,undefined, walks a few hundred random small rings as a program of its own.  No GPU."""

import ctypes as C
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest
from _nstep_cases import synthetic, synthetic_states
from _nstep_spec import avail_spec, cut_push_spec, mark_cut_spec, new_cut, nstep_fetch_spec
from _replay_spec import new_ring

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "collectivecrossing_amd" / "csrc"
SOURCE = Path(__file__).with_name("nstep_host_rule.cpp")
CONSTS = (6.0, 4.0, 5.0, 7.0)


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
    so = tmp_path_factory.mktemp("nstep_host_rule") / "libnstep_host_rule.so"
    subprocess.run([cxx, "-std=c++17", "-O2", "-ffp-contract=off", "-fPIC", "-shared", f"-I{CSRC}", str(SOURCE), "-o", str(so)],
                   check=True)
    lib = C.CDLL(str(so))
    for name in ("host_nstep_push", "host_nstep_mark", "host_nstep_fetch"):
        getattr(lib, name).restype = None
    lib.host_nstep_avail.restype = C.c_longlong
    return lib


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint8).reshape(a.shape + (a.itemsize,)) if a.dtype.itemsize > 1 else a


def _fetch(host, ring, cut, index, n, gamma):
    N, B = ring["N"], len(index)
    out = dict(reward=np.full((B, N), -7.0), discount=np.full((B, N), -7, np.float32), span=np.full((B, N), 77, np.uint8),
               done=np.full((B, N), 77, np.uint8), valid=np.full((B, N), 77, np.uint8), last=np.full(B, -7, np.int64),
               m_env=np.full(B, -7, np.int32))
    index = np.ascontiguousarray(index, np.int64)
    host.host_nstep_fetch(_p(ring["reward"]), _p(ring["done"]), _p(ring["valid"]), _p(cut), C.c_longlong(int(ring["state"][0])),
                          C.c_longlong(ring["S"]), C.c_longlong(ring["E"]), C.c_longlong(N), C.c_int(n), C.c_float(gamma),
                          C.c_longlong(B), _p(index), *(_p(out[k]) for k in ("reward", "discount", "span", "done", "valid", "last", "m_env")))
    return out


def _check(host, ring, cut, index, n, gamma, tag):
    got = _fetch(host, ring, cut, index, n, gamma)
    want = nstep_fetch_spec(ring, cut, index, n, gamma, CONSTS, details=True)
    for k in ("reward", "discount", "span", "done", "valid"):
        assert got[k].dtype == want[k].dtype, k
        np.testing.assert_array_equal(_bits(got[k]), _bits(want[k]), err_msg=f"{tag}: {k}")
    np.testing.assert_array_equal(got["last"], [-1 if w is None else w["last"] for w in want["windows"]], err_msg=f"{tag}: last")
    np.testing.assert_array_equal(got["m_env"], [1 if w is None else w["m_env"] for w in want["windows"]], err_msg=f"{tag}: m_env")
    return got


def test_cut_bytes_equal_the_spec(host):
    rng = np.random.default_rng(1)
    for S, E in ((4, 3), (1, 5), (6, 24)):
        got, want = new_cut(S, E), new_cut(S, E)
        head = 0
        for K in (1, max(1, S // 2), S, max(1, S - 1), 1):
            ef = (rng.integers(0, 256, (K, E)).astype(np.uint8) * (rng.random((K, E)) < 0.5)).astype(np.uint8)
            head += K
            host.host_nstep_push(_p(got), C.c_longlong(head), C.c_longlong(K), C.c_longlong(S), C.c_longlong(E), _p(ef))
            cut_push_spec(want, head, S, E, ef)
            np.testing.assert_array_equal(got, want, err_msg=f"S {S} head {head} K {K}")
            mask = (rng.random(E) < 0.5).astype(np.uint8) * 9
            for m in (mask, None):
                host.host_nstep_mark(_p(got), C.c_longlong(head), C.c_longlong(S), C.c_longlong(E), _p(m))
                mark_cut_spec(want, head, S, E, m)
                np.testing.assert_array_equal(got, want, err_msg=f"S {S} head {head}: mark")
        fresh = new_cut(S, E)
        host.host_nstep_mark(_p(fresh), C.c_longlong(0), C.c_longlong(S), C.c_longlong(E), None)
        assert not fresh.any()                                            # an empty ring: nothing to mark
        host.host_nstep_push(_p(fresh), C.c_longlong(0), C.c_longlong(1), C.c_longlong(S), C.c_longlong(E), _p(np.full((1, E), 4, np.uint8)))
        assert fresh[:E].all() and not fresh[E:].any()                    # head' - K < 0 counts as 0


def test_availability_equals_the_spec(host):
    for S in (1, 2, 5, 6, 16):
        for head in sorted({0, 1, S - 1, S, S + 1, 2 * S, 2 * S + 3, (1 << 40) + 3}):
            for p in range(S):
                assert host.host_nstep_avail(C.c_longlong(head), C.c_longlong(p), C.c_longlong(S)) == avail_spec(head, p, S), (S, head, p)


def test_walk_and_chain_on_the_synthetic_ring(host):
    ring, cut, where = synthetic()
    R = ring["S"] * ring["E"]
    index = np.array([-1, R, 1 << 40] + list(range(R)) + [3, 3], np.int64)
    for head, what in synthetic_states():
        ring["state"][0] = head
        for n in (1, 2, 3, 5):
            for gamma in (0.5, 0.99, 1.0, 0.0):
                got = _check(host, ring, cut, index, n, gamma, f"{what} n {n} gamma {gamma}")
                assert (got["span"][:3] == 1).all() and (got["discount"][:3] == np.float32(gamma)).all()
    ring["state"][0] = 7
    got = _fetch(host, ring, cut, np.array([where["agent_early"], where["nan_just_beyond"]], np.int64), 3, 0.5)
    assert got["span"][0].tolist() == [1, 1, 3] and got["valid"][0].tolist() == [4, 0, 4] and np.isnan(got["reward"][0, 2])
    assert not np.isnan(got["reward"][1]).any() and got["m_env"].tolist() == [3, 2]


@pytest.mark.parametrize("seed", range(6))
def test_walk_and_chain_on_random_rings(host, seed):
    rng = np.random.default_rng(seed)
    S, E, N = int(rng.integers(1, 18)), int(rng.integers(1, 5)), int(rng.integers(1, 5))
    ring, R = new_ring(S, E, N), S * E
    ring["reward"][:] = rng.standard_normal((R, N)) * 10.0 ** rng.integers(-3, 4, (R, N))
    ring["done"][:] = rng.random((R, N)) < 0.15
    ring["valid"][:] = (rng.random((R, N)) < 0.85) * 4
    cut = (rng.random(R) < 0.2).astype(np.uint8) * rng.integers(1, 256, R).astype(np.uint8)
    index = np.concatenate([np.arange(-1, R + 1), rng.integers(0, R, 7)])
    for head in sorted({0, 1, S // 2, S, S + 1, 3 * S + S // 2}):
        ring["state"][0] = head
        for n in sorted({1, 2, min(S, 3), min(S, 16)}):
            if n <= S:
                _check(host, ring, cut, index, n, float(rng.choice([0.99, 0.9, 1.0, 0.0])), f"S {S} head {head} n {n}")


def test_walk_under_address_and_undefined_behaviour_sanitizers(tmp_path):
    """The same source as a program of its own (its own ``main``), built with the sanitizers and run as a subprocess: every
    ring array has exactly the ring's size, so a slot outside it ends the program."""
    cxx = _compiler()
    if cxx is None:
        pytest.skip("no host C++ compiler (c++, clang++ or ROCm's clang++)")
    exe = tmp_path / "nstep_host_rule_san"
    plain = [cxx, "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-DNSTEP_HOST_MAIN", f"-I{CSRC}", str(SOURCE), "-o", str(exe)]
    subprocess.run(plain, check=True)                                    # (the program itself compiles: a failure below is the runtime's)
    build = subprocess.run(plain + ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"], capture_output=True, text=True)
    if build.returncode:
        pytest.skip("the compiler has no sanitizer runtime: " + build.stderr.strip()[-200:])
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    print(run.stdout.strip())
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-4000:]
    assert "windows walked" in run.stdout
