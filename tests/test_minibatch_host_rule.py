"""The rules of csrc/ccx_minibatch.h -- the very source the kernels of ccx_minibatch.hip inline -- compiled for the host as a
program of its own (tests/minibatch_host_rule.cpp, its own ``main``), built with -fsanitize=address,undefined where the
compiler has the runtime, and run as a subprocess: the permutations, walk lengths, draws and states it prints equal the spec
(tests/_minibatch_spec.py) as exact integers.  Nothing is loaded into Python.  No GPU."""

import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest
from _minibatch_spec import M_LIST, advance_spec, draw_spec, perm_spec
from _replay_spec import rows_spec

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "collectivecrossing_amd" / "csrc"
SOURCE = Path(__file__).with_name("minibatch_host_rule.cpp")


def _compiler():
    for name in ("c++", "clang++"):
        if shutil.which(name):
            return shutil.which(name)
    rocm = Path("/opt/rocm/llvm/bin/clang++")
    return str(rocm) if rocm.exists() else None


@pytest.fixture(scope="module")
def printed(tmp_path_factory):
    cxx = _compiler()
    if cxx is None:
        pytest.skip("no host C++ compiler (c++, clang++ or ROCm's clang++)")
    exe = tmp_path_factory.mktemp("minibatch_host_rule") / "minibatch_host_rule"
    plain = [cxx, "-std=c++17", "-O1", "-g", f"-I{CSRC}", str(SOURCE), "-o", str(exe)]
    subprocess.run(plain, check=True)                                    # (the program itself compiles: a failure below is the runtime's)
    build = subprocess.run(plain + ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"], capture_output=True, text=True)
    sanitized = build.returncode == 0
    if not sanitized:
        subprocess.run(plain, check=True)                                # no sanitizer runtime: the plain program again
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-4000:]
    lines = {}
    pending = None
    for line in run.stdout.splitlines():
        head, _, tail = line.partition(":")
        key = tuple(head.split())
        values = [int(v) for v in tail.split()]
        if key[0] == "state":
            lines[pending + ("state",)] = [int(v) for v in key[1:]]
        elif key[0] == "longest":
            lines[("longest",)] = int(key[2])
        else:
            assert key not in lines, key
            lines[key] = values
            pending = key
    print(f"sanitizers: {'address,undefined' if sanitized else 'none (no runtime)'}; {len(lines)} records; longest walk {lines[('longest',)]}")
    return lines


def test_permutations_and_walk_lengths_equal_the_spec(printed):
    seen, longest = 0, 0
    for key, got in printed.items():
        if key[0] != "perm":
            continue
        seed, M, epoch = (int(v) for v in key[1:])
        pi, steps = perm_spec(M, seed, epoch, want_steps=True)
        assert got == pi.tolist(), key
        assert printed[("walk",) + key[1:]] == steps.tolist(), key
        longest = max(longest, int(steps.max()))
        seen += 1
    assert {int(k[2]) for k in printed if k[0] == "perm"} == set(M_LIST)
    assert seen >= 2 * 26 * 4 + 3 * 3 and printed[("longest",)] == longest
    print(f"{seen} permutations; the longest walk over the cases: {longest}")


def test_draws_and_states_equal_the_spec(printed):
    seen = junk = 0
    for key, got in printed.items():
        if key[0] != "draw" or key[-1] == "state":
            continue
        seed, M, B, epoch, cursor = (int(v) for v in key[1:])
        state = np.array([epoch, cursor, 0, 0], np.int64)
        assert got == draw_spec(M, B, seed, state).tolist(), key
        advance_spec(state, B, M)
        assert printed[key + ("state",)] == state[:2].tolist(), key
        seen += 1
        junk += cursor < 0 or cursor >= M
    assert seen >= 2 * 7 * 8 and junk >= 2 * 7 * 4


def test_row_places_and_empty_units(printed):
    for key, got in printed.items():
        if key[0] == "row":
            E, j = int(key[1]), int(key[2])
            assert got == [int(j < E), j if j < E else j - E, 0, j], key
        if key[0] == "empty":
            N = int(key[1])
            consts = (5.0, 6.0, 7.0, 8.0)                                 # kinds: 0 -> (0, 0), 1 -> (5, 6), 2 -> (7, 8), 3 -> (-1, -1)
            rows = rows_spec(np.zeros((N, 4), np.float32), consts).reshape(-1, 2)
            value = {0: [0.0, 0.0], 1: [5.0, 6.0], 2: [7.0, 8.0], 3: [-1.0, -1.0]}
            assert [value[k] for k in got] == rows.tolist(), key
    assert ("empty", "4") in printed and ("row", "5", "14") in printed
