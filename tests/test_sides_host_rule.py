"""The index map of csrc/ccx_sides.h -- the very source the kernels of CCX_SIDES inline -- compiled for the host and walked
over every (workgroup, lane) of a launch against a NumPy statement of "selected rows": every selected row of every group
exactly once, in ascending order within its group, surplus lanes of tail tiles marked and repeating the tile's last row, and
the prefix counts the host side launches with.  Tiles of 64 (forward, draw) and of 256 (backward).  No GPU."""

import ctypes as C
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "collectivecrossing_amd" / "csrc"
NS = (1, 3, 8, 32, 64)
MS = (1, 2, 63, 64, 65, 300)


def selected_rows(mask: int, M: int, N: int) -> np.ndarray:
    """THE statement: flat rows m * N + a for every m and every set bit a, m-major, then a ascending."""
    slots = np.array([a for a in range(N) if mask >> a & 1], np.int64)
    return (np.arange(M, dtype=np.int64)[:, None] * N + slots[None, :]).ravel()


def random_groups(rng, N: int, num: int) -> list[int]:
    """`num` non-empty, pairwise disjoint masks over N slots (num <= N); some slots stay unowned."""
    owner = rng.integers(-1, num, size=N)
    owner[rng.permutation(N)[:num]] = np.arange(num)                      # every group owns at least one slot
    return [int(sum(1 << a for a in range(N) if owner[a] == k)) for k in range(num)]


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
    so = tmp_path_factory.mktemp("sides_host_rule") / "libsides_host_rule.so"
    subprocess.run([cxx, "-std=c++17", "-O2", "-fPIC", "-shared", f"-I{CSRC}", str(Path(__file__).with_name("sides_host_rule.cpp")),
                    "-o", str(so)], check=True)
    lib = C.CDLL(str(so))
    lib.host_sides_grid.restype = C.c_longlong
    lib.host_sides_walk.restype = None
    lib.host_sides_check.restype = C.c_int
    return lib


def _walk(host, masks, M, N, per):
    num = len(masks)
    arr = (C.c_uint64 * num)(*masks)
    first = np.zeros(num + 1, np.uint32)
    grid = host.host_sides_grid(C.c_int(num), arr, C.c_longlong(M), C.c_int(per), first.ctypes.data_as(C.c_void_p))
    n = grid * per
    group, slot = np.full(n, -1, np.int32), np.full(n, -1, np.int32)
    row, env_row = np.full(n, -1, np.int64), np.full(n, -1, np.int64)
    live = np.full(n, 7, np.uint8)
    host.host_sides_walk(C.c_int(num), arr, C.c_longlong(M), C.c_int(N), C.c_int(per), first.ctypes.data_as(C.c_void_p),
                         *(a.ctypes.data_as(C.c_void_p) for a in (group, row, env_row, slot, live)))
    return grid, first, group, row, env_row, slot, live


@pytest.mark.parametrize("per", (64, 256))
@pytest.mark.parametrize("N", NS)
def test_the_map_hits_every_selected_row_once_and_in_order(host, N, per):
    rng = np.random.default_rng(1000 * N + per)
    for num in range(1, min(8, N) + 1):
        for M in MS:
            masks = random_groups(rng, N, num)
            grid, first, group, row, env_row, slot, live = _walk(host, masks, M, N, per)
            tiles = [-(-M * bin(m).count("1") // per) for m in masks]
            assert grid == sum(tiles)
            np.testing.assert_array_equal(first, np.concatenate([[0], np.cumsum(tiles)]))
            assert set(np.unique(live)) <= {0, 1}
            # a workgroup carries one group: the groups' tiles follow each other in table order
            np.testing.assert_array_equal(group.reshape(grid, per), np.repeat(np.arange(num), tiles)[:, None].repeat(per, 1))
            for k, mask in enumerate(masks):
                want = selected_rows(mask, M, N)
                mine = group == k
                got = row[mine & (live == 1)]
                np.testing.assert_array_equal(got, want, err_msg=f"N={N} M={M} masks={masks} group {k}")
                np.testing.assert_array_equal(env_row[mine & (live == 1)], want // N)
                np.testing.assert_array_equal(slot[mine & (live == 1)], want % N)
                # surplus lanes: only in the group's last tile, behind the live ones, repeating the last selected row
                surplus = mine & (live == 0)
                assert surplus.sum() == tiles[k] * per - want.size
                assert (row[surplus] == want[-1]).all()
                idx = np.flatnonzero(surplus)
                assert idx.size == 0 or idx[0] == (first[k + 1] * per - idx.size)


def test_the_two_sides_and_a_full_mask(host):
    for nb, ne, M in ((5, 3, 13), (2, 1, 64), (16, 16, 300), (1, 63, 3)):
        N = nb + ne
        masks = [(1 << nb) - 1, ((1 << N) - 1) & ~((1 << nb) - 1)]
        grid, first, group, row, _, _, live = _walk(host, masks, M, N, 64)
        both = np.sort(row[live == 1])
        np.testing.assert_array_equal(both, np.arange(M * N))             # the two sides cover every flat row once
        grid1, _, _, row1, _, _, live1 = _walk(host, [(1 << N) - 1], M, N, 64)
        np.testing.assert_array_equal(row1[live1 == 1], np.arange(M * N))  # "all": the identity map
        assert grid1 == -(-M * N // 64)


def test_check_masks(host):
    def check(masks, N):
        which = C.c_int(-1)
        rc = host.host_sides_check((C.c_uint64 * max(1, len(masks)))(*masks), C.c_int(len(masks)), C.c_int(N), C.byref(which))
        return rc, which.value
    assert check([0b00011, 0b11100], 5) == (0, 1)
    assert check([(1 << 64) - 1], 64)[0] == 0
    assert check([], 5)[0] == 1 and check([1 << k for k in range(9)], 64)[0] == 1
    assert check([0b1, 0], 5) == (2, 1)
    assert check([0b1, 0b100000], 5) == (3, 1)
    assert check([1 << 63], 63) == (3, 0)
    assert check([0b011, 0b100, 0b110], 5) == (4, 2)
