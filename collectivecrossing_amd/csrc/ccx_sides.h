// ccx_sides.h -- the index map of CCX_SIDES (include/ccx.h): which rows of an [M][N][..] array a group of agent slots owns,
// in which order, and which workgroup and lane of a launch carries which of them.  Included by ccx_sides.hip and by the
// sides kernel of ccx_mlp_backward.hip, which inline exactly these functions; it also compiles with a plain host C++
// compiler (tests/test_sides_host_rule.py walks every (workgroup, lane) against a NumPy statement of "selected rows").
// Plain C++17: no HIP type, no global state, integers only.
//
// A group is a 64-bit slot mask (bit a = agent slot a) with S = popcount set bits.  Its SELECTED rows of an array of M * N
// flat rows are m * N + a for every m and every set bit a, in ascending flat index; selection index j = m * S + i names the
// i-th set bit of env-row m.  A launch cuts every group's M * S selected rows into tiles of 64 (forward, draw) or blocks of
// 256 (backward); the tiles of the groups follow each other in table order, so a workgroup carries rows of ONE group and
// whatever depends on the group (the weights' addresses) is uniform over it.
#pragma once
#include <stdint.h>

#ifndef CCX_HD
#if defined(__HIPCC__)
#define CCX_HD __host__ __device__ __forceinline__
#else
#define CCX_HD inline
#endif
#endif

namespace ccx_sides {

constexpr int kMaxGroups = 8;                                            // CCX_SIDES_MAX_GROUPS
constexpr int kTileRows = 64;                                            // selected rows to a workgroup of the forward / draw

// one row of the table: ccx_slot_group's layout (40 bytes); w1t == null marks the head-less group of the draw (unowned slots)
struct Group {
    uint64_t slots;
    const float* w1t;
    const float* b1;
    const float* w2;
    const float* b2;
};

// the table as it travels in the kernel arguments: the groups (and, in the draw, one head-less group behind them) and the
// first workgroup of each; first[num] is the grid
struct Table {
    Group g[kMaxGroups + 1];
    uint32_t first[kMaxGroups + 2];
    int32_t num;
    int32_t pad;
};

CCX_HD int popcount(uint64_t mask) { return __builtin_popcountll(mask); }

// the index of the i-th set bit of mask, 0 <= i < popcount(mask): drop the i lowest set bits, count the zeros below the next
CCX_HD int nth_slot(uint64_t mask, int i) {
    for (; i > 0; --i) mask &= mask - 1;
    return __builtin_ctzll(mask);
}

// tiles of `per` selected rows a group of S slots has over M env-rows
CCX_HD long long tiles_of(long long M, int S, int per) { return (M * S + per - 1) / per; }

// The prefix counts of a table whose `num` groups are set, for tiles of `per` selected rows: first[k] is group k's first
// workgroup, first[num] the grid, which is also returned (it may exceed 32 bits: the caller checks before it launches).
CCX_HD long long set_first(Table& tab, long long M, int per) {
    long long first = 0;
    for (int k = 0; k < tab.num; ++k) {
        tab.first[k] = (uint32_t)first;
        first += tiles_of(M, popcount(tab.g[k].slots), per);
    }
    tab.first[tab.num] = (uint32_t)first;
    return first;
}

// Workgroup w of the launch (0 <= w < first[num]): its group and its tile within the group.  A scan of at most nine prefix
// counts; w is uniform over a workgroup, so on the device this is scalar work.
CCX_HD void locate(const uint32_t* first, int num, uint32_t w, int& group, uint32_t& tile) {
    group = 0;
    tile = w;
    for (int k = 0; k < num; ++k) {
        if (w >= first[k]) {
            group = k;
            tile = w - first[k];
        }
    }
}

// Where a run of selection indices starts: j0 = m0 * S + i0 with 0 <= i0 < S.  j0 is uniform (a tile's or a sub-tile's
// first index), so the one 64-bit division is paid once per wave; what a lane adds stays in 32 bits.
struct Start {
    long long m0;
    uint32_t i0;
};
CCX_HD Start start_of(long long j0, int S) {
    const long long m0 = j0 / S;
    return Start{m0, (uint32_t)(j0 - m0 * S)};
}

// Selection index j0 + off (0 <= off < 2^20): env-row m, slot a, flat row m * N + a.
struct Row {
    long long m, row;
    uint32_t a;
};
CCX_HD Row row_of(uint64_t mask, int S, int N, const Start& s, uint32_t off) {
    const uint32_t t = s.i0 + off, q = t / (uint32_t)S, i = t - q * (uint32_t)S;
    const long long m = s.m0 + q;
    const uint32_t a = (uint32_t)nth_slot(mask, (int)i);
    return Row{m, m * N + a, a};
}

// Lane `lane` of tile `tile` of a group: how many of the tile's rows exist (nr, 1..per), and the lane's row.  A surplus lane
// of the tail tile (lane >= nr) repeats the tile's last row: it may load what that row loads and must store nothing.
CCX_HD int tile_rows(long long M, int S, long long tile, int per) {
    const long long left = M * S - tile * per;
    return left < per ? (int)left : per;
}
CCX_HD Row lane_row(uint64_t mask, int S, long long M, int N, long long tile, int per, uint32_t lane) {
    const int nr = tile_rows(M, S, tile, per);
    return row_of(mask, S, N, start_of(tile * per, S), (int)lane < nr ? lane : (uint32_t)(nr - 1));
}

// What a call's table must satisfy: 1..kMaxGroups groups, every mask non-empty, without a bit at or above N, and pairwise
// disjoint.  0 when it does, else which rule fails (1: the count, 2: an empty mask, 3: a bit at or above N, 4: an overlap)
// and, in `which`, the first group that breaks it.
CCX_HD int check_masks(const uint64_t* masks, int num, int N, int& which) {
    which = 0;
    if (num < 1 || num > kMaxGroups) return 1;
    const uint64_t all = N >= 64 ? ~(uint64_t)0 : (((uint64_t)1 << N) - 1);
    uint64_t seen = 0;
    for (int k = 0; k < num; ++k) {
        which = k;
        if (masks[k] == 0) return 2;
        if (masks[k] & ~all) return 3;
        if (masks[k] & seen) return 4;
        seen |= masks[k];
    }
    return 0;
}

}  // namespace ccx_sides
