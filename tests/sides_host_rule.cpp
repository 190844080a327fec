// The index map of csrc/ccx_sides.h compiled for the host (tests/test_sides_host_rule.py), behind a C interface for ctypes.
// The loops here only walk workgroups and lanes; every index is one of ccx_sides.h's functions.
#include "ccx_sides.h"

extern "C" {

// first: u32 [num + 1], the prefix counts the host side launches with; returns the grid
long long host_sides_grid(int num, const uint64_t* masks, long long M, int per, uint32_t* first) {
    ccx_sides::Table tab{};
    tab.num = num;
    for (int k = 0; k < num; ++k) tab.g[k].slots = masks[k];
    const long long grid = ccx_sides::set_first(tab, M, per);
    for (int k = 0; k <= num; ++k) first[k] = tab.first[k];
    return grid;
}

// every (workgroup, lane) of the launch: its group, its flat row, env-row and slot, and whether the lane is live
void host_sides_walk(int num, const uint64_t* masks, long long M, int N, int per, const uint32_t* first, int* group, long long* row,
                     long long* env_row, int* slot, unsigned char* live) {
    for (uint32_t w = 0; w < first[num]; ++w) {
        int g;
        uint32_t tile;
        ccx_sides::locate(first, num, w, g, tile);
        const int S = ccx_sides::popcount(masks[g]);
        const int nr = ccx_sides::tile_rows(M, S, tile, per);
        for (int lane = 0; lane < per; ++lane) {
            const ccx_sides::Row r = ccx_sides::lane_row(masks[g], S, M, N, tile, per, (uint32_t)lane);
            const long long at = (long long)w * per + lane;
            group[at] = g;
            row[at] = r.row;
            env_row[at] = r.m;
            slot[at] = (int)r.a;
            live[at] = lane < nr;
        }
    }
}

int host_sides_check(const uint64_t* masks, int num, int N, int* which) { return ccx_sides::check_masks(masks, num, N, *which); }

}  // extern "C"
