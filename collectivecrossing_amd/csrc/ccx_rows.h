// ccx_rows.h -- how a wave moves its 64 rows of five f32 (logits or Q-values in, gradients out) between global memory and
// its lanes.  One LDS scheme for the eight kernels that take such rows from memory: sample_kernel (ccx_sample.hip),
// evaluate_fwd_kernel / evaluate_bwd_kernel (ccx_evaluate.hip), ppo_partial_kernel / ppo_bwd_kernel (ccx_ppo_loss.hip) and
// q_act_kernel / td_partial_kernel / td_bwd_kernel (ccx_qlearn.hip).  Device code only.
//
// One lane owns one row; wave number `wave` of the launch takes rows 64 wave .. 64 wave + 63 (Wave, below: what a lane knows
// about its place, derived once from M, the wave and the lane).
// Loads.  A wave's rows are 1280 contiguous bytes at a lane stride of 20; its 80 16-byte pieces are loaded whole (lanes 0-63
// one each, lanes 0-15 a second one), written to LDS as they are, and each lane reads back its five dwords at a stride of
// 5 dwords (odd: the 32 lanes of a lane group hit 32 banks).  Every load is unconditional at a clamped index; the up to three
// floats behind the last whole piece are fetched as dwords by the last row's lane.
// Stores: the mirror image.  Each lane writes its five values to LDS where it read its row (the lane's own 20 bytes: no
// other lane's row is overwritten), then the wave stores whole pieces, lanes 0-63 one each and lanes 0-15 a second one:
// every 128-byte line of the wave's 1280 bytes is written whole by two global_store_dwordx4, not touched by five
// global_store_dword at a 20-byte stride.  Only pieces that lie entirely inside 5 M floats are stored; the up to three
// floats behind the last whole piece are stored as dwords by the last row's lane.
// Both functions hold a __syncthreads(): every wave of the workgroup calls them, each with its own 80 pieces of LDS.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace ccx_rows {

// A lane's place among M >= 1 rows of five floats: its wave of the launch (a workgroup of several waves passes its global
// wave number), its row, the row its small loads are clamped to (the tail wave's surplus lanes load what the last row
// loads), and the extent of the rows in floats and in whole 16-byte pieces (at least one).
struct Wave {
    long long M, wave, row, rl, floats, last_piece;
    uint32_t lane;
};

__device__ __forceinline__ Wave wave_of(long long M, long long wave, uint32_t lane) {
    const long long row = wave * 64 + lane;
    const long long rl = row < M ? row : M - 1;
    const long long floats = M * 5, last_piece = floats / 4 - 1;
    return Wave{M, wave, row, rl, floats, last_piece, lane};
}

// The wave's rows at `rows` (16-byte aligned) through LDS into l[5] of each lane.  Returns with the pieces read back;
// surplus lanes (row >= M) hold the last whole piece's neighbourhood, never anything out of bounds.
__device__ __forceinline__ void load_rows(const float* rows, float4 (&pieces)[80], const Wave& W, float (&l)[5]) {
    const float4* src = reinterpret_cast<const float4*>(rows);
    const long long p0 = W.wave * 80 + W.lane, p1 = W.wave * 80 + 64 + (W.lane & 15u);
    const float4 v0 = src[p0 < W.last_piece ? p0 : W.last_piece];
    const float4 v1 = src[p1 < W.last_piece ? p1 : W.last_piece];      // (lanes 16-63 repeat the lines of lanes 0-15)
    pieces[W.lane] = v0;
    pieces[64 + (W.lane & 15u)] = v1;                                   // (the four lanes of an address write the same bytes)
    __syncthreads();
    const float* mine = reinterpret_cast<const float*>(pieces) + 5 * W.lane;
#pragma unroll
    for (int k = 0; k < 5; ++k) l[k] = mine[k];
    if (W.row == W.M - 1) {                                             // one lane of the launch, and only where 5 M % 4 != 0
        const int whole = 5 - (int)(W.floats & 3);
#pragma unroll
        for (int k = 2; k < 5; ++k)
            if (k >= whole) l[k] = rows[W.row * 5 + k];
    }
}

// g[5] of each lane with row < M through LDS to `rows` (16-byte aligned), after load_rows on the same pieces.
__device__ __forceinline__ void store_rows(float* rows, float4 (&pieces)[80], const Wave& W, const float (&g)[5]) {
    // each lane overwrites the 20 bytes it read its own row from; surplus lanes write nothing (what lies there belongs to
    // pieces behind the last whole one, which are not stored)
    float* mine = reinterpret_cast<float*>(pieces) + 5 * W.lane;
    if (W.row < W.M) {
#pragma unroll
        for (int k = 0; k < 5; ++k) mine[k] = g[k];
    }
    __syncthreads();
    float4* dst = reinterpret_cast<float4*>(rows);
    const long long p0 = W.wave * 80 + W.lane, p1 = W.wave * 80 + 64 + W.lane;
    if (p0 <= W.last_piece) dst[p0] = pieces[W.lane];
    if (W.lane < 16u && p1 <= W.last_piece) dst[p1] = pieces[64 + W.lane];
    if (W.row == W.M - 1) {                                             // the floats behind the last whole piece
        const int whole = 5 - (int)(W.floats & 3);
#pragma unroll
        for (int k = 2; k < 5; ++k)
            if (k >= whole) rows[W.row * 5 + k] = g[k];
    }
}

}  // namespace ccx_rows
