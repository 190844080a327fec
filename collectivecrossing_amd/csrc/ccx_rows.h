// ccx_rows.h -- how a wave moves its 64 rows of five f32 (logits in, gradients out) between global memory and its lanes:
// the LDS scheme of ccx_sample.hip, shared by ccx_evaluate.hip and ccx_ppo_loss.hip.  Device code only.
//
// One lane owns one row; wave number `wave` of the launch takes rows 64 wave .. 64 wave + 63.
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

// The wave's rows through LDS into l[5] of each lane.  M >= 1 rows of five floats at `src` (16-byte aligned), floats = 5 M,
// last_piece = floats / 4 - 1 (at least one whole piece).  Returns with the pieces read back; surplus lanes (row >= M) hold
// the last whole piece's neighbourhood, never anything out of bounds.
__device__ __forceinline__ void load_rows(const float* rows, long long M, float4 (&pieces)[80], uint32_t lane, long long wave,
                                          long long row, long long floats, long long last_piece, float (&l)[5]) {
    const float4* src = reinterpret_cast<const float4*>(rows);
    const long long p0 = wave * 80 + lane, p1 = wave * 80 + 64 + (lane & 15u);
    const float4 v0 = src[p0 < last_piece ? p0 : last_piece];
    const float4 v1 = src[p1 < last_piece ? p1 : last_piece];          // (lanes 16-63 repeat the lines of lanes 0-15)
    pieces[lane] = v0;
    pieces[64 + (lane & 15u)] = v1;                                     // (the four lanes of an address write the same bytes)
    __syncthreads();
    const float* mine = reinterpret_cast<const float*>(pieces) + 5 * lane;
#pragma unroll
    for (int k = 0; k < 5; ++k) l[k] = mine[k];
    if (row == M - 1) {                                                 // one lane of the launch, and only where 5 M % 4 != 0
        const int whole = 5 - (int)(floats & 3);
#pragma unroll
        for (int k = 2; k < 5; ++k)
            if (k >= whole) l[k] = rows[row * 5 + k];
    }
}

// g[5] of each lane with row < M through LDS to `dst` (16-byte aligned), after load_rows on the same pieces.
__device__ __forceinline__ void store_rows(float* rows, long long M, float4 (&pieces)[80], uint32_t lane, long long wave,
                                           long long row, long long floats, long long last_piece, const float (&g)[5]) {
    // each lane overwrites the 20 bytes it read its own row from; surplus lanes write nothing (what lies there belongs to
    // pieces behind the last whole one, which are not stored)
    float* mine = reinterpret_cast<float*>(pieces) + 5 * lane;
    if (row < M) {
#pragma unroll
        for (int k = 0; k < 5; ++k) mine[k] = g[k];
    }
    __syncthreads();
    float4* dst = reinterpret_cast<float4*>(rows);
    const long long p0 = wave * 80 + lane, p1 = wave * 80 + 64 + lane;
    if (p0 <= last_piece) dst[p0] = pieces[lane];
    if (lane < 16u && p1 <= last_piece) dst[p1] = pieces[64 + lane];
    if (row == M - 1) {                                                 // the floats behind the last whole piece
        const int whole = 5 - (int)(floats & 3);
#pragma unroll
        for (int k = 2; k < 5; ++k)
            if (k >= whole) rows[row * 5 + k] = g[k];
    }
}

}  // namespace ccx_rows
