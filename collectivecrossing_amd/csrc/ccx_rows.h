// ccx_rows.h -- how a wave moves its 64 rows of W f32 (W = 5: logits or Q-values in, gradients out; W = 6: the rows of a
// dueling head, CCX_DUELING) between global memory and its lanes.  One LDS scheme for the kernels that take such rows from
// memory: sample_kernel (ccx_sample.hip), evaluate_fwd_kernel / evaluate_bwd_kernel (ccx_evaluate.hip), ppo_partial_kernel /
// ppo_bwd_kernel (ccx_ppo_loss.hip), q_act_kernel / td_partial_kernel / td_bwd_kernel (ccx_qlearn.hip) and dueling_fwd_kernel /
// dueling_bwd_kernel (ccx_dueling.hip).  Device code only.  W is a template parameter with the default 5: what is said
// below for five holds for six with 24 bytes, 96 pieces and lanes 0-31 in the place of 20, 80 and lanes 0-15.
//
// One lane owns one row; wave number `wave` of the launch takes rows 64 wave .. 64 wave + 63 (Wave, below: what a lane knows
// about its place, derived once from M, the wave and the lane).
// Loads.  A wave's rows are 1280 contiguous bytes at a lane stride of 20; its 80 16-byte pieces are loaded whole (lanes 0-63
// one each, lanes 0-15 a second one), written to LDS as they are, and each lane reads back its five dwords at a stride of
// 5 dwords (odd: the 32 lanes of a lane group hit 32 banks; six dwords at a stride of 6 are three aligned 8-byte reads).
// Every load is unconditional at a clamped index; the up to three floats behind the last whole piece are fetched as dwords
// by the last row's lane.
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

// A lane's place among M >= 1 rows of W floats: its wave of the launch (a workgroup of several waves passes its global
// wave number), its row, the row its small loads are clamped to (the tail wave's surplus lanes load what the last row
// loads), and the extent of the rows in floats and in whole 16-byte pieces (at least one).
template <int W = 5>
struct WaveT {
    static_assert(W == 5 || W == 6, "a wave's pieces behind the first 64 are 16 (W - 4): a power of two for rows of 5 and 6");
    long long M, wave, row, rl, floats, last_piece;
    uint32_t lane;
};
using Wave = WaveT<5>;

template <int W = 5>
__device__ __forceinline__ WaveT<W> wave_of(long long M, long long wave, uint32_t lane) {
    const long long row = wave * 64 + lane;
    const long long rl = row < M ? row : M - 1;
    const long long floats = M * W, last_piece = floats / 4 - 1;
    return WaveT<W>{M, wave, row, rl, floats, last_piece, lane};
}

// The wave's rows at `rows` (16-byte aligned) through LDS into l[W] of each lane.  Returns with the pieces read back;
// surplus lanes (row >= M) hold the last whole piece's neighbourhood, never anything out of bounds.
template <int W>
__device__ __forceinline__ void load_rows(const float* rows, float4 (&pieces)[16 * W], const WaveT<W>& Wv, float (&l)[W]) {
    constexpr uint32_t kMore = 16u * W - 64u;                           // the pieces behind the first 64: 16 (W = 5) or 32 (W = 6)
    const float4* src = reinterpret_cast<const float4*>(rows);
    const long long p0 = Wv.wave * (16 * W) + Wv.lane, p1 = Wv.wave * (16 * W) + 64 + (Wv.lane & (kMore - 1u));
    const float4 v0 = src[p0 < Wv.last_piece ? p0 : Wv.last_piece];
    const float4 v1 = src[p1 < Wv.last_piece ? p1 : Wv.last_piece];    // (the lanes behind kMore repeat the lines of the first ones)
    pieces[Wv.lane] = v0;
    pieces[64 + (Wv.lane & (kMore - 1u))] = v1;                         // (the lanes of an address write the same bytes)
    __syncthreads();
    const float* mine = reinterpret_cast<const float*>(pieces) + W * Wv.lane;
#pragma unroll
    for (int k = 0; k < W; ++k) l[k] = mine[k];
    if (Wv.row == Wv.M - 1) {                                           // one lane of the launch, and only where W M % 4 != 0
        const int whole = W - (int)(Wv.floats & 3);
#pragma unroll
        for (int k = W - 3; k < W; ++k)
            if (k >= whole) l[k] = rows[Wv.row * W + k];
    }
}

// g[W] of each lane with row < M through LDS to `rows` (16-byte aligned).  The pieces are those of a load_rows of the same
// W before it (each lane overwrites the bytes it read its own row from), or pieces that no lane reads any more.
template <int W>
__device__ __forceinline__ void store_rows(float* rows, float4 (&pieces)[16 * W], const WaveT<W>& Wv, const float (&g)[W]) {
    constexpr uint32_t kMore = 16u * W - 64u;
    // each lane overwrites the W dwords of its own row; surplus lanes write nothing (what lies there belongs to
    // pieces behind the last whole one, which are not stored)
    float* mine = reinterpret_cast<float*>(pieces) + W * Wv.lane;
    if (Wv.row < Wv.M) {
#pragma unroll
        for (int k = 0; k < W; ++k) mine[k] = g[k];
    }
    __syncthreads();
    float4* dst = reinterpret_cast<float4*>(rows);
    const long long p0 = Wv.wave * (16 * W) + Wv.lane, p1 = Wv.wave * (16 * W) + 64 + Wv.lane;
    if (p0 <= Wv.last_piece) dst[p0] = pieces[Wv.lane];
    if (Wv.lane < kMore && p1 <= Wv.last_piece) dst[p1] = pieces[64 + Wv.lane];
    if (Wv.row == Wv.M - 1) {                                           // the floats behind the last whole piece
        const int whole = W - (int)(Wv.floats & 3);
#pragma unroll
        for (int k = W - 3; k < W; ++k)
            if (k >= whole) rows[Wv.row * W + k] = g[k];
    }
}

}  // namespace ccx_rows
