// ccx_mlp_tile.h -- the workgroup tile of CCX_MLP's forward (include/ccx.h): 64 rows through both layers, by ccx_mlp.h's
// per-row functions.  Shared by ccx_mlp.hip (64 ADJACENT rows of a [rows][L] array) and ccx_sides.hip (64 SELECTED rows of
// one slot group, ccx_sides.h): which 64 rows a tile holds, how their x reaches LDS and where their outputs go is a `Rows`
// argument; everything between -- the mapping of hidden units to waves, the chains, the layer-2 order -- is stated once here,
// so "the rows of a group get exactly CCX_MLP's outputs" holds because both run this.  Device code, and the host's helpers
// for the launch (LDS size, the opt-in above 64 KB, the shape check).
//
// Mapping.  A workgroup takes 64 rows and has G = H / 16 waves; lane l of every wave owns row l of the tile, wave g owns hidden
// units 16 g .. 16 g + 15 -- one group of the layer-2 order.  So the 16 accumulators of a lane are its whole register state,
// every row's chain is split over G waves, and the order of operations is the header's for any G.
// Loads.  The x tile sits in LDS row by row at a row stride of L | 1 dwords: odd, so the 64 lanes of a wave, which read the
// same k of 64 different rows, hit different banks.  `Rows::load_x` fills it.
// Weights.  w1t[k][16 g ..], b1, w2[o][16 g ..] and b2 have wave-uniform addresses (g comes through readfirstlane): the
// compiler reads them with scalar loads into SGPRs, once per wave, not 64 times.
// Layer 2.  Wave g writes its O partials per row to LDS (over the x tile, behind a barrier); then the 64 O sums of the tile
// are spread over all threads in the flat order of the tile's y: item i = row * O + o adds the G partials in group order and
// stores at `Rows::y_index`.  With KEEP the tile's y also stays in LDS for a fused consumer.
#pragma once
#include "ccx_internal.h"
#include "ccx_mlp.h"

namespace ccx_tile {

struct MlpArgs {
    const float* x;                    // [rows][L]
    const float* w1t;                  // [L][H]
    const float* b1;                   // [H]
    const float* w2;                   // [O][H]
    const float* b2;                   // [O]
    float* y;                          // [rows][O]; may be null in the fused kernels
    float* hidden;                     // [rows][H] or null
    long long rows;
    int32_t L, H, O, activation;
};

using ccx_mlp::lds_floats;                                               // the LDS floats a workgroup needs (ccx_mlp.h)

// The tile of workgroup blockIdx.x of a launch over ceil(rows / 64) workgroups: rows 64 b .. 64 b + 63 of the array.
// The tile's x is 64 L contiguous floats that start at a multiple of 64 floats: its 16 L 16-byte pieces are loaded whole by
// all waves (coalesced global_load_dwordx4, every byte fetched once, indices clamped to the array's last whole piece).
// rows * L need not be a multiple of 4: the up to three floats behind the last whole piece are fetched as dwords by the last
// workgroup.  x must be 16-byte aligned.
struct AdjacentRows {
    long long r0;
    int nr;
    __device__ __forceinline__ void begin(const MlpArgs& A) {
        r0 = (long long)blockIdx.x * 64;
        const long long left = A.rows - r0;
        nr = left < 64 ? (int)left : 64;
    }
    __device__ __forceinline__ void load_x(const MlpArgs& A, float* lds, uint32_t tid, int T) const {
        const int L = A.L, Lp = L | 1;
        // whole pieces through all threads, indices clamped to the array's last whole piece
        const long long floats = A.rows * L, last_piece = floats / 4 - 1, tile_p0 = (long long)blockIdx.x * 16 * L;
        if (last_piece >= 0) {
            const float4* src = reinterpret_cast<const float4*>(A.x);
            for (int p = (int)tid; p < 16 * L; p += T) {
                const long long gp = tile_p0 + p;
                const float4 v = src[gp < last_piece ? gp : last_piece];
                const float f[4] = {v.x, v.y, v.z, v.w};
                uint32_t r = (uint32_t)(4 * p) / (uint32_t)L, k = (uint32_t)(4 * p) - r * (uint32_t)L;
                const bool whole = gp <= last_piece;
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    if (whole) lds[r * (uint32_t)Lp + k] = f[i];              // (r <= 63: the tile has 64 L floats)
                    ++k;
                    if (k == (uint32_t)L) {
                        k = 0;
                        ++r;
                    }
                }
            }
        }
        const int ntail = (int)(floats & 3);
        if (blockIdx.x == gridDim.x - 1 && (int)tid < ntail) {               // the floats behind the last whole piece: this tile's
            const long long fi = floats - ntail + tid;
            const uint32_t lf = (uint32_t)(fi - r0 * L), r = lf / (uint32_t)L, k = lf - r * (uint32_t)L;
            lds[r * (uint32_t)Lp + k] = A.x[fi];
        }
    }
    __device__ __forceinline__ long long row(uint32_t lane) const { return r0 + lane; }               // lane < nr
    __device__ __forceinline__ long long y_index(const MlpArgs& A, int i, int) const { return r0 * A.O + i; }
};

// The tile Rows describes: y (and hidden) written, and with KEEP the tile's y left in LDS at the returned pointer (valid
// behind the caller's barrier).  Rows: begin(A) sets the tile up (nr, the rows that exist, 1..64); load_x(A, lds, tid, T)
// brings x of rows 0 .. nr - 1 to lds[r * (L | 1) + k] over the T threads (the barrier behind it is mlp_tile's); row(lane) is
// the array row of tile row `lane` < nr (for hidden); y_index(A, i, o) is where item i = r * O + o of the tile's y goes.
template <bool KEEP, class Rows>
__device__ __forceinline__ float* mlp_tile(const MlpArgs& A, Rows R, float* lds) {
    const uint32_t tid = threadIdx.x, lane = tid & 63u;
    const int g = __builtin_amdgcn_readfirstlane((int)(tid >> 6));
    const int L = A.L, H = A.H, O = A.O, G = H / ccx_mlp::kGroup, T = G * 64, Lp = L | 1;
    R.begin(A);
    const int nr = R.nr;
    // 1. the x tile
    R.load_x(A, lds, tid, T);
    __syncthreads();
    // 2. layer 1: this wave's 16 units of the lane's row (surplus lanes of the tail tile repeat its last row)
    const uint32_t rl = (int)lane < nr ? lane : (uint32_t)(nr - 1);
    const float* xr = lds + rl * (uint32_t)Lp;
    const float* wg = A.w1t + ccx_mlp::kGroup * g;
    float a[ccx_mlp::kGroup];
#pragma unroll
    for (int j = 0; j < ccx_mlp::kGroup; ++j) a[j] = A.b1[ccx_mlp::kGroup * g + j];
#pragma unroll 2
    for (int k = 0; k < L; ++k) ccx_mlp::layer1_step(a, xr[k], wg + (long long)k * H);
    if (A.activation == ccx_mlp::kRelu) {
#pragma unroll
        for (int j = 0; j < ccx_mlp::kGroup; ++j) a[j] = ccx_mlp::relu_spec(a[j]);
    } else {
#pragma unroll
        for (int j = 0; j < ccx_mlp::kGroup; ++j) a[j] = ccx_mlp::tanh_spec(a[j]);
    }
    if (A.hidden && (int)lane < nr) {
        float4* hp = reinterpret_cast<float4*>(A.hidden + R.row(lane) * H + ccx_mlp::kGroup * g);
#pragma unroll
        for (int q = 0; q < 4; ++q) hp[q] = make_float4(a[4 * q], a[4 * q + 1], a[4 * q + 2], a[4 * q + 3]);
    }
    __syncthreads();                                                      // every wave has read its x: the tile may go
    // 3. layer 2: the partials of this wave's group, [G][64][O] in LDS
    const int per = 64 * O;
    for (int o = 0; o < O; ++o) lds[g * per + (int)lane * O + o] = ccx_mlp::layer2_partial(a, A.w2 + o * H + ccx_mlp::kGroup * g);
    __syncthreads();
    // 4. the tile's 64 O sums in the flat order of y, over all threads
    float* ykeep = lds + G * per;
    const int valid = nr * O;
    for (int i = (int)tid; i < per; i += T) {
        const int o = i % O;
        const float y = ccx_mlp::layer2_sum(A.b2[o], lds + i, G, per);
        if (A.y && i < valid) A.y[R.y_index(A, i, o)] = y;
        if (KEEP) ykeep[i] = y;
    }
    return ykeep;
}

// Workgroups of more than 64 KB of LDS (L > 255) are opted into before the launch.
template <typename K>
hipError_t allow_lds(K kernel, size_t bytes) {
    if (bytes <= 65536) return hipSuccess;
    return hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
}

inline int check_dims(const char* who, int32_t L, int32_t H, int32_t O, int32_t activation) {
    if (!ccx_mlp::shape_ok(L, H, O, activation))
        return ccxi::fail(CCX_EINVAL, "%s: L = %d, H = %d, O = %d, activation = %d: 1 <= L <= %d, H a multiple of 16 in 16..%d, 1 <= O <= %d and "
                          "activation 0 (tanh) or 1 (relu) are required", who, L, H, O, activation, ccx_mlp::kMaxL, ccx_mlp::kMaxH, ccx_mlp::kMaxO);
    return CCX_OK;
}

}  // namespace ccx_tile
