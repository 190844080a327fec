// ccx_mlp.hip -- CCX_MLP (include/ccx.h): a two-layer perceptron from observation rows to logits as a fixed sequence of f32
// operations per row, as a kernel of its own (ccx_mlp_forward) and fused with CCX_SAMPLE (ccx_mlp_sample_actions: rows in,
// actions / logp / entropy out, one launch).
//
// Mapping.  A workgroup takes 64 adjacent rows and has G = H / 16 waves; lane l of every wave owns row l of the tile, wave g
// owns hidden units 16 g .. 16 g + 15 -- one group of the layer-2 order.  So the 16 accumulators of a lane are its whole
// register state, every row's chain is split over G waves, and the order of operations is the header's for any G.
// Loads.  The tile's x is 64 L contiguous floats that start at a multiple of 64 floats: its 16 L 16-byte pieces are loaded
// whole by all waves (coalesced global_load_dwordx4, every byte fetched once, indices clamped to the array's last whole
// piece) and written to LDS row by row at a row stride of L | 1 dwords: odd, so the 64 lanes of a wave, which read the same
// k of 64 different rows, hit different banks.  rows * L need not be a multiple of 4: the up to three floats behind the last
// whole piece are fetched as dwords by the last workgroup.  x must be 16-byte aligned.
// Weights.  w1t[k][16 g ..], b1, w2[o][16 g ..] and b2 have wave-uniform addresses (g comes through readfirstlane): the
// compiler reads them with scalar loads into SGPRs, once per wave, not 64 times.
// Layer 2.  Wave g writes its O partials per row to LDS (over the x tile, behind a barrier); then the 64 O sums of the tile
// are spread over all threads in the flat order of y: item i = row * O + o adds the G partials in group order and stores
// y[64 O b + i]: adjacent threads store adjacent dwords.  The fused kernel also keeps y in LDS, and wave 0 then runs
// ccx_softmax.h's sample_slot on its lane's five logits: the same code ccx_sample.hip runs on logits read from memory.
// Arithmetic.  ccx_mlp.h's functions, one f32 operation per line (-ffp-contract=off; `/` is the correctly rounded division,
// asked for on this unit's compile line).
#include "ccx_draw.h"
#include "ccx_mlp.h"

using ccx_draw::DrawArgs;
using ccxi::fail;

namespace {

struct MlpArgs {
    const float* x;                    // [rows][L]
    const float* w1t;                  // [L][H]
    const float* b1;                   // [H]
    const float* w2;                   // [O][H]
    const float* b2;                   // [O]
    float* y;                          // [rows][O]; may be null in the fused kernel
    float* hidden;                     // [rows][H] or null
    long long rows;
    int32_t L, H, O, activation;
};

// LDS floats a workgroup needs: the x tile at its odd row stride, later overlaid by the partials (and y in the fused kernel)
inline size_t lds_floats(int L, int H, int O, bool draw) {
    const size_t tile = (size_t)64 * (size_t)(L | 1), sums = (size_t)(H / ccx_mlp::kGroup + (draw ? 1 : 0)) * 64 * (size_t)O;
    return tile > sums ? tile : sums;
}

// The tile of workgroup blockIdx.x: y (and hidden) written, and with KEEP the tile's y left in LDS at the returned pointer
// (valid behind the caller's barrier).
template <bool KEEP>
__device__ __forceinline__ float* mlp_tile(const MlpArgs& A, float* lds) {
    const uint32_t tid = threadIdx.x, lane = tid & 63u;
    const int g = __builtin_amdgcn_readfirstlane((int)(tid >> 6));
    const int L = A.L, H = A.H, O = A.O, G = H / ccx_mlp::kGroup, T = G * 64, Lp = L | 1;
    const long long r0 = (long long)blockIdx.x * 64, left = A.rows - r0;
    const int nr = left < 64 ? (int)left : 64;
    // 1. the x tile: whole pieces through all threads, indices clamped to the array's last whole piece
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
        float4* hp = reinterpret_cast<float4*>(A.hidden + (r0 + lane) * H + ccx_mlp::kGroup * g);
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
        if (A.y && i < valid) A.y[r0 * O + i] = y;
        if (KEEP) ykeep[i] = y;
    }
    return ykeep;
}

__global__ __launch_bounds__(1024) void mlp_forward_kernel(const MlpArgs A) {
    extern __shared__ float lds[];
    mlp_tile<false>(A, lds);
}

// ccx_sample.hip's kernel with the logits taken from the tile instead of from memory: 64 rows = 64 slots = wave 0's lanes,
// under ccx_draw.h's slot rule.
template <bool DET, bool STATS>
__global__ __launch_bounds__(1024) void mlp_draw_kernel(const MlpArgs A, const DrawArgs D) {
    extern __shared__ float lds[];
    const uint32_t lane = threadIdx.x & 63u;
    const bool first = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)) == 0;
    const ccx_draw::Slot s = ccx_draw::slot_of(D, lane);
    ccx_draw::Small v;
    if (first) v = ccx_draw::small_loads<DET>(D, s, D.masks != nullptr);   // wave 0's small loads, in flight under the layers
    const float* y = mlp_tile<true>(A, lds);
    __syncthreads();
    if (!first || s.slot >= D.EN) return;
    float l[5];
#pragma unroll
    for (int k = 0; k < 5; ++k) l[k] = y[5 * lane + k];
    ccx_draw::finish<DET, STATS>(D, s, v, l);
}

// Workgroups of more than 64 KB of LDS (L > 255) are opted into before the launch.
template <typename K>
hipError_t allow_lds(K kernel, size_t bytes) {
    if (bytes <= 65536) return hipSuccess;
    return hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
}

int check_shape(const char* who, int64_t rows, int32_t L, int32_t H, int32_t O, int32_t activation) {
    if (rows < 1) return fail(CCX_EINVAL, "%s: rows = %lld, at least 1 is required", who, (long long)rows);
    if (rows > (int64_t)0x7FFFFFFF * 64) return fail(CCX_EINVAL, "%s: rows = %lld exceed the grid (2^31 - 1 workgroups of 64 rows)", who, (long long)rows);
    if (!ccx_mlp::shape_ok(L, H, O, activation))
        return fail(CCX_EINVAL, "%s: L = %d, H = %d, O = %d, activation = %d: 1 <= L <= %d, H a multiple of 16 in 16..%d, 1 <= O <= %d and "
                    "activation 0 (tanh) or 1 (relu) are required", who, L, H, O, activation, ccx_mlp::kMaxL, ccx_mlp::kMaxH, ccx_mlp::kMaxO);
    return CCX_OK;
}

}  // namespace

extern "C" {

int ccx_mlp_forward(ccx_handle* h, int64_t rows, int32_t L, int32_t H, int32_t O, int32_t activation, const float* x,
                    const float* w1t, const float* b1, const float* w2, const float* b2, float* y, float* hidden_or_null) {
    if (!h) return fail(CCX_EINVAL, "NULL handle");
    if (!x || !w1t || !b1 || !w2 || !b2 || !y) return fail(CCX_EINVAL, "ccx_mlp_forward: NULL argument (only hidden may be NULL)");
    if (const int rc = check_shape("ccx_mlp_forward", rows, L, H, O, activation)) return rc;
    if ((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(hidden_or_null)) & 15u)
        return fail(CCX_EINVAL, "ccx_mlp_forward: x and hidden must be 16-byte aligned");
    if ((reinterpret_cast<uintptr_t>(w1t) | reinterpret_cast<uintptr_t>(b1) | reinterpret_cast<uintptr_t>(w2) |
         reinterpret_cast<uintptr_t>(b2) | reinterpret_cast<uintptr_t>(y)) & 3u)
        return fail(CCX_EINVAL, "ccx_mlp_forward: w1t, b1, w2, b2 and y must be 4-byte aligned");
    CCX_HIP(hipSetDevice(h->device));
    const MlpArgs A{x, w1t, b1, w2, b2, y, hidden_or_null, (long long)rows, L, H, O, activation};
    const size_t bytes = lds_floats(L, H, O, false) * sizeof(float);
    CCX_HIP(allow_lds(mlp_forward_kernel, bytes));
    hipLaunchKernelGGL(mlp_forward_kernel, dim3((unsigned)((rows + 63) / 64)), dim3(64 * (H / ccx_mlp::kGroup)), bytes, h->stream, A);
    CCX_HIP(hipGetLastError());
    return CCX_OK;
}

int ccx_mlp_sample_actions(ccx_handle* h, int32_t H, int32_t activation, const float* obs, const float* w1t, const float* b1,
                           const float* w2, const float* b2, const uint8_t* masks_or_null, int32_t deterministic, uint8_t* actions,
                           float* logp_or_null, float* entropy_or_null, float* logits_or_null) {
    if (!h) return fail(CCX_EINVAL, "NULL handle");
    if (!obs || !w1t || !b1 || !w2 || !b2 || !actions)
        return fail(CCX_EINVAL, "ccx_mlp_sample_actions: NULL argument (obs, the four parameter arrays and actions are required)");
    const int32_t L = ccx_obs_len(h->N);
    const int64_t rows = (int64_t)h->E * h->N;
    if (const int rc = check_shape("ccx_mlp_sample_actions", rows, L, H, 5, activation)) return rc;
    if (reinterpret_cast<uintptr_t>(obs) & 15u) return fail(CCX_EINVAL, "ccx_mlp_sample_actions: obs must be 16-byte aligned");
    if ((reinterpret_cast<uintptr_t>(w1t) | reinterpret_cast<uintptr_t>(b1) | reinterpret_cast<uintptr_t>(w2) |
         reinterpret_cast<uintptr_t>(b2) | reinterpret_cast<uintptr_t>(logp_or_null) | reinterpret_cast<uintptr_t>(entropy_or_null) |
         reinterpret_cast<uintptr_t>(logits_or_null)) & 3u)
        return fail(CCX_EINVAL, "ccx_mlp_sample_actions: w1t, b1, w2, b2, logp, entropy and logits must be 4-byte aligned");
    CCX_HIP(hipSetDevice(h->device));
    const MlpArgs A{obs, w1t, b1, w2, b2, logits_or_null, nullptr, (long long)rows, L, H, 5, activation};
    const DrawArgs D = ccx_draw::draw_args(h, masks_or_null, actions, logp_or_null, entropy_or_null);
    const size_t bytes = lds_floats(L, H, 5, true) * sizeof(float);
    const dim3 grid((unsigned)((rows + 63) / 64)), block(64 * (H / ccx_mlp::kGroup));
    const bool stats = logp_or_null || entropy_or_null, det = deterministic != 0;
#define CCX_MLP_DRAW(DET, STATS)                                                                  \
    do {                                                                                          \
        CCX_HIP(allow_lds(mlp_draw_kernel<DET, STATS>, bytes));                                   \
        hipLaunchKernelGGL((mlp_draw_kernel<DET, STATS>), grid, block, bytes, h->stream, A, D);   \
    } while (0)
    if (det) {
        if (stats) CCX_MLP_DRAW(true, true);
        else CCX_MLP_DRAW(true, false);
    } else {
        if (stats) CCX_MLP_DRAW(false, true);
        else CCX_MLP_DRAW(false, false);
    }
#undef CCX_MLP_DRAW
    CCX_HIP(hipGetLastError());
    return CCX_OK;
}

}  // extern "C"
