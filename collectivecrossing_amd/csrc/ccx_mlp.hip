// ccx_mlp.hip -- CCX_MLP (include/ccx.h): a two-layer perceptron from observation rows to logits as a fixed sequence of f32
// operations per row, as a kernel of its own (ccx_mlp_forward) and fused with CCX_SAMPLE (ccx_mlp_sample_actions: rows in,
// actions / logp / entropy out, one launch).
//
// The tile -- 64 rows through both layers, the mapping of hidden units to waves, the loads, the layer-2 order -- is
// ccx_mlp_tile.h's mlp_tile over AdjacentRows: workgroup b takes rows 64 b .. 64 b + 63, and adjacent threads store adjacent
// dwords of y.  The fused kernel also keeps y in LDS, and wave 0 then runs ccx_softmax.h's sample_slot on its lane's five
// logits: the same code ccx_sample.hip runs on logits read from memory.
// Arithmetic.  ccx_mlp.h's functions, one f32 operation per line (-ffp-contract=off; `/` is the correctly rounded division,
// asked for on this unit's compile line).
#include "ccx_draw.h"
#include "ccx_mlp_tile.h"

using ccx_draw::DrawArgs;
using ccx_tile::AdjacentRows;
using ccx_tile::MlpArgs;
using ccx_tile::allow_lds;
using ccx_tile::lds_floats;
using ccx_tile::mlp_tile;
using ccxi::fail;
using ccxi::misaligned;
using ccxi::with_flags;

namespace {

__global__ __launch_bounds__(1024) void mlp_forward_kernel(const MlpArgs A) {
    extern __shared__ float lds[];
    mlp_tile<false>(A, AdjacentRows(), lds);
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
    const float* y = mlp_tile<true>(A, AdjacentRows(), lds);
    __syncthreads();
    if (!first || s.slot >= D.EN) return;
    float l[5];
#pragma unroll
    for (int k = 0; k < 5; ++k) l[k] = y[5 * lane + k];
    ccx_draw::finish<DET, STATS>(D, s, v, l);
}

int check_shape(const char* who, int64_t rows, int32_t L, int32_t H, int32_t O, int32_t activation) {
    if (rows < 1) return fail(CCX_EINVAL, "%s: rows = %lld, at least 1 is required", who, (long long)rows);
    if (rows > (int64_t)0x7FFFFFFF * 64) return fail(CCX_EINVAL, "%s: rows = %lld exceed the grid (2^31 - 1 workgroups of 64 rows)", who, (long long)rows);
    if (const int rc = ccx_tile::check_dims(who, L, H, O, activation)) return rc;
    return CCX_OK;
}

}  // namespace

extern "C" {

int ccx_mlp_forward(ccx_handle* h, int64_t rows, int32_t L, int32_t H, int32_t O, int32_t activation, const float* x,
                    const float* w1t, const float* b1, const float* w2, const float* b2, float* y, float* hidden_or_null) {
    if (!h) return fail(CCX_EINVAL, "NULL handle");
    if (!x || !w1t || !b1 || !w2 || !b2 || !y) return fail(CCX_EINVAL, "ccx_mlp_forward: NULL argument (only hidden may be NULL)");
    if (const int rc = check_shape("ccx_mlp_forward", rows, L, H, O, activation)) return rc;
    if (misaligned(16, x, hidden_or_null)) return fail(CCX_EINVAL, "ccx_mlp_forward: x and hidden must be 16-byte aligned");
    if (misaligned(4, w1t, b1, w2, b2, y))
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
    if (misaligned(16, obs)) return fail(CCX_EINVAL, "ccx_mlp_sample_actions: obs must be 16-byte aligned");
    if (misaligned(4, w1t, b1, w2, b2, logp_or_null, entropy_or_null, logits_or_null))
        return fail(CCX_EINVAL, "ccx_mlp_sample_actions: w1t, b1, w2, b2, logp, entropy and logits must be 4-byte aligned");
    CCX_HIP(hipSetDevice(h->device));
    const MlpArgs A{obs, w1t, b1, w2, b2, logits_or_null, nullptr, (long long)rows, L, H, 5, activation};
    const DrawArgs D = ccx_draw::draw_args(h, masks_or_null, actions, logp_or_null, entropy_or_null);
    const size_t bytes = lds_floats(L, H, 5, true) * sizeof(float);
    const dim3 grid((unsigned)((rows + 63) / 64)), block(64 * (H / ccx_mlp::kGroup));
    const int rc = with_flags([&](auto det, auto stats) -> int {
        constexpr bool DET = decltype(det)::value, STATS = decltype(stats)::value;
        CCX_HIP(allow_lds(mlp_draw_kernel<DET, STATS>, bytes));
        hipLaunchKernelGGL((mlp_draw_kernel<DET, STATS>), grid, block, bytes, h->stream, A, D);
        return CCX_OK;
    }, deterministic != 0, logp_or_null || entropy_or_null);
    if (rc) return rc;
    CCX_HIP(hipGetLastError());
    return CCX_OK;
}

}  // extern "C"
