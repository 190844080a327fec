// ccx_dueling.hip -- CCX_DUELING (include/ccx.h): the dueling combine over rows from memory, forward ([rows][6] -> [rows][5],
// up to four arrays of equal row count in ONE launch) and backward ([rows][5] -> [rows][6]).  The rule is ccx_dueling.h; the
// rows travel through LDS in whole 16-byte pieces by ccx_rows.h (rows of six: 96 pieces to a wave).  And the head's forward
// fused with ccx_q_actions' choice for ONE head (ccx_mlp_q_actions: observation rows in, actions out, one launch), which
// applies the same forward to a tile's outputs; its per-side sibling is obs_q_groups_kernel in ccx_sides.hip, beside the map
// it needs.
//
// dueling_fwd_kernel / dueling_bwd_kernel: one lane owns one row, a workgroup is one wave.  The forward's grid is
// (ceil(rows / 64), num): blockIdx.y picks the pair of pointers from the table, which travels BY VALUE in the kernel arguments
// (ccx_adam.hip's way: no host-to-device copy, so the call captures); the index is uniform, so the pick is scalar work.  Every
// element of every output is written.
// obs_q_kernel: ccx_mlp.hip's fused draw kernel over ccx_mlp_tile.h's mlp_tile, unchanged, with ccx_qact.h's from_tile behind
// the tile.
#include "ccx_mlp_tile.h"
#include "ccx_qact.h"
#include "ccx_rows.h"

using ccx_draw::DrawArgs;
using ccxi::fail;
using ccxi::misaligned;
using ccxi::with_flags;

namespace {

constexpr int kMaxArrays = 4;

struct DuelArgs {
    const float* va[kMaxArrays];       // [rows][6] each
    float* q[kMaxArrays];              // [rows][5] each
    long long rows;
};

__global__ __launch_bounds__(64) void dueling_fwd_kernel(const DuelArgs A) {
    __shared__ float4 in[96], out[80];
    const ccx_rows::WaveT<6> Wi = ccx_rows::wave_of<6>(A.rows, blockIdx.x, threadIdx.x);
    const ccx_rows::WaveT<5> Wo = ccx_rows::wave_of<5>(A.rows, blockIdx.x, threadIdx.x);
    float va[6], q[5];
    ccx_rows::load_rows(A.va[blockIdx.y], in, Wi, va);
    ccx_dueling::forward(va, q);
    ccx_rows::store_rows(A.q[blockIdx.y], out, Wo, q);
}

__global__ __launch_bounds__(64) void dueling_bwd_kernel(const float* grad_q, float* grad_va, long long rows) {
    __shared__ float4 in[80], out[96];
    const ccx_rows::WaveT<5> Wi = ccx_rows::wave_of<5>(rows, blockIdx.x, threadIdx.x);
    const ccx_rows::WaveT<6> Wo = ccx_rows::wave_of<6>(rows, blockIdx.x, threadIdx.x);
    float g[5], gva[6];
    ccx_rows::load_rows(grad_q, in, Wi, g);
    ccx_dueling::backward(g, gva);
    ccx_rows::store_rows(grad_va, out, Wo, gva);
}

// ccx_mlp.hip's mlp_draw_kernel with ccx_q_actions' choice (ccx_qact.h) in the place of the softmax draw: O = 5 takes the
// tile's outputs as the Q-values, O = 6 (DUEL) puts them through the dueling combine first.  The rate travels with wave 0's
// small loads.  With DUEL the tile stores no y (A.y is null): the COMBINED values go to q from wave 0's lanes.
template <bool EPS, bool DUEL>
__global__ __launch_bounds__(1024) void obs_q_kernel(const ccx_tile::MlpArgs A, const DrawArgs D, const float* epsilon, uint8_t* explored,
                                                      float* q) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const uint32_t lane = threadIdx.x & 63u;
    const bool first = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)) == 0;
    const ccx_draw::Slot s = ccx_draw::slot_of(D, lane);
    ccx_draw::Small v;
    float eps = 0.0f;
    if (first) {                                                          // wave 0's small loads, in flight under the layers
        v = ccx_draw::small_loads<!EPS>(D, s, D.masks != nullptr);
        if (EPS) eps = epsilon[0];
    }
    const float* y = ccx_tile::mlp_tile<true>(A, ccx_tile::AdjacentRows(), lds);
    __syncthreads();
    if (!first || s.slot >= D.EN) return;
    ccx_qact::from_tile<EPS, DUEL>(D, s, v, y, lane, eps, explored, q ? q + s.slot * 5 : nullptr);
}

}  // namespace

extern "C" {

int ccx_dueling_forward(ccx_handle* h, int64_t rows, int32_t num, const float* const* va, float* const* q) {
    if (!h) return fail(CCX_EINVAL, "NULL handle");
    if (!va || !q) return fail(CCX_EINVAL, "ccx_dueling_forward: NULL va or q");
    if (num < 1 || num > kMaxArrays) return fail(CCX_EINVAL, "ccx_dueling_forward: num = %d out of range (1 .. %d)", (int)num, kMaxArrays);
    unsigned blocks = 0;
    if (int rc = ccxi::row_blocks("ccx_dueling_forward", rows, 64, blocks)) return rc;
    if ((int64_t)blocks * num > 0x7FFFFFFFll)
        return fail(CCX_EINVAL, "ccx_dueling_forward: %lld rows of %d arrays need more than 2^31 - 1 workgroups", (long long)rows, (int)num);
    DuelArgs A{};
    for (int a = 0; a < num; ++a) {
        if (!va[a] || !q[a]) return fail(CCX_EINVAL, "ccx_dueling_forward: NULL va[%d] or q[%d]", a, a);
        if (misaligned(16, va[a], q[a])) return fail(CCX_EINVAL, "ccx_dueling_forward: va[%d] and q[%d] must be 16-byte aligned", a, a);
        A.va[a] = va[a];
        A.q[a] = q[a];
    }
    A.rows = rows;
    CCX_HIP(hipSetDevice(h->device));
    hipLaunchKernelGGL(dueling_fwd_kernel, dim3(blocks, (unsigned)num), dim3(64), 0, h->stream, A);
    CCX_HIP(hipGetLastError());
    return CCX_OK;
}

int ccx_dueling_backward(ccx_handle* h, int64_t rows, const float* grad_q, float* grad_va) {
    if (!h) return fail(CCX_EINVAL, "NULL handle");
    if (!grad_q || !grad_va) return fail(CCX_EINVAL, "ccx_dueling_backward: NULL grad_q or grad_va");
    unsigned blocks = 0;
    if (int rc = ccxi::row_blocks("ccx_dueling_backward", rows, 64, blocks)) return rc;
    if (misaligned(16, grad_q, grad_va)) return fail(CCX_EINVAL, "ccx_dueling_backward: grad_q and grad_va must be 16-byte aligned");
    CCX_HIP(hipSetDevice(h->device));
    hipLaunchKernelGGL(dueling_bwd_kernel, dim3(blocks), dim3(64), 0, h->stream, grad_q, grad_va, (long long)rows);
    CCX_HIP(hipGetLastError());
    return CCX_OK;
}

int ccx_mlp_q_actions(ccx_handle* h, int32_t H, int32_t activation, int32_t O, const float* obs, const float* w1t, const float* b1,
                      const float* w2, const float* b2, const uint8_t* masks_or_null, const float* epsilon_or_null, uint8_t* actions,
                      uint8_t* explored_or_null, float* q_or_null) {
    if (!h) return fail(CCX_EINVAL, "NULL handle");
    if (!obs || !w1t || !b1 || !w2 || !b2 || !actions)
        return fail(CCX_EINVAL, "ccx_mlp_q_actions: NULL argument (obs, the four parameter arrays and actions are required)");
    if (O != 5 && O != 6) return fail(CCX_EINVAL, "ccx_mlp_q_actions: O = %d, 5 (plain) or 6 (dueling) is required", (int)O);
    const int32_t L = ccx_obs_len(h->N);
    const int64_t rows = (int64_t)h->E * h->N;                           // E < 2^31, N <= 64: a grid below 2^31 workgroups
    if (const int rc = ccx_tile::check_dims("ccx_mlp_q_actions", L, H, O, activation)) return rc;
    if (misaligned(16, obs)) return fail(CCX_EINVAL, "ccx_mlp_q_actions: obs must be 16-byte aligned");
    if (misaligned(4, w1t, b1, w2, b2, epsilon_or_null, q_or_null))
        return fail(CCX_EINVAL, "ccx_mlp_q_actions: w1t, b1, w2, b2, epsilon and q must be 4-byte aligned");
    CCX_HIP(hipSetDevice(h->device));
    const DrawArgs D = ccx_qact::draw_args(h, masks_or_null, actions);
    const size_t bytes = ccx_tile::lds_floats(L, H, O, true) * sizeof(float);
    const dim3 grid((unsigned)((rows + 63) / 64)), block(64 * (H / ccx_mlp::kGroup));
    const int rc = with_flags([&](auto eps, auto duel) -> int {
        constexpr bool EPS = decltype(eps)::value, DUEL = decltype(duel)::value;
        const ccx_tile::MlpArgs A{obs, w1t, b1, w2, b2, DUEL ? nullptr : q_or_null, nullptr, (long long)rows, L, H, O, activation};
        CCX_HIP(ccx_tile::allow_lds(obs_q_kernel<EPS, DUEL>, bytes));
        hipLaunchKernelGGL((obs_q_kernel<EPS, DUEL>), grid, block, bytes, h->stream, A, D, epsilon_or_null, explored_or_null, q_or_null);
        return CCX_OK;
    }, epsilon_or_null != nullptr, O == 6);
    if (rc) return rc;
    CCX_HIP(hipGetLastError());
    return CCX_OK;
}

}  // extern "C"
