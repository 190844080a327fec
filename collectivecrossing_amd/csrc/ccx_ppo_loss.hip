// ccx_ppo_loss.hip -- CCX_PPO_LOSS (include/ccx.h): the clipped-surrogate PPO loss over the rows that count, its statistics
// and its gradient with respect to logits and values, plus the masked moments that normalise the advantages.  The per-row
// rule and the final values are ccx_ppo.h (which calls ccx_softmax.h's evaluate_row*), the reduction tree is ccx_tree.h; the
// logits travel through LDS by ccx_rows.h.  What stands around the rule -- a row's gate, the selection into the sums, the
// final kernel's body, the backward's scale, the forward entry -- is ccx_loss.h's, shared with ccx_qlearn.hip and ccx_c51.hip.
// `valid` is a selection inside the kernels: shapes stay static, nothing is compacted, nothing synchronises with the host.
//
// Forward: two launches.  ppo_partial_kernel: a workgroup of four waves takes 256 consecutive rows, one lane one row; each
// wave reduces its 64 rows' six f64 terms by a butterfly (a group of the tree), lane 0 leaves them in LDS, and the first six
// threads add the four groups and write the block's six partials to the workspace ([6][B] f64).  ppo_final_kernel: ONE wave
// adds the partials lane-strided, runs the same butterfly and writes the eight f32 of `stats`.  There is no atomic and no
// last-block-done counter: a kernel boundary orders the partials, and two plain launches cannot hang.
// Backward: one launch, ppo_bwd_kernel, one lane one row, a workgroup is one wave (ccx_evaluate.hip's shape); it recomputes
// the forward terms from the inputs and reads nothing else but `stats`.
// The masked moments: moments_partial_kernel / moments_final_kernel, the same tree over three sums (their terms are f64 and
// they have no action byte: the partial kernel selects for itself, the final kernel and the entry are the frame's).
#include "ccx_loss.h"
#include "ccx_ppo.h"
#include "ccx_rows.h"

using ccxi::fail;
using ccxi::misaligned;
using ccxi::with_flags;

namespace {

struct PpoArgs {
    const float* logits;
    const uint8_t* actions;
    const uint8_t* masks;              // read only where MASK
    const float* logp_old;
    const float* advantages;
    const float* returns;
    const float* values;
    const uint8_t* valid;              // or null
    const float* norm;                 // or null: {mean, std}
    const float* stats_in;             // backward: the forward's stats
    const float* grad_loss;            // backward, or null (= 1.0f)
    float* grad_logits;                // backward, written only where GL
    float* grad_values;                // backward, written only where GV
    double* partials;                  // forward: [6][B]
    float* stats;                      // forward
    float lo, hi, vf_coef, ent_coef, adv_eps;
    long long M, B;
};

struct MomentArgs {
    const float* x;
    const uint8_t* valid;              // or null
    double* partials;                  // [3][B]
    float* out;
    long long M, B;
};

template <bool MASK>
__global__ __launch_bounds__(256) void ppo_partial_kernel(const PpoArgs A) {
    __shared__ float4 pieces[ccx_tree::kBlockGroups][80];
    __shared__ double groups[ccx_ppo::kSums][ccx_tree::kBlockGroups];
    const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
    const ccx_rows::Wave W = ccx_rows::wave_of(A.M, (long long)blockIdx.x * ccx_tree::kBlockGroups + w, lane);
    const long long row = W.row, rl = W.rl;                             // surplus lanes load what the last row loads
    const ccx_loss::Gate G = ccx_loss::gate_of(A.actions, A.valid, rl);
    const uint32_t mbyte = MASK ? (uint32_t)A.masks[rl] : 0x1Fu;
    const bool has_norm = A.norm != nullptr;
    const float lpo = A.logp_old[rl], adv = A.advantages[rl], ret = A.returns[rl], val = A.values[rl];
    float mean = 0.0f, denom = 1.0f;
    if (has_norm) {
        mean = A.norm[0];
        denom = A.norm[1] + A.adv_eps;
    }
    float l[5];
    ccx_rows::load_rows(A.logits, pieces[w], W, l);
    const bool counts = row < A.M && ccx_ppo::row_counts(G.has_valid, G.vbyte, G.a);
    const float an = ccx_ppo::normalised(has_norm, adv, mean, denom);
    ccx_ppo::Row t;
    ccx_ppo::forward_row(l, mbyte, G.a, lpo, an, ret, val, A.lo, A.hi, t);
    const float terms[5] = {t.surr, t.vl, t.H, t.kl, t.cf};
    double s[ccx_ppo::kSums];
    ccx_loss::select_sums(counts, terms, s);
    ccx_tree::block_sums(s, groups, A.partials, A.B);
}

__global__ __launch_bounds__(64) void ppo_final_kernel(const PpoArgs A) {
    ccx_loss::final_body<ccx_ppo::kSums, 8>(A.partials, A.B, A.stats, [&A](const auto& s, auto& st) { ccx_ppo::loss_finals(s, A.vf_coef, A.ent_coef, st); });
}

template <bool MASK, bool GL, bool GV>
__global__ __launch_bounds__(64) void ppo_bwd_kernel(const PpoArgs A) {
    __shared__ float4 pieces[GL ? 80 : 1];
    const uint32_t lane = threadIdx.x;
    const long long row = (long long)blockIdx.x * 64 + lane;
    const long long rl = row < A.M ? row : A.M - 1;                     // (ccx_rows::Wave's row and rl: the wave's context is built where GL)
    const ccx_loss::Gate G = ccx_loss::gate_of(A.actions, A.valid, rl);
    const float ret = A.returns[rl], val = A.values[rl];
    const ccx_loss::Scale S = ccx_loss::scale_of(A.stats_in, A.grad_loss);
    const bool counts = S.any && ccx_ppo::row_counts(G.has_valid, G.vbyte, G.a);
    if constexpr (GL) {
        const uint32_t mbyte = MASK ? (uint32_t)A.masks[rl] : 0x1Fu;
        const bool has_norm = A.norm != nullptr;
        const float lpo = A.logp_old[rl], adv = A.advantages[rl];
        float mean = 0.0f, denom = 1.0f;
        if (has_norm) {
            mean = A.norm[0];
            denom = A.norm[1] + A.adv_eps;
        }
        const float se = S.sc * A.ent_coef;
        const float gent = 0.0f - se;
        float l[5], gr[5];
        const ccx_rows::Wave W = ccx_rows::wave_of(A.M, blockIdx.x, lane);
        ccx_rows::load_rows(A.logits, pieces, W, l);
        const float an = ccx_ppo::normalised(has_norm, adv, mean, denom);
        ccx_ppo::backward_row_logits(l, mbyte, G.a, lpo, an, ret, val, A.lo, A.hi, S.sc, gent, gr);
#pragma unroll
        for (int k = 0; k < 5; ++k) gr[k] = counts ? gr[k] : 0.0f;
        ccx_rows::store_rows(A.grad_logits, pieces, W, gr);
    }
    if constexpr (GV) {
        const float scv = S.sc * A.vf_coef;
        const float gv = ccx_ppo::backward_row_value(ret, val, scv);
        if (row < A.M) A.grad_values[row] = counts ? gv : 0.0f;
    }
}

__global__ __launch_bounds__(256) void moments_partial_kernel(const MomentArgs A) {
    __shared__ double groups[ccx_ppo::kMomentSums][ccx_tree::kBlockGroups];
    const long long row = (long long)blockIdx.x * ccx_tree::kBlockRows + threadIdx.x;
    const long long rl = row < A.M ? row : A.M - 1;
    const bool counts = row < A.M && (A.valid == nullptr || A.valid[rl] != 0);
    const double x = (double)A.x[rl];                                   // exact
    const double xx = x * x;                                            // exact: 48 significant bits at most
    double s[ccx_ppo::kMomentSums] = {counts ? 1.0 : 0.0, counts ? x : 0.0, counts ? xx : 0.0};
    ccx_tree::block_sums(s, groups, A.partials, A.B);
}

__global__ __launch_bounds__(64) void moments_final_kernel(const MomentArgs A) {
    ccx_loss::final_body<ccx_ppo::kMomentSums, 4>(A.partials, A.B, A.out, [](const auto& s, auto& o) { ccx_ppo::moments_finals(s, o); });
}

bool finite_nonneg(float v) { return v >= 0.0f && v < __builtin_inff(); }                // (false for NaN)

int check_hyper(const char* who, float clip, float vf_coef, float ent_coef, float adv_eps) {
    if (!(clip > 0.0f && clip < 1.0f)) return fail(CCX_EINVAL, "%s: clip must lie in (0, 1), got %g", who, (double)clip);
    if (!finite_nonneg(vf_coef)) return fail(CCX_EINVAL, "%s: vf_coef must be finite and not negative, got %g", who, (double)vf_coef);
    if (!finite_nonneg(ent_coef)) return fail(CCX_EINVAL, "%s: ent_coef must be finite and not negative, got %g", who, (double)ent_coef);
    if (!finite_nonneg(adv_eps)) return fail(CCX_EINVAL, "%s: adv_eps must be finite and not negative, got %g", who, (double)adv_eps);
    return CCX_OK;
}

// what ccx_ppo_loss and its backward pass alike
PpoArgs ppo_args(int64_t rows, const float* logits, const uint8_t* actions, const uint8_t* masks_or_null, const float* logp_old,
                 const float* advantages, const float* returns, const float* values, const uint8_t* valid_or_null,
                 const float* norm_or_null, float clip, float vf_coef, float ent_coef, float adv_eps) {
    PpoArgs A{};
    A.logits = logits;
    A.actions = actions;
    A.masks = masks_or_null;
    A.logp_old = logp_old;
    A.advantages = advantages;
    A.returns = returns;
    A.values = values;
    A.valid = valid_or_null;
    A.norm = norm_or_null;
    A.lo = 1.0f - clip;                                                 // computed once, one f32 operation each
    A.hi = 1.0f + clip;
    A.vf_coef = vf_coef;
    A.ent_coef = ent_coef;
    A.adv_eps = adv_eps;
    A.M = rows;
    return A;
}

}  // namespace

extern "C" {

int64_t ccx_ppo_workspace_bytes(int64_t rows) { return ccx_loss::workspace_bytes(rows, ccx_ppo::kSums); }

int ccx_masked_moments(ccx_handle* h, int64_t rows, const float* x, const uint8_t* valid_or_null, void* workspace, float* out) {
    return ccx_loss::forward("ccx_masked_moments", h, x && workspace && out, "x, workspace and out are required", rows, workspace,
                             ccx_loss::no_check, ccx_loss::no_check, [&](double* partials, unsigned blocks) {
        MomentArgs A{};
        A.x = x;
        A.valid = valid_or_null;
        A.partials = partials;
        A.out = out;
        A.M = rows;
        A.B = blocks;
        hipLaunchKernelGGL(moments_partial_kernel, dim3(blocks), dim3(256), 0, h->stream, A);
        return A;
    }, moments_final_kernel);
}

int ccx_ppo_loss(ccx_handle* h, int64_t rows, const float* logits, const uint8_t* actions, const uint8_t* masks_or_null,
                 const float* logp_old, const float* advantages, const float* returns, const float* values,
                 const uint8_t* valid_or_null, const float* norm_or_null, float clip, float vf_coef, float ent_coef, float adv_eps,
                 void* workspace, float* stats) {
    const char* who = "ccx_ppo_loss";
    return ccx_loss::forward(who, h, logits && actions && logp_old && advantages && returns && values && workspace && stats,
                             "only masks, valid and norm may be NULL", rows, workspace, [&] {
        return misaligned(16, logits) ? fail(CCX_EINVAL, "%s: logits must be 16-byte aligned", who) : CCX_OK;
    }, [&] { return check_hyper(who, clip, vf_coef, ent_coef, adv_eps); }, [&](double* partials, unsigned blocks) {
        PpoArgs A = ppo_args(rows, logits, actions, masks_or_null, logp_old, advantages, returns, values, valid_or_null, norm_or_null,
                             clip, vf_coef, ent_coef, adv_eps);
        A.partials = partials;
        A.stats = stats;
        A.B = blocks;
        if (masks_or_null) hipLaunchKernelGGL((ppo_partial_kernel<true>), dim3(blocks), dim3(256), 0, h->stream, A);
        else hipLaunchKernelGGL((ppo_partial_kernel<false>), dim3(blocks), dim3(256), 0, h->stream, A);
        return A;
    }, ppo_final_kernel);
}

int ccx_ppo_loss_backward(ccx_handle* h, int64_t rows, const float* logits, const uint8_t* actions, const uint8_t* masks_or_null,
                          const float* logp_old, const float* advantages, const float* returns, const float* values,
                          const uint8_t* valid_or_null, const float* norm_or_null, float clip, float vf_coef, float ent_coef,
                          float adv_eps, const float* stats, const float* grad_loss_or_null, float* grad_logits_or_null,
                          float* grad_values_or_null) {
    if (!h) return fail(CCX_EINVAL, "NULL handle");
    if (!logits || !actions || !logp_old || !advantages || !returns || !values || !stats)
        return fail(CCX_EINVAL, "ccx_ppo_loss_backward: NULL argument (only masks, valid, norm, grad_loss and one gradient output may be NULL)");
    if (!grad_logits_or_null && !grad_values_or_null)
        return fail(CCX_EINVAL, "ccx_ppo_loss_backward: both gradient outputs are NULL (at least one of grad_logits, grad_values is required)");
    unsigned blocks = 0;
    if (int rc = ccxi::row_blocks("ccx_ppo_loss_backward", rows, 64, blocks)) return rc;
    if (misaligned(16, logits, grad_logits_or_null))
        return fail(CCX_EINVAL, "ccx_ppo_loss_backward: logits and grad_logits must be 16-byte aligned");
    if (int rc = check_hyper("ccx_ppo_loss_backward", clip, vf_coef, ent_coef, adv_eps)) return rc;
    CCX_HIP(hipSetDevice(h->device));
    PpoArgs A = ppo_args(rows, logits, actions, masks_or_null, logp_old, advantages, returns, values, valid_or_null, norm_or_null, clip,
                         vf_coef, ent_coef, adv_eps);
    A.stats_in = stats;
    A.grad_loss = grad_loss_or_null;
    A.grad_logits = grad_logits_or_null;
    A.grad_values = grad_values_or_null;
    const dim3 grid(blocks), block(64);
    // the masks are read for the logits' gradient only: without it there is one kernel
    if (!grad_logits_or_null) hipLaunchKernelGGL((ppo_bwd_kernel<false, false, true>), grid, block, 0, h->stream, A);
    else
        with_flags([&](auto mask, auto gv) {
            hipLaunchKernelGGL((ppo_bwd_kernel<decltype(mask)::value, true, decltype(gv)::value>), grid, block, 0, h->stream, A);
        }, masks_or_null != nullptr, grad_values_or_null != nullptr);
    CCX_HIP(hipGetLastError());
    return CCX_OK;
}

}  // extern "C"
