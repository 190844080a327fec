// ccx_evaluate.hip -- CCX_EVALUATE (include/ccx.h): log pi(a_stored | s) and the entropy of the masked distribution under
// new logits, and the gradient of both with respect to those logits.  The distribution is CCX_SAMPLE's (ccx_softmax.h), so
// on the logits an action was sampled from the forward reproduces ccx_sample_actions' logp and entropy bit for bit.
//
// One lane owns one row; a wave takes 64 adjacent rows, a workgroup is one wave.  Loads of the logits and stores of the
// gradients go through LDS in whole 16-byte pieces: ccx_rows.h (the scheme of ccx_sample.hip, shared with ccx_ppo_loss.hip).
// The backward recomputes the forward quantities from the logits: nothing is saved between the passes but the inputs.
#include "ccx_internal.h"
#include "ccx_rows.h"
#include "ccx_softmax.h"

using ccxi::fail;
using ccxi::misaligned;
using ccxi::with_flags;

namespace {

struct EvalArgs {
    const float* logits;
    const uint8_t* actions;
    const uint8_t* masks;              // read only where MASK
    const float* grad_logp;            // backward, read only where GLP
    const float* grad_entropy;         // backward, read only where GENT
    float* logp;                       // forward
    float* entropy;                    // forward, written only where ENT
    float* grad_logits;                // backward
    long long M;
};

template <bool MASK, bool ENT>
__global__ __launch_bounds__(64) void evaluate_fwd_kernel(const EvalArgs A) {
    __shared__ float4 pieces[80];
    const ccx_rows::Wave W = ccx_rows::wave_of(A.M, blockIdx.x, threadIdx.x);
    const long long row = W.row, rl = W.rl;                             // the tail wave's surplus lanes load what its last row loads
    const uint32_t a = A.actions[rl];
    const uint32_t mbyte = MASK ? (uint32_t)A.masks[rl] : 0x1Fu;
    float l[5];
    ccx_rows::load_rows(A.logits, pieces, W, l);
    if (row >= A.M) return;
    float logp, entropy = 0.0f;
    ccx_softmax::evaluate_row<ENT>(l, mbyte, a, logp, entropy);
    A.logp[row] = logp;
    if (ENT) A.entropy[row] = entropy;
}

template <bool MASK, bool GLP, bool GENT>
__global__ __launch_bounds__(64) void evaluate_bwd_kernel(const EvalArgs A) {
    __shared__ float4 pieces[80];
    const ccx_rows::Wave W = ccx_rows::wave_of(A.M, blockIdx.x, threadIdx.x);
    const long long rl = W.rl;
    const uint32_t a = A.actions[rl];
    const uint32_t mbyte = MASK ? (uint32_t)A.masks[rl] : 0x1Fu;
    const float glp = GLP ? A.grad_logp[rl] : 0.0f;
    const float gent = GENT ? A.grad_entropy[rl] : 0.0f;
    float l[5], g[5];
    ccx_rows::load_rows(A.logits, pieces, W, l);
    ccx_softmax::evaluate_row_backward<GLP, GENT>(l, mbyte, a, glp, gent, g);
    ccx_rows::store_rows(A.grad_logits, pieces, W, g);
}

}  // namespace

extern "C" {

int ccx_evaluate_actions(ccx_handle* h, int64_t rows, const float* logits, const uint8_t* actions, const uint8_t* masks_or_null,
                         float* logp, float* entropy_or_null) {
    if (!h) return fail(CCX_EINVAL, "NULL handle");
    if (!logits || !actions || !logp)
        return fail(CCX_EINVAL, "ccx_evaluate_actions: NULL argument (logits, actions and logp are required)");
    unsigned blocks = 0;
    if (int rc = ccxi::row_blocks("ccx_evaluate_actions", rows, 64, blocks)) return rc;
    if (misaligned(16, logits)) return fail(CCX_EINVAL, "ccx_evaluate_actions: logits must be 16-byte aligned");
    CCX_HIP(hipSetDevice(h->device));
    EvalArgs A{};
    A.logits = logits;
    A.actions = actions;
    A.masks = masks_or_null;
    A.logp = logp;
    A.entropy = entropy_or_null;
    A.M = rows;
    const dim3 grid(blocks), block(64);
    with_flags([&](auto mask, auto ent) {
        hipLaunchKernelGGL((evaluate_fwd_kernel<decltype(mask)::value, decltype(ent)::value>), grid, block, 0, h->stream, A);
    }, masks_or_null != nullptr, entropy_or_null != nullptr);
    CCX_HIP(hipGetLastError());
    return CCX_OK;
}

int ccx_evaluate_actions_backward(ccx_handle* h, int64_t rows, const float* logits, const uint8_t* actions,
                                  const uint8_t* masks_or_null, const float* grad_logp_or_null, const float* grad_entropy_or_null,
                                  float* grad_logits) {
    if (!h) return fail(CCX_EINVAL, "NULL handle");
    if (!logits || !actions || !grad_logits)
        return fail(CCX_EINVAL, "ccx_evaluate_actions_backward: NULL argument (logits, actions and grad_logits are required)");
    if (!grad_logp_or_null && !grad_entropy_or_null)
        return fail(CCX_EINVAL, "ccx_evaluate_actions_backward: both gradients are NULL (at least one of grad_logp, grad_entropy is required)");
    unsigned blocks = 0;
    if (int rc = ccxi::row_blocks("ccx_evaluate_actions_backward", rows, 64, blocks)) return rc;
    if (misaligned(16, logits, grad_logits))
        return fail(CCX_EINVAL, "ccx_evaluate_actions_backward: logits and grad_logits must be 16-byte aligned");
    CCX_HIP(hipSetDevice(h->device));
    EvalArgs A{};
    A.logits = logits;
    A.actions = actions;
    A.masks = masks_or_null;
    A.grad_logp = grad_logp_or_null;
    A.grad_entropy = grad_entropy_or_null;
    A.grad_logits = grad_logits;
    A.M = rows;
    const dim3 grid(blocks), block(64);
    with_flags([&](auto mask, auto glp, auto gent) {
        constexpr bool MASK = decltype(mask)::value, GLP = decltype(glp)::value, GENT = decltype(gent)::value;
        if constexpr (GLP || GENT)                                      // (both null was refused above)
            hipLaunchKernelGGL((evaluate_bwd_kernel<MASK, GLP, GENT>), grid, block, 0, h->stream, A);
    }, masks_or_null != nullptr, grad_logp_or_null != nullptr, grad_entropy_or_null != nullptr);
    CCX_HIP(hipGetLastError());
    return CCX_OK;
}

}  // extern "C"
