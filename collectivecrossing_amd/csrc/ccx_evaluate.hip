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
    const uint32_t lane = threadIdx.x;
    const long long row = (long long)blockIdx.x * 64 + lane;
    const long long rl = row < A.M ? row : A.M - 1;                     // the tail wave's surplus lanes load what its last row loads
    const uint32_t a = A.actions[rl];
    const uint32_t mbyte = MASK ? (uint32_t)A.masks[rl] : 0x1Fu;
    const long long floats = A.M * 5, last_piece = floats / 4 - 1;      // M >= 1: at least one whole piece
    float l[5];
    ccx_rows::load_rows(A.logits, A.M, pieces, lane, blockIdx.x, row, floats, last_piece, l);
    if (row >= A.M) return;
    float logp, entropy = 0.0f;
    ccx_softmax::evaluate_row<ENT>(l, mbyte, a, logp, entropy);
    A.logp[row] = logp;
    if (ENT) A.entropy[row] = entropy;
}

template <bool MASK, bool GLP, bool GENT>
__global__ __launch_bounds__(64) void evaluate_bwd_kernel(const EvalArgs A) {
    __shared__ float4 pieces[80];
    const uint32_t lane = threadIdx.x;
    const long long row = (long long)blockIdx.x * 64 + lane;
    const long long rl = row < A.M ? row : A.M - 1;
    const uint32_t a = A.actions[rl];
    const uint32_t mbyte = MASK ? (uint32_t)A.masks[rl] : 0x1Fu;
    const float glp = GLP ? A.grad_logp[rl] : 0.0f;
    const float gent = GENT ? A.grad_entropy[rl] : 0.0f;
    const long long floats = A.M * 5, last_piece = floats / 4 - 1;
    float l[5], g[5];
    ccx_rows::load_rows(A.logits, A.M, pieces, lane, blockIdx.x, row, floats, last_piece, l);
    ccx_softmax::evaluate_row_backward<GLP, GENT>(l, mbyte, a, glp, gent, g);
    ccx_rows::store_rows(A.grad_logits, A.M, pieces, lane, blockIdx.x, row, floats, last_piece, g);
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
    if (reinterpret_cast<uintptr_t>(logits) & 15u) return fail(CCX_EINVAL, "ccx_evaluate_actions: logits must be 16-byte aligned");
    CCX_HIP(hipSetDevice(h->device));
    EvalArgs A{};
    A.logits = logits;
    A.actions = actions;
    A.masks = masks_or_null;
    A.logp = logp;
    A.entropy = entropy_or_null;
    A.M = rows;
    const dim3 grid(blocks), block(64);
    if (masks_or_null) {
        if (entropy_or_null) hipLaunchKernelGGL((evaluate_fwd_kernel<true, true>), grid, block, 0, h->stream, A);
        else hipLaunchKernelGGL((evaluate_fwd_kernel<true, false>), grid, block, 0, h->stream, A);
    } else {
        if (entropy_or_null) hipLaunchKernelGGL((evaluate_fwd_kernel<false, true>), grid, block, 0, h->stream, A);
        else hipLaunchKernelGGL((evaluate_fwd_kernel<false, false>), grid, block, 0, h->stream, A);
    }
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
    if ((reinterpret_cast<uintptr_t>(logits) | reinterpret_cast<uintptr_t>(grad_logits)) & 15u)
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
    const int which = (grad_logp_or_null ? 1 : 0) | (grad_entropy_or_null ? 2 : 0);
    if (masks_or_null) {
        if (which == 3) hipLaunchKernelGGL((evaluate_bwd_kernel<true, true, true>), grid, block, 0, h->stream, A);
        else if (which == 1) hipLaunchKernelGGL((evaluate_bwd_kernel<true, true, false>), grid, block, 0, h->stream, A);
        else hipLaunchKernelGGL((evaluate_bwd_kernel<true, false, true>), grid, block, 0, h->stream, A);
    } else {
        if (which == 3) hipLaunchKernelGGL((evaluate_bwd_kernel<false, true, true>), grid, block, 0, h->stream, A);
        else if (which == 1) hipLaunchKernelGGL((evaluate_bwd_kernel<false, true, false>), grid, block, 0, h->stream, A);
        else hipLaunchKernelGGL((evaluate_bwd_kernel<false, false, true>), grid, block, 0, h->stream, A);
    }
    CCX_HIP(hipGetLastError());
    return CCX_OK;
}

}  // extern "C"
