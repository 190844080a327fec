// ccx_evaluate.hip -- CCX_EVALUATE (include/ccx.h): log pi(a_stored | s) and the entropy of the masked distribution under
// new logits, and the gradient of both with respect to those logits.  The distribution is CCX_SAMPLE's (ccx_softmax.h), so
// on the logits an action was sampled from the forward reproduces ccx_sample_actions' logp and entropy bit for bit.
//
// One lane owns one row; a wave takes 64 adjacent rows, a workgroup is one wave.
// Loads: ccx_sample.hip's scheme.  A wave's logits are 1280 contiguous bytes at a lane stride of 20; its 80 16-byte pieces
// are loaded whole (lanes 0-63 one each, lanes 0-15 a second one), written to LDS as they are, and each lane reads back its
// five dwords at a stride of 5 dwords (odd: the 32 lanes of a lane group hit 32 banks).  Every load is unconditional at a
// clamped index; the up to three floats behind the last whole piece are fetched as dwords by the last row's lane.
// Stores of the backward: the mirror image.  Each lane writes its five gradients to LDS where it read its logits (the
// lane's own 20 bytes: no other lane's logits are overwritten), then the wave stores whole pieces, lanes 0-63 one each and
// lanes 0-15 a second one: every 128-byte line of the wave's 1280 bytes is written whole by two global_store_dwordx4, not
// touched by five global_store_dword at a 20-byte stride.  Only pieces that lie entirely inside 5 M floats are stored; the
// up to three floats behind the last whole piece are stored as dwords by the last row's lane.
// The backward recomputes the forward quantities from the logits: nothing is saved between the passes but the inputs.
#include "ccx_internal.h"
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

// The wave's logits through LDS into l[5] of each lane (the load side both kernels share).  Returns with the pieces read
// back; surplus lanes of the tail wave (row >= M) hold the last row's values.
__device__ __forceinline__ void load_rows(const EvalArgs& A, float4 (&pieces)[80], uint32_t lane, long long row, long long floats,
                                          long long last_piece, float (&l)[5]) {
    const float4* src = reinterpret_cast<const float4*>(A.logits);
    const long long p0 = (long long)blockIdx.x * 80 + lane, p1 = (long long)blockIdx.x * 80 + 64 + (lane & 15u);
    const float4 v0 = src[p0 < last_piece ? p0 : last_piece];
    const float4 v1 = src[p1 < last_piece ? p1 : last_piece];          // (lanes 16-63 repeat the lines of lanes 0-15)
    pieces[lane] = v0;
    pieces[64 + (lane & 15u)] = v1;                                     // (the four lanes of an address write the same bytes)
    __syncthreads();
    const float* mine = reinterpret_cast<const float*>(pieces) + 5 * lane;
#pragma unroll
    for (int k = 0; k < 5; ++k) l[k] = mine[k];
    if (row == A.M - 1) {                                               // one lane of the launch, and only where 5 M % 4 != 0
        const int whole = 5 - (int)(floats & 3);
#pragma unroll
        for (int k = 2; k < 5; ++k)
            if (k >= whole) l[k] = A.logits[row * 5 + k];
    }
}

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
    load_rows(A, pieces, lane, row, floats, last_piece, l);
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
    load_rows(A, pieces, lane, row, floats, last_piece, l);
    ccx_softmax::evaluate_row_backward<GLP, GENT>(l, mbyte, a, glp, gent, g);
    // each lane overwrites the 20 bytes it read its own logits from; surplus lanes write nothing (what lies there belongs
    // to pieces behind the last whole one, which are not stored)
    float* mine = reinterpret_cast<float*>(pieces) + 5 * lane;
    if (row < A.M) {
#pragma unroll
        for (int k = 0; k < 5; ++k) mine[k] = g[k];
    }
    __syncthreads();
    float4* dst = reinterpret_cast<float4*>(A.grad_logits);
    const long long p0 = (long long)blockIdx.x * 80 + lane, p1 = (long long)blockIdx.x * 80 + 64 + lane;
    if (p0 <= last_piece) dst[p0] = pieces[lane];
    if (lane < 16u && p1 <= last_piece) dst[p1] = pieces[64 + lane];
    if (row == A.M - 1) {                                               // the floats behind the last whole piece
        const int whole = 5 - (int)(floats & 3);
#pragma unroll
        for (int k = 2; k < 5; ++k)
            if (k >= whole) A.grad_logits[row * 5 + k] = g[k];
    }
}

int check_rows(const char* who, int64_t rows, unsigned& blocks) {
    if (rows < 1) return fail(CCX_EINVAL, "%s: rows must be at least 1, got %lld", who, (long long)rows);
    const int64_t b = (rows + 63) / 64;
    if (b > 0x7FFFFFFFll) return fail(CCX_EINVAL, "%s: %lld rows need more than 2^31 - 1 workgroups", who, (long long)rows);
    blocks = (unsigned)b;
    return CCX_OK;
}

}  // namespace

extern "C" {

int ccx_evaluate_actions(ccx_handle* h, int64_t rows, const float* logits, const uint8_t* actions, const uint8_t* masks_or_null,
                         float* logp, float* entropy_or_null) {
    if (!h) return fail(CCX_EINVAL, "NULL handle");
    if (!logits || !actions || !logp)
        return fail(CCX_EINVAL, "ccx_evaluate_actions: NULL argument (logits, actions and logp are required)");
    unsigned blocks = 0;
    if (int rc = check_rows("ccx_evaluate_actions", rows, blocks)) return rc;
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
    if (int rc = check_rows("ccx_evaluate_actions_backward", rows, blocks)) return rc;
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
