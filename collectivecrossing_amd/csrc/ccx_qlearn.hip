// ccx_qlearn.hip -- CCX_QLEARN (include/ccx.h): epsilon-greedy actions over the legal set from a network's Q-values, and the
// double-DQN TD error with its Huber loss, its means over the rows that count and its gradient with respect to the Q-values.
// The per-slot and per-row rules and the final values are ccx_qlearn.h; the tree is ccx_tree.h's; the slot rule (which (e, a) a
// lane owns, its small loads, its key) is ccx_draw.h's; from a slot's five Q-values to its stores is ccx_qact.h's choose (the
// fused actor kernels of ccx_mlp.hip and ccx_sides.hip run the same); the rows of five f32 travel through LDS by ccx_rows.h.
//
// q_act_kernel: ccx_sample.hip's shape.  One lane owns one slot, a workgroup is one wave; every load -- the small ones, the
// exploration rate, the wave's pieces -- is issued before the first wait.  The greedy instantiation reads neither counter.
// td_partial_kernel / td_final_kernel / td_bwd_kernel: the frame of a loss over the rows that count (ccx_loss.h) around
// ccx_qlearn.h's rule, in ccx_ppo_loss.hip's shapes.  Forward: a workgroup of four waves takes 256 consecutive rows, one lane
// one row, up to three arrays of rows through LDS; ONE wave then writes `stats`.  Backward: one lane one row, a workgroup is
// one wave; every element of grad_q is written, whole 16-byte pieces through LDS.
// tdn_partial_kernel / tdn_bwd_kernel: the same two bodies with discount[row] in the place of gamma (CCX_NSTEP:
// ccx_td_loss_discounted and its backward); td_final_kernel serves both.
#include "ccx_loss.h"
#include "ccx_qact.h"
#include "ccx_rows.h"

using ccx_draw::DrawArgs;
using ccxi::fail;
using ccxi::misaligned;
using ccxi::with_flags;

namespace {

template <bool MASK, bool EPS>
__global__ __launch_bounds__(64) void q_act_kernel(const float* q, const DrawArgs D, const float* epsilon, uint8_t* explored) {
    __shared__ float4 pieces[80];
    const uint32_t lane = threadIdx.x;
    const ccx_draw::Slot s = ccx_draw::slot_of(D, lane);
    // every load is issued before the first wait: the small ones, the rate, then the wave's pieces
    const ccx_draw::Small v = ccx_draw::small_loads<!EPS>(D, s, MASK);
    float eps = 0.0f;
    if (EPS) eps = epsilon[0];
    const ccx_rows::Wave W = ccx_rows::wave_of(D.EN, blockIdx.x, lane);  // (W.row is s.slot; the small loads clamp for themselves)
    float l[5];
    ccx_rows::load_rows(q, pieces, W, l);
    if (s.slot >= D.EN) return;
    ccx_qact::choose<EPS>(D, s, v, l, eps, explored);
}

struct TdArgs {
    const float* q;
    const float* q_next_target;
    const float* q_next_online;        // read only where DOUBLE
    const uint8_t* actions;
    const double* reward;
    const uint8_t* done;
    const uint8_t* masks_next;         // or null (everything legal)
    const uint8_t* valid;              // or null
    const float* weights;              // or null
    const float* stats_in;             // backward: the forward's stats
    const float* grad_loss;            // backward, or null (= 1.0f)
    float* grad_q;                     // backward
    double* partials;                  // forward: [6][B]
    float* stats;                      // forward
    float* td_error;                   // forward, or null
    float gamma, delta, c;
    long long M, B;
};

struct TdSmall {
    ccx_loss::Gate G;
    uint32_t mbyte;
    bool done, has_w;
    float r, w;
};

// what a row reads besides its rows of five: unconditional loads at a clamped index (surplus lanes load what the last row loads)
__device__ __forceinline__ TdSmall td_small(const TdArgs& A, long long rl) {
    TdSmall v;
    v.done = A.done[rl] != 0;
    v.r = (float)A.reward[rl];                                          // one rounding, as CCX_GAE does it
    v.mbyte = A.masks_next ? (uint32_t)A.masks_next[rl] : ccx_qlearn::kLegalAll;
    v.G = ccx_loss::gate_of(A.actions, A.valid, rl);                    // (behind the others: the test of the valid byte waits for it)
    v.has_w = A.weights != nullptr;
    v.w = v.has_w ? A.weights[rl] : 1.0f;
    return v;
}

// the forward of one workgroup, shared by td_partial_kernel (one gamma for the launch) and tdn_partial_kernel (discount[row]):
// gamma_at(rl) is the row's discount, loaded at the clamped index with the small loads
template <bool DOUBLE, class GammaAt>
__device__ __forceinline__ void td_partial_body(const TdArgs& A, float4 (&pieces)[DOUBLE ? 3 : 2][ccx_tree::kBlockGroups][80],
                                                double (&groups)[ccx_qlearn::kSums][ccx_tree::kBlockGroups], GammaAt gamma_at) {
    const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
    const ccx_rows::Wave W = ccx_rows::wave_of(A.M, (long long)blockIdx.x * ccx_tree::kBlockGroups + w, lane);
    const long long row = W.row;
    const TdSmall v = td_small(A, W.rl);
    const float gamma = gamma_at(W.rl);
    float q[5], qt[5], qo[5];
    ccx_rows::load_rows(A.q, pieces[0][w], W, q);
    ccx_rows::load_rows(A.q_next_target, pieces[1][w], W, qt);
    if constexpr (DOUBLE) ccx_rows::load_rows(A.q_next_online, pieces[2][w], W, qo);
    const bool counts = row < A.M && ccx_qlearn::row_counts(v.G.has_valid, v.G.vbyte, v.G.a);
    const bool bad = row < A.M && ccx_qlearn::row_bad(v.G.has_valid, v.G.vbyte, v.G.a);
    ccx_qlearn::Row t;
    if constexpr (DOUBLE) ccx_qlearn::forward_row(q, v.G.a, v.r, v.done, qt, qo, v.mbyte, gamma, A.delta, A.c, v.has_w, v.w, t);
    else ccx_qlearn::forward_row(q, v.G.a, v.r, v.done, qt, qt, v.mbyte, gamma, A.delta, A.c, v.has_w, v.w, t);
    if (A.td_error && row < A.M) A.td_error[row] = counts ? t.d : 0.0f;
    const float terms[4] = {t.term, t.ad, t.qa, t.y};
    double s[ccx_qlearn::kSums];
    ccx_loss::select_sums(counts, terms, s);
    s[5] = bad ? 1.0 : 0.0;
    ccx_tree::block_sums(s, groups, A.partials, A.B);
}

template <bool DOUBLE>
__global__ __launch_bounds__(256) void td_partial_kernel(const TdArgs A) {
    __shared__ float4 pieces[DOUBLE ? 3 : 2][ccx_tree::kBlockGroups][80];
    __shared__ double groups[ccx_qlearn::kSums][ccx_tree::kBlockGroups];
    td_partial_body<DOUBLE>(A, pieces, groups, [g = A.gamma](long long) { return g; });
}

template <bool DOUBLE>
__global__ __launch_bounds__(256) void tdn_partial_kernel(const TdArgs A, const float* discount) {
    __shared__ float4 pieces[DOUBLE ? 3 : 2][ccx_tree::kBlockGroups][80];
    __shared__ double groups[ccx_qlearn::kSums][ccx_tree::kBlockGroups];
    td_partial_body<DOUBLE>(A, pieces, groups, [discount](long long rl) { return discount[rl]; });
}

__global__ __launch_bounds__(64) void td_final_kernel(const TdArgs A) {
    ccx_loss::final_body<ccx_qlearn::kSums, 8>(A.partials, A.B, A.stats, [](const auto& s, auto& st) { ccx_qlearn::td_finals(s, st); });
}

template <bool DOUBLE, class GammaAt>
__device__ __forceinline__ void td_bwd_body(const TdArgs& A, float4 (&pieces)[DOUBLE ? 3 : 2][80], GammaAt gamma_at) {
    const ccx_rows::Wave W = ccx_rows::wave_of(A.M, blockIdx.x, threadIdx.x);
    const TdSmall v = td_small(A, W.rl);
    const float gamma = gamma_at(W.rl);
    const ccx_loss::Scale S = ccx_loss::scale_of(A.stats_in, A.grad_loss);
    float q[5], qt[5], qo[5];
    ccx_rows::load_rows(A.q, pieces[0], W, q);
    ccx_rows::load_rows(A.q_next_target, pieces[1], W, qt);
    if constexpr (DOUBLE) ccx_rows::load_rows(A.q_next_online, pieces[2], W, qo);
    const float gw = ccx_qlearn::row_scale(v.has_w, S.sc, v.w);
    const bool counts = S.any && ccx_qlearn::row_counts(v.G.has_valid, v.G.vbyte, v.G.a);
    ccx_qlearn::Row t;
    if constexpr (DOUBLE) ccx_qlearn::forward_row(q, v.G.a, v.r, v.done, qt, qo, v.mbyte, gamma, A.delta, A.c, v.has_w, v.w, t);
    else ccx_qlearn::forward_row(q, v.G.a, v.r, v.done, qt, qt, v.mbyte, gamma, A.delta, A.c, v.has_w, v.w, t);
    const float ga = ccx_qlearn::backward_row(t.d, t.ad, A.delta, gw);
    float gr[5];
#pragma unroll
    for (int k = 0; k < 5; ++k) gr[k] = (counts && v.G.a == (uint32_t)k) ? ga : 0.0f;
    ccx_rows::store_rows(A.grad_q, pieces[0], W, gr);
}

template <bool DOUBLE>
__global__ __launch_bounds__(64) void td_bwd_kernel(const TdArgs A) {
    __shared__ float4 pieces[DOUBLE ? 3 : 2][80];
    td_bwd_body<DOUBLE>(A, pieces, [g = A.gamma](long long) { return g; });
}

template <bool DOUBLE>
__global__ __launch_bounds__(64) void tdn_bwd_kernel(const TdArgs A, const float* discount) {
    __shared__ float4 pieces[DOUBLE ? 3 : 2][80];
    td_bwd_body<DOUBLE>(A, pieces, [discount](long long rl) { return discount[rl]; });
}

int check_td(const char* who, const void* q, const void* qt, const void* qo, float gamma, float huber_delta) {
    if (misaligned(16, q, qt, qo))
        return fail(CCX_EINVAL, "%s: q, q_next_target and q_next_online must be 16-byte aligned", who);
    if (int rc = ccx_loss::check_gamma(who, gamma)) return rc;
    if (!(huber_delta > 0.0f)) return fail(CCX_EINVAL, "%s: huber_delta must be > 0 (+inf: the squared error), got %g", who, (double)huber_delta);
    return CCX_OK;
}

TdArgs td_args(int64_t rows, const float* q, const uint8_t* actions, const double* reward, const uint8_t* done,
               const float* q_next_target, const float* q_next_online_or_null, const uint8_t* masks_next_or_null,
               const uint8_t* valid_or_null, const float* weights_or_null, float gamma, float huber_delta) {
    TdArgs A{};
    A.q = q;
    A.q_next_target = q_next_target;
    A.q_next_online = q_next_online_or_null;
    A.actions = actions;
    A.reward = reward;
    A.done = done;
    A.masks_next = masks_next_or_null;
    A.valid = valid_or_null;
    A.weights = weights_or_null;
    A.gamma = gamma;
    A.delta = huber_delta;
    A.c = 0.5f * huber_delta;                                           // computed once, one f32 operation
    A.M = rows;
    return A;
}

// ccx_td_loss (discount == NULL: one gamma) and ccx_td_loss_discounted (discount [M]): the same checks, the same two launches
int td_forward(const char* who, ccx_handle* h, int64_t rows, const float* q, const uint8_t* actions, const double* reward,
               const uint8_t* done, const float* q_next_target, const float* q_next_online_or_null, const uint8_t* masks_next_or_null,
               const uint8_t* valid_or_null, const float* weights_or_null, const float* discount, float gamma, float huber_delta,
               void* workspace, float* stats, float* td_error_or_null) {
    return ccx_loss::forward(who, h, q && actions && reward && done && q_next_target && workspace && stats,
                             "only q_next_online, masks_next, valid, weights and td_error may be NULL", rows, workspace, [&] {
        return check_td(who, q, q_next_target, q_next_online_or_null, gamma, huber_delta);
    }, [&] {
        return misaligned(4, discount) ? fail(CCX_EINVAL, "%s: discount must be 4-byte aligned", who) : CCX_OK;
    }, [&](double* partials, unsigned blocks) {
        TdArgs A = td_args(rows, q, actions, reward, done, q_next_target, q_next_online_or_null, masks_next_or_null, valid_or_null,
                           weights_or_null, gamma, huber_delta);
        A.partials = partials;
        A.stats = stats;
        A.td_error = td_error_or_null;
        A.B = blocks;
        const dim3 grid(blocks), block(256);
        if (discount) {
            if (q_next_online_or_null) hipLaunchKernelGGL((tdn_partial_kernel<true>), grid, block, 0, h->stream, A, discount);
            else hipLaunchKernelGGL((tdn_partial_kernel<false>), grid, block, 0, h->stream, A, discount);
        } else {
            if (q_next_online_or_null) hipLaunchKernelGGL((td_partial_kernel<true>), grid, block, 0, h->stream, A);
            else hipLaunchKernelGGL((td_partial_kernel<false>), grid, block, 0, h->stream, A);
        }
        return A;
    }, td_final_kernel);
}

int td_backward(const char* who, ccx_handle* h, int64_t rows, const float* q, const uint8_t* actions, const double* reward,
                const uint8_t* done, const float* q_next_target, const float* q_next_online_or_null, const uint8_t* masks_next_or_null,
                const uint8_t* valid_or_null, const float* weights_or_null, const float* discount, float gamma, float huber_delta,
                const float* stats, const float* grad_loss_or_null, float* grad_q) {
    if (!h) return fail(CCX_EINVAL, "NULL handle");
    if (!q || !actions || !reward || !done || !q_next_target || !stats || !grad_q)
        return fail(CCX_EINVAL, "%s: NULL argument (only q_next_online, masks_next, valid, weights and grad_loss may be NULL)", who);
    unsigned blocks = 0;
    if (int rc = ccxi::row_blocks(who, rows, 64, blocks)) return rc;
    if (int rc = check_td(who, q, q_next_target, q_next_online_or_null, gamma, huber_delta)) return rc;
    if (misaligned(16, grad_q)) return fail(CCX_EINVAL, "%s: grad_q must be 16-byte aligned", who);
    if (misaligned(4, discount)) return fail(CCX_EINVAL, "%s: discount must be 4-byte aligned", who);
    CCX_HIP(hipSetDevice(h->device));
    TdArgs A = td_args(rows, q, actions, reward, done, q_next_target, q_next_online_or_null, masks_next_or_null, valid_or_null,
                       weights_or_null, gamma, huber_delta);
    A.stats_in = stats;
    A.grad_loss = grad_loss_or_null;
    A.grad_q = grad_q;
    const dim3 grid(blocks), block(64);
    if (discount) {
        if (q_next_online_or_null) hipLaunchKernelGGL((tdn_bwd_kernel<true>), grid, block, 0, h->stream, A, discount);
        else hipLaunchKernelGGL((tdn_bwd_kernel<false>), grid, block, 0, h->stream, A, discount);
    } else {
        if (q_next_online_or_null) hipLaunchKernelGGL((td_bwd_kernel<true>), grid, block, 0, h->stream, A);
        else hipLaunchKernelGGL((td_bwd_kernel<false>), grid, block, 0, h->stream, A);
    }
    CCX_HIP(hipGetLastError());
    return CCX_OK;
}

}  // namespace

extern "C" {

int ccx_q_actions(ccx_handle* h, const float* q, const uint8_t* masks_or_null, const float* epsilon_or_null, uint8_t* actions,
                  uint8_t* explored_or_null) {
    if (!h) return fail(CCX_EINVAL, "NULL handle");
    if (!q || !actions) return fail(CCX_EINVAL, "ccx_q_actions: NULL argument (q and actions are required)");
    if (misaligned(16, q)) return fail(CCX_EINVAL, "ccx_q_actions: q must be 16-byte aligned");
    CCX_HIP(hipSetDevice(h->device));
    const DrawArgs D = ccx_qact::draw_args(h, masks_or_null, actions);
    const dim3 grid((unsigned)((D.EN + 63) / 64)), block(64);           // E < 2^31, N <= 64: below 2^31
    with_flags([&](auto mask, auto eps) {
        hipLaunchKernelGGL((q_act_kernel<decltype(mask)::value, decltype(eps)::value>), grid, block, 0, h->stream, q, D,
                           epsilon_or_null, explored_or_null);
    }, masks_or_null != nullptr, epsilon_or_null != nullptr);
    CCX_HIP(hipGetLastError());
    return CCX_OK;
}

int64_t ccx_td_workspace_bytes(int64_t rows) { return ccx_loss::workspace_bytes(rows, ccx_qlearn::kSums); }

int ccx_td_loss(ccx_handle* h, int64_t rows, const float* q, const uint8_t* actions, const double* reward, const uint8_t* done,
                const float* q_next_target, const float* q_next_online_or_null, const uint8_t* masks_next_or_null,
                const uint8_t* valid_or_null, const float* weights_or_null, float gamma, float huber_delta, void* workspace,
                float* stats, float* td_error_or_null) {
    return td_forward("ccx_td_loss", h, rows, q, actions, reward, done, q_next_target, q_next_online_or_null, masks_next_or_null,
                      valid_or_null, weights_or_null, nullptr, gamma, huber_delta, workspace, stats, td_error_or_null);
}

int ccx_td_loss_backward(ccx_handle* h, int64_t rows, const float* q, const uint8_t* actions, const double* reward,
                         const uint8_t* done, const float* q_next_target, const float* q_next_online_or_null,
                         const uint8_t* masks_next_or_null, const uint8_t* valid_or_null, const float* weights_or_null, float gamma,
                         float huber_delta, const float* stats, const float* grad_loss_or_null, float* grad_q) {
    return td_backward("ccx_td_loss_backward", h, rows, q, actions, reward, done, q_next_target, q_next_online_or_null,
                       masks_next_or_null, valid_or_null, weights_or_null, nullptr, gamma, huber_delta, stats, grad_loss_or_null, grad_q);
}

int ccx_td_loss_discounted(ccx_handle* h, int64_t rows, const float* q, const uint8_t* actions, const double* reward,
                           const uint8_t* done, const float* q_next_target, const float* q_next_online_or_null,
                           const uint8_t* masks_next_or_null, const uint8_t* valid_or_null, const float* weights_or_null,
                           const float* discount, float huber_delta, void* workspace, float* stats, float* td_error_or_null) {
    if (!discount) return fail(CCX_EINVAL, "ccx_td_loss_discounted: NULL discount");
    return td_forward("ccx_td_loss_discounted", h, rows, q, actions, reward, done, q_next_target, q_next_online_or_null,
                      masks_next_or_null, valid_or_null, weights_or_null, discount, 0.0f, huber_delta, workspace, stats, td_error_or_null);
}

int ccx_td_loss_discounted_backward(ccx_handle* h, int64_t rows, const float* q, const uint8_t* actions, const double* reward,
                                    const uint8_t* done, const float* q_next_target, const float* q_next_online_or_null,
                                    const uint8_t* masks_next_or_null, const uint8_t* valid_or_null, const float* weights_or_null,
                                    const float* discount, float huber_delta, const float* stats, const float* grad_loss_or_null,
                                    float* grad_q) {
    if (!discount) return fail(CCX_EINVAL, "ccx_td_loss_discounted_backward: NULL discount");
    return td_backward("ccx_td_loss_discounted_backward", h, rows, q, actions, reward, done, q_next_target, q_next_online_or_null,
                       masks_next_or_null, valid_or_null, weights_or_null, discount, 0.0f, huber_delta, stats, grad_loss_or_null, grad_q);
}

}  // extern "C"
