// ccx_c51.hip -- CCX_C51 (include/ccx.h): categorical Q-heads.  Expected values of a [M][5][A] array of logits, the projected
// target with the cross-entropy loss, its means over the rows that count, and the gradient with respect to the logits.  The
// per-place rules and the wave sums are ccx_c51.h; greedy, the counting rule and the final values are ccx_qlearn.h's; the
// f64 tree is ccx_tree.h's; a row's gate, the selection into the sums, the final kernel's body, the backward's scale and the
// forward entry are ccx_loss.h's (the frame of a loss over the rows that count).
//
// Everywhere a lane owns an atom and a wave works on one row at a time; a row of A floats is one coalesced run, and f32
// alignment is all that is asked (A = 51 gives 204-byte rows).
// c51_q_kernel: a workgroup of four waves, one row each; a wave walks its row's five actions and lanes 0..4 store the five
// expected values.
// c51_partial_kernel / c51_final_kernel: a workgroup of SIXTEEN waves takes the 256 consecutive rows of one block of the tree,
// wave w the rows w, w + 16, ...: with double-Q it reads the five rows of next_online, then row k* of next_target and row a of
// logits, nothing else; a cut target (done, or a zero discount) reads no next-state row at all and a row that does not count
// reads no logits.  The projection is a gather: lane i walks j = 0 .. A - 1 with p_j and b_j broadcast from lane j, so the
// additions of m_i stand in ascending j without an atomic.  Lane 0 leaves the row's four f32 terms in LDS; behind a barrier
// thread t < 256 owns row t as the tree wants it, and ccx_tree::block_sums_wide writes the block's partials ([6][B] f64).
// ONE wave then adds the partials and writes `stats`.
// c51_bwd_kernel: a workgroup of four waves, one row each; every element of the row's 5 A gradients is written.
#include "ccx_loss.h"

#include "ccx_c51.h"

using ccxi::fail;
using ccxi::misaligned;

namespace {

constexpr int kLossWaves = 16, kRowWaves = 4;

struct CatArgs {
    const float* logits;
    const float* next_target;
    const float* next_online;          // read only where DOUBLE
    const uint8_t* actions;
    const double* reward;
    const uint8_t* done;
    const uint8_t* masks_next;         // or null (everything legal)
    const uint8_t* valid;              // or null
    const float* weights;              // or null
    const float* discount;             // or null (gamma)
    const float* stats_in;             // backward: the forward's stats
    const float* grad_loss;            // backward, or null (= 1.0f)
    const float* proj_in;              // backward
    float* grad_logits;                // backward
    double* partials;                  // forward: [6][B]
    float* stats;                      // forward
    float* row_loss;                   // forward, or null
    float* proj;                       // forward
    float* q;                          // q_values
    ccx_c51::Support Z;
    float gamma;
    long long M, B;
};

__device__ __forceinline__ uint32_t wave_id() { return (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)); }

__device__ __forceinline__ float lane_value(float v, int j) {
    return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), j));
}

__global__ __launch_bounds__(64 * kRowWaves) void c51_q_kernel(const CatArgs A) {
    const uint32_t lane = threadIdx.x & 63u;
    const long long row = (long long)blockIdx.x * kRowWaves + wave_id();
    if (row >= A.M) return;
    const int At = A.Z.A;
    const bool live = lane < (uint32_t)At;
    const float z = ccx_c51::atom_value(A.Z.vmin, A.Z.dz, (int)lane);
    float q[5];
#pragma unroll
    for (int k = 0; k < 5; ++k) {
        const ccx_c51::Dist D = ccx_c51::wave_dist(A.logits + (row * 5 + k) * At, lane, At);
        q[k] = ccx_c51::wave_expected(D, z, live);
    }
    if (lane < 5u) A.q[row * 5 + lane] = ccx_qlearn::pick(q, lane);
}

template <bool DOUBLE>
__global__ __launch_bounds__(64 * kLossWaves) void c51_partial_kernel(const CatArgs A) {
    __shared__ float terms[4][ccx_tree::kBlockRows];                     // term, ce, qa, y of the block's rows
    __shared__ double groups[ccx_c51::kSums][ccx_tree::kBlockGroups];
    const uint32_t lane = threadIdx.x & 63u, w = wave_id();
    const int At = A.Z.A;
    const bool live = lane < (uint32_t)At;
    const float z = ccx_c51::atom_value(A.Z.vmin, A.Z.dz, (int)lane);
    const float fi = (float)lane;
    const bool has_w = A.weights != nullptr;
    const long long base = (long long)blockIdx.x * ccx_tree::kBlockRows;
    for (uint32_t rloc = w; rloc < (uint32_t)ccx_tree::kBlockRows; rloc += kLossWaves) {
        const long long row = base + rloc;
        if (row >= A.M) break;                                            // (wave-uniform: the rows of a wave ascend)
        const ccx_loss::Gate G = ccx_loss::gate_of(A.actions, A.valid, row);
        if (!ccx_qlearn::row_counts(G.has_valid, G.vbyte, G.a)) {         // wave-uniform: nothing of the row is read
            if (live) A.proj[row * At + lane] = 0.0f;
            if (lane == 0u && A.row_loss) A.row_loss[row] = 0.0f;
            continue;
        }
        const float r = (float)A.reward[row];                             // one rounding, as CCX_GAE does it
        const float disc = A.discount ? A.discount[row] : A.gamma;
        const bool cut = ccx_c51::target_cut(A.done[row] != 0, disc);
        float pe = 0.0f, pS = 1.0f;
        if (!cut) {                                                       // wave-uniform
            const uint32_t mbyte = A.masks_next ? (uint32_t)A.masks_next[row] : ccx_qlearn::kLegalAll;
            const float* sel = (DOUBLE ? A.next_online : A.next_target) + row * 5 * At;
            float q[5], e5[5], S5[5];
#pragma unroll
            for (int k = 0; k < 5; ++k) {
                const ccx_c51::Dist D = ccx_c51::wave_dist(sel + k * At, lane, At);
                q[k] = ccx_c51::wave_expected(D, z, live);
                e5[k] = D.e;
                S5[k] = D.S;
            }
            const uint32_t kstar = ccx_qlearn::greedy(q, ccx_qlearn::legal_set(mbyte));
            if constexpr (DOUBLE) {
                const ccx_c51::Dist D = ccx_c51::wave_dist(A.next_target + (row * 5 + kstar) * At, lane, At);
                pe = D.e;
                pS = D.S;
            } else {
                pe = ccx_qlearn::pick(e5, kstar);
                pS = ccx_qlearn::pick(S5, kstar);
            }
        }
        const float pj = ccx_c51::target_mass(pe, pS, cut, (int)lane);
        const float bj = ccx_c51::target_place(r, disc, cut, z, A.Z.vmin, A.Z.dz, A.Z.top);
        float m = 0.0f;
        for (int j = 0; j < At; ++j) m = ccx_c51::project_add(m, lane_value(pj, j), lane_value(bj, j), fi);
        const ccx_c51::Dist D = ccx_c51::wave_dist(A.logits + (row * 5 + G.a) * At, lane, At);
        const float lS = ccx_c51::log_sum(D.S);
        const float ce = ccx_c51::ce_of(ccx_c51::wave_sum(ccx_c51::ce_place(m, D.d, lS, live)));
        const float qa = ccx_c51::wave_expected(D, z, live);
        const float y = ccx_c51::wave_sum(ccx_c51::mean_place(m, z, live));
        const float wi = has_w ? A.weights[row] : 1.0f;
        const float term = ccx_c51::weighted(has_w, wi, ce);
        if (live) A.proj[row * At + lane] = m;
        if (lane == 0u) {
            if (A.row_loss) A.row_loss[row] = ce;
            terms[0][rloc] = term;
            terms[1][rloc] = ce;
            terms[2][rloc] = qa;
            terms[3][rloc] = y;
        }
    }
    __syncthreads();
    // thread t < 256 owns row t of the block (what LDS holds for a row that does not count was never written: selected away)
    double s[ccx_c51::kSums] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    if (threadIdx.x < (uint32_t)ccx_tree::kBlockRows) {
        const long long row = base + threadIdx.x;
        const ccx_loss::Gate G = ccx_loss::gate_of(A.actions, A.valid, row < A.M ? row : A.M - 1);
        const bool counts = row < A.M && ccx_qlearn::row_counts(G.has_valid, G.vbyte, G.a);
        const bool bad = row < A.M && ccx_qlearn::row_bad(G.has_valid, G.vbyte, G.a);
        const float t[4] = {terms[0][threadIdx.x], terms[1][threadIdx.x], terms[2][threadIdx.x], terms[3][threadIdx.x]};
        ccx_loss::select_sums(counts, t, s);
        s[5] = bad ? 1.0 : 0.0;
    }
    ccx_tree::block_sums_wide(s, groups, A.partials, A.B);
}

__global__ __launch_bounds__(64) void c51_final_kernel(const CatArgs A) {
    // {S_term/n, S_ce/n, S_qa/n, S_y/n, 0, 0, n, bad}
    ccx_loss::final_body<ccx_c51::kSums, 8>(A.partials, A.B, A.stats, [](const auto& s, auto& st) { ccx_qlearn::td_finals(s, st); });
}

__global__ __launch_bounds__(64 * kRowWaves) void c51_bwd_kernel(const CatArgs A) {
    const uint32_t lane = threadIdx.x & 63u;
    const long long row = (long long)blockIdx.x * kRowWaves + wave_id();
    if (row >= A.M) return;
    const int At = A.Z.A;
    const bool live = lane < (uint32_t)At;
    const bool has_w = A.weights != nullptr;
    const ccx_loss::Gate G = ccx_loss::gate_of(A.actions, A.valid, row);
    const bool counts = ccx_loss::any_counted(A.stats_in) && ccx_qlearn::row_counts(G.has_valid, G.vbyte, G.a);
    float g = 0.0f;
    if (counts) {                                                         // wave-uniform: a row that does not count reads nothing
        const float sc = ccx_loss::scale_of(A.stats_in, A.grad_loss).sc;
        const float gw = ccx_qlearn::row_scale(has_w, sc, has_w ? A.weights[row] : 1.0f);
        const ccx_c51::Dist D = ccx_c51::wave_dist(A.logits + (row * 5 + G.a) * At, lane, At);
        float m = 0.0f;
        if (live) m = A.proj_in[row * At + lane];
        const float Msum = ccx_c51::wave_sum(ccx_c51::live_or_zero(m, live));
        g = ccx_c51::grad_place(D.e, D.S, Msum, m, gw);
    }
    if (live) {
#pragma unroll
        for (uint32_t k = 0; k < 5u; ++k) A.grad_logits[(row * 5 + k) * At + lane] = (counts && G.a == k) ? g : 0.0f;
    }
}

int check_support(const char* who, int32_t atoms, float vmin, float vmax) {
    if (atoms < ccx_c51::kMinAtoms || atoms > ccx_c51::kMaxAtoms)
        return fail(CCX_EINVAL, "%s: atoms must lie in 2 .. 64, got %d", who, (int)atoms);
    const float dz = ccx_c51::atom_gap(vmin, vmax, atoms);
    if (!(vmin - vmin == 0.0f) || !(vmax - vmax == 0.0f) || !(vmin < vmax) || !(dz - dz == 0.0f) || !(dz > 0.0f))
        return fail(CCX_EINVAL, "%s: vmin < vmax must both be finite, with a finite atom spacing above zero, got %g and %g", who,
                    (double)vmin, (double)vmax);
    return CCX_OK;
}

}  // namespace

extern "C" {

int64_t ccx_c51_workspace_bytes(int64_t rows) { return ccx_loss::workspace_bytes(rows, ccx_c51::kSums); }

int ccx_c51_q_values(ccx_handle* h, int64_t rows, int32_t atoms, float vmin, float vmax, const float* logits, float* q) {
    const char* who = "ccx_c51_q_values";
    if (!h) return fail(CCX_EINVAL, "NULL handle");
    if (!logits || !q) return fail(CCX_EINVAL, "%s: NULL argument (logits and q are required)", who);
    unsigned blocks = 0;
    if (int rc = ccxi::row_blocks(who, rows, kRowWaves, blocks)) return rc;
    if (int rc = check_support(who, atoms, vmin, vmax)) return rc;
    if (misaligned(4, logits)) return fail(CCX_EINVAL, "%s: logits must be 4-byte aligned", who);
    if (misaligned(16, q)) return fail(CCX_EINVAL, "%s: q must be 16-byte aligned (it is what ccx_q_actions takes)", who);
    CCX_HIP(hipSetDevice(h->device));
    CatArgs A{};
    A.logits = logits;
    A.q = q;
    A.Z = ccx_c51::support_of(atoms, vmin, vmax);
    A.M = rows;
    hipLaunchKernelGGL(c51_q_kernel, dim3(blocks), dim3(64 * kRowWaves), 0, h->stream, A);
    CCX_HIP(hipGetLastError());
    return CCX_OK;
}

int ccx_c51_loss(ccx_handle* h, int64_t rows, int32_t atoms, float vmin, float vmax, const float* logits, const uint8_t* actions,
                 const double* reward, const uint8_t* done, const float* next_target, const float* next_online_or_null,
                 const uint8_t* masks_next_or_null, const uint8_t* valid_or_null, const float* weights_or_null,
                 const float* discount_or_null, float gamma, void* workspace, float* stats, float* row_loss_or_null, float* proj) {
    const char* who = "ccx_c51_loss";
    return ccx_loss::forward(who, h, logits && actions && reward && done && next_target && workspace && stats && proj,
                             "only next_online, masks_next, valid, weights, discount and row_loss may be NULL", rows, workspace, [&] {
        if (int rc = check_support(who, atoms, vmin, vmax)) return rc;
        if (!discount_or_null)
            if (int rc = ccx_loss::check_gamma(who, gamma)) return rc;
        if (misaligned(4, logits, next_target, next_online_or_null, weights_or_null, discount_or_null, stats, row_loss_or_null, proj))
            return fail(CCX_EINVAL, "%s: the f32 arrays must be 4-byte aligned", who);
        // (the workspace is named with the reward here: the frame's own refusal behind this one finds nothing left)
        if (misaligned(8, reward, workspace)) return fail(CCX_EINVAL, "%s: reward and workspace must be 8-byte aligned", who);
        return (int)CCX_OK;
    }, ccx_loss::no_check, [&](double* partials, unsigned blocks) {
        CatArgs A{};
        A.logits = logits;
        A.next_target = next_target;
        A.next_online = next_online_or_null;
        A.actions = actions;
        A.reward = reward;
        A.done = done;
        A.masks_next = masks_next_or_null;
        A.valid = valid_or_null;
        A.weights = weights_or_null;
        A.discount = discount_or_null;
        A.gamma = discount_or_null ? 0.0f : gamma;
        A.partials = partials;
        A.stats = stats;
        A.row_loss = row_loss_or_null;
        A.proj = proj;
        A.Z = ccx_c51::support_of(atoms, vmin, vmax);
        A.M = rows;
        A.B = blocks;
        const dim3 grid(blocks), block(64 * kLossWaves);
        if (next_online_or_null) hipLaunchKernelGGL((c51_partial_kernel<true>), grid, block, 0, h->stream, A);
        else hipLaunchKernelGGL((c51_partial_kernel<false>), grid, block, 0, h->stream, A);
        return A;
    }, c51_final_kernel);
}

int ccx_c51_loss_backward(ccx_handle* h, int64_t rows, int32_t atoms, const float* logits, const uint8_t* actions, const float* proj,
                          const uint8_t* valid_or_null, const float* weights_or_null, const float* stats,
                          const float* grad_loss_or_null, float* grad_logits) {
    const char* who = "ccx_c51_loss_backward";
    if (!h) return fail(CCX_EINVAL, "NULL handle");
    if (!logits || !actions || !proj || !stats || !grad_logits)
        return fail(CCX_EINVAL, "%s: NULL argument (only valid, weights and grad_loss may be NULL)", who);
    unsigned blocks = 0;
    if (int rc = ccxi::row_blocks(who, rows, kRowWaves, blocks)) return rc;
    if (atoms < ccx_c51::kMinAtoms || atoms > ccx_c51::kMaxAtoms)
        return fail(CCX_EINVAL, "%s: atoms must lie in 2 .. 64, got %d", who, (int)atoms);
    if (misaligned(4, logits, proj, weights_or_null, stats, grad_loss_or_null, grad_logits))
        return fail(CCX_EINVAL, "%s: the f32 arrays must be 4-byte aligned", who);
    CCX_HIP(hipSetDevice(h->device));
    CatArgs A{};
    A.logits = logits;
    A.actions = actions;
    A.proj_in = proj;
    A.valid = valid_or_null;
    A.weights = weights_or_null;
    A.stats_in = stats;
    A.grad_loss = grad_loss_or_null;
    A.grad_logits = grad_logits;
    A.Z.A = atoms;
    A.M = rows;
    hipLaunchKernelGGL(c51_bwd_kernel, dim3(blocks), dim3(64 * kRowWaves), 0, h->stream, A);
    CCX_HIP(hipGetLastError());
    return CCX_OK;
}

}  // extern "C"
