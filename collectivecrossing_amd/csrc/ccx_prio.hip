// ccx_prio.hip -- CCX_PRIO (include/ccx.h): proportional prioritised replay over the ring of CCX_REPLAY.  The priorities are
// fixed-point integers, so the sum tree is exact: its bits depend on neither reduction order nor tree shape, and a descent
// cannot run off the end.  The rule (tree shape, quantisation, the point of a draw, the descent, the weight) is ccx_prio.h's;
// the word is ccx_kernels.h's; the slot map is ccx_replay.h's.
//
// prio_set_kernel: one lane per (step, env) of the block the ring's push has just written: leaf = max_leaf, both read here.
// prio_mark_kernel / prio_max_kernel: an update in two launches, so that the leaf of a slot named by several b becomes the
// MAXIMUM of their new values in any lane order: the first stores -|leaf| at every named slot (a benign race: every writer
// stores the same value, and 0 stays 0), the second does a signed atomicMax of the new values, which are all >= 1.
// max_leaf takes one 64-bit atomicMax per wave.  No floating-point atomic, no last writer.
// prio_tree_kernel<LEAF>: a workgroup sums kFan^2 nodes of one level into the kFan nodes above them and the one above
// those, with the minimum of the non-zero leaves alongside; launched over the leaves, then over every second level, and at
// last as ONE workgroup whose top node is T: it writes T and min_leaf into pstate.  No last-block-done counter.
// prio_draw_kernel: one lane per draw: the two words, the point, the descent, the weight.
// prio_count_kernel: one plain lane adds 1 to draws BEHIND the draw that read it.
#include "ccx_internal.h"
#include "ccx_nstep.h"   // pushed_at: the head the ring's push read
#include "ccx_prio.h"

using ccxi::blocks_of;
using ccxi::fail;
using ccxi::misaligned;

namespace {

static_assert(ccx_prio::kStream == ccx::kPrioStream, "one constant for the prioritised draw's stream");
static_assert(ccx_prio::kFan == 16, "prio_tree_kernel: groups of 16 lanes, 16 groups to a workgroup of 256");

constexpr int kBlock = ccx_prio::kFan * ccx_prio::kFan;                   // 256

__global__ __launch_bounds__(256) void prio_set_kernel(int* leaf, const long long* ring_state, const long long* pstate,
                                                       const long long K, const long long total, const int S, const int E) {
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t >= total) return;
    const long long s = t / E, e = t - s * E;
    const long long head = ccx_nstep::pushed_at(ring_state[0], K);        // the head the ring's push read: it has advanced by K since
    leaf[ccx_replay::slot_of(head, s, S, E, e)] = (int)pstate[0];
}

__global__ __launch_bounds__(256) void prio_mark_kernel(int* leaf, const long long* index, const long long B, const long long R) {
    const long long b = (long long)blockIdx.x * 256 + threadIdx.x;
    if (b >= B) return;
    const long long i = index[b];
    if (!ccx_replay::in_ring(i, R)) return;
    const int v = leaf[i];
    if (v > 0) leaf[i] = -v;                                              // (v < 0: another lane has marked it already)
}

struct UpdateArgs {
    const float* td[ccx_prio::kMaxTd];                                    // [B][N] each
    int* leaf;
    long long* pstate;
    const long long* index;
    long long B, R;
    int count, N;
    float alpha, eps;
};

__global__ __launch_bounds__(256) void prio_max_kernel(const UpdateArgs A) {
    const long long b = (long long)blockIdx.x * 256 + threadIdx.x;
    int wrote = 0;                                                        // the new value where this lane writes one (>= 1)
    if (b < A.B) {
        const long long i = A.index[b];
        if (ccx_replay::in_ring(i, A.R) && A.leaf[i] != 0) {
            float m = 0.0f;
            for (int a = 0; a < A.count; ++a)
                for (int n = 0; n < A.N; ++n) m = ccx_prio::td_max(m, A.td[a][b * A.N + n]);
            wrote = ccx_prio::quantise(m, A.alpha, A.eps);
            atomicMax(&A.leaf[i], wrote);
        }
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const int o = __shfl_xor(wrote, d, 64);
        wrote = o > wrote ? o : wrote;
    }
    if ((threadIdx.x & 63u) == 0u && wrote > 0) atomicMax(&A.pstate[0], (long long)wrote);
}

// the minimum of two minima of non-zero leaves, 0 = none below
__device__ __forceinline__ long long min_nz(long long a, long long b) { return a == 0 ? b : (b == 0 ? a : (a < b ? a : b)); }

template <bool LEAF>
__global__ __launch_bounds__(256) void prio_tree_kernel(const int* leaf, const long long* sum_in, const long long* min_in,
                                                        const long long n_in, const long long n_mid, long long* sum_mid,
                                                        long long* min_mid, long long* sum_out, long long* min_out) {
    __shared__ long long part[2][ccx_prio::kFan];
    const long long i = (long long)blockIdx.x * kBlock + threadIdx.x;
    long long s = 0, m = 0;
    if (i < n_in) {
        if constexpr (LEAF) {
            s = leaf[i];
            m = s;
        } else {
            s = sum_in[i];
            m = min_in[i];
        }
    }
#pragma unroll
    for (int d = ccx_prio::kFan / 2; d >= 1; d >>= 1) {
        s += __shfl_xor(s, d, ccx_prio::kFan);
        m = min_nz(m, __shfl_xor(m, d, ccx_prio::kFan));
    }
    const int g = threadIdx.x / ccx_prio::kFan;
    if (threadIdx.x % ccx_prio::kFan == 0) {
        const long long node = i / ccx_prio::kFan;
        if (node < n_mid) {
            sum_mid[node] = s;
            min_mid[node] = m;
        }
        part[0][g] = s;
        part[1][g] = m;
    }
    __syncthreads();
    if (threadIdx.x < ccx_prio::kFan) {
        s = part[0][threadIdx.x];
        m = part[1][threadIdx.x];
#pragma unroll
        for (int d = ccx_prio::kFan / 2; d >= 1; d >>= 1) {
            s += __shfl_xor(s, d, ccx_prio::kFan);
            m = min_nz(m, __shfl_xor(m, d, ccx_prio::kFan));
        }
        if (threadIdx.x == 0) {
            sum_out[blockIdx.x] = s;
            min_out[blockIdx.x] = m;
        }
    }
}

struct DrawArgs {
    const int* leaf;
    const long long* tree;
    const long long* pstate;
    const float* beta;
    long long* index;                                                     // [B]
    float* weights;                                                       // [B][N]
    int* leaf_drawn;                                                      // [B]
    ccx_prio::Shape shape;
    long long B;
    int N, stratified;
    uint32_t seed_lo, seed_hi;
};

__global__ __launch_bounds__(256) void prio_draw_kernel(const DrawArgs A) {
    const long long b = (long long)blockIdx.x * 256 + threadIdx.x;
    if (b >= A.B) return;
    const unsigned long long T = (unsigned long long)A.pstate[2];
    const long long min_leaf = A.pstate[3];
    const ccx_replay::Key k = ccx_replay::key_of((unsigned long long)b, (unsigned long long)A.pstate[1]);
    const uint32_t w0 = ccx::random_word(A.seed_lo, A.seed_hi ^ ccx::kPrioStream, k.genv, k.episode, k.step, 0u);
    const uint32_t w1 = ccx::random_word(A.seed_lo, A.seed_hi ^ ccx::kPrioStream, k.genv, k.episode, k.step, 1u);
    const unsigned long long x = ccx_prio::point_of(w0, w1, (unsigned long long)b, (unsigned long long)A.B, A.stratified != 0);
    const unsigned long long u = ccx_replay::mulhi64(x, T);
    const long long i = ccx_prio::descend(A.leaf, A.tree, A.shape, ccx_prio::kFan, u, T);
    const bool drawn = i >= 0;
    const int lv = drawn ? A.leaf[i] : 0;
    const float w = ccx_prio::weight(min_leaf, lv, A.beta[0], drawn);
    A.index[b] = i;
    A.leaf_drawn[b] = lv;
    for (int n = 0; n < A.N; ++n) A.weights[b * A.N + n] = w;
}

__global__ __launch_bounds__(64) void prio_count_kernel(long long* pstate) {
    if (threadIdx.x == 0u && blockIdx.x == 0u) pstate[1] += 1;
}

// what every entry takes: the handle, the ring's S, the leaves and pstate
int check_prio(const char* who, const ccx_handle* h, int64_t ring_steps, const int32_t* leaf, const int64_t* pstate, int64_t& R) {
    if (int rc = ccxi::check_ring_steps(who, h, ring_steps)) return rc;
    if (!leaf || !pstate) return fail(CCX_EINVAL, "%s: NULL leaf or pstate", who);
    if (misaligned(4, leaf)) return fail(CCX_EINVAL, "%s: leaf must be 4-byte aligned", who);
    if (misaligned(8, pstate)) return fail(CCX_EINVAL, "%s: pstate must be 8-byte aligned", who);
    R = ring_steps * (int64_t)h->E;
    return CCX_OK;
}

}  // namespace

extern "C" {

int64_t ccx_prio_tree_words(int64_t records) { return records >= (1ll << 31) ? 0 : ccx_prio::tree_words(records); }

int ccx_prio_push(ccx_handle* h, int64_t ring_steps, const int64_t* ring_state, int64_t K, int32_t* leaf, const int64_t* pstate) {
    int64_t R = 0;
    if (int rc = check_prio("ccx_prio_push", h, ring_steps, leaf, pstate, R)) return rc;
    if (!ring_state) return fail(CCX_EINVAL, "ccx_prio_push: NULL ring_state");
    if (misaligned(8, ring_state)) return fail(CCX_EINVAL, "ccx_prio_push: ring_state must be 8-byte aligned");
    if (K < 1 || K > ring_steps)
        return fail(CCX_EINVAL, "ccx_prio_push: K = %lld out of range (1 <= K <= ring_steps = %lld)", (long long)K, (long long)ring_steps);
    CCX_HIP(hipSetDevice(h->device));
    const long long total = K * (int64_t)h->E;                            // <= R < 2^31
    hipLaunchKernelGGL(prio_set_kernel, dim3(blocks_of(total)), dim3(256), 0, h->stream, leaf, reinterpret_cast<const long long*>(ring_state),
                       reinterpret_cast<const long long*>(pstate), (long long)K, total, (int)ring_steps, (int)h->E);
    CCX_HIP(hipGetLastError());
    return CCX_OK;
}

int ccx_prio_update(ccx_handle* h, int64_t ring_steps, int32_t* leaf, int64_t* pstate, int64_t batch, const int64_t* index,
                    int32_t num_td, const float* const* td_error, float alpha, float eps) {
    UpdateArgs A{};
    int64_t R = 0;
    if (int rc = check_prio("ccx_prio_update", h, ring_steps, leaf, pstate, R)) return rc;
    if (!index || !td_error) return fail(CCX_EINVAL, "ccx_prio_update: NULL index or td_error");
    if (int rc = ccxi::check_batch_size("ccx_prio_update", h, batch)) return rc;
    if (num_td < 1 || num_td > ccx_prio::kMaxTd)
        return fail(CCX_EINVAL, "ccx_prio_update: num_td = %d out of range (1 .. %d)", (int)num_td, ccx_prio::kMaxTd);
    if (!(alpha >= 0.0f && alpha <= 1.0f)) return fail(CCX_EINVAL, "ccx_prio_update: alpha must lie in [0, 1]");
    if (!(eps > 0.0f) || eps == __builtin_inff()) return fail(CCX_EINVAL, "ccx_prio_update: eps must be a finite number > 0");
    if (misaligned(8, index)) return fail(CCX_EINVAL, "ccx_prio_update: index must be 8-byte aligned");
    for (int a = 0; a < num_td; ++a) {
        if (!td_error[a]) return fail(CCX_EINVAL, "ccx_prio_update: NULL td_error[%d]", a);
        if (misaligned(4, td_error[a])) return fail(CCX_EINVAL, "ccx_prio_update: td_error[%d] must be 4-byte aligned", a);
        A.td[a] = td_error[a];
    }
    CCX_HIP(hipSetDevice(h->device));
    A.leaf = leaf;
    A.pstate = reinterpret_cast<long long*>(pstate);
    A.index = reinterpret_cast<const long long*>(index);
    A.B = batch;
    A.R = R;
    A.count = num_td;
    A.N = h->N;
    A.alpha = alpha;
    A.eps = eps;
    hipLaunchKernelGGL(prio_mark_kernel, dim3(blocks_of(batch)), dim3(256), 0, h->stream, leaf, A.index, (long long)batch, (long long)R);
    hipLaunchKernelGGL(prio_max_kernel, dim3(blocks_of(batch)), dim3(256), 0, h->stream, A);
    CCX_HIP(hipGetLastError());
    return CCX_OK;
}

int ccx_prio_sample(ccx_handle* h, int64_t ring_steps, const int32_t* leaf, int64_t* pstate, const float* beta, int64_t* tree,
                    int64_t batch, int32_t stratified, int64_t* index, float* weights, int32_t* leaf_drawn) {
    DrawArgs A{};
    int64_t R = 0;
    if (int rc = check_prio("ccx_prio_sample", h, ring_steps, leaf, pstate, R)) return rc;
    if (!beta || !tree || !index || !weights || !leaf_drawn) return fail(CCX_EINVAL, "ccx_prio_sample: NULL argument");
    if (batch < 1 || batch >= (1ll << 31) || batch * (int64_t)h->N > (1ll << 31))
        return fail(CCX_EINVAL, "ccx_prio_sample: batch = %lld out of range (1 <= B < 2^31, B <= 2^31 / N)", (long long)batch);
    if (misaligned(8, tree, index)) return fail(CCX_EINVAL, "ccx_prio_sample: tree and index must be 8-byte aligned");
    if (misaligned(4, beta, weights, leaf_drawn)) return fail(CCX_EINVAL, "ccx_prio_sample: beta, weights and leaf_drawn must be 4-byte aligned");
    CCX_HIP(hipSetDevice(h->device));
    const ccx_prio::Shape s = ccx_prio::shape_of(R, ccx_prio::kFan);
    if (s.n[s.top - 1] > kBlock) return fail(CCX_EINVAL, "ccx_prio_sample: %lld records are more than the tree holds", (long long)R);
    long long* t = reinterpret_cast<long long*>(tree);
    long long* ps = reinterpret_cast<long long*>(pstate);
    const auto sums = [&](int l) { return t + s.off[l]; };
    const auto mins = [&](int l) { return t + s.nodes + s.off[l]; };
    for (int j = 0; j < s.launches; ++j) {                                // level 2j -> levels 2j + 1 and 2j + 2
        const int l = 2 * j;
        const dim3 grid((unsigned)s.n[l + 2]);
        if (j == 0)
            hipLaunchKernelGGL(prio_tree_kernel<true>, grid, dim3(256), 0, h->stream, leaf, nullptr, nullptr, (long long)s.n[0], (long long)s.n[1],
                               sums(1), mins(1), sums(2), mins(2));
        else
            hipLaunchKernelGGL(prio_tree_kernel<false>, grid, dim3(256), 0, h->stream, nullptr, sums(l), mins(l), (long long)s.n[l],
                               (long long)s.n[l + 1], sums(l + 1), mins(l + 1), sums(l + 2), mins(l + 2));
    }
    hipLaunchKernelGGL(prio_tree_kernel<false>, dim3(1), dim3(256), 0, h->stream, nullptr, sums(s.top - 1), mins(s.top - 1),
                       (long long)s.n[s.top - 1], (long long)s.n[s.top], sums(s.top), mins(s.top), ps + 2, ps + 3);
    A.leaf = leaf;
    A.tree = t;
    A.pstate = ps;
    A.beta = beta;
    A.index = reinterpret_cast<long long*>(index);
    A.weights = weights;
    A.leaf_drawn = leaf_drawn;
    A.shape = s;
    A.B = batch;
    A.N = h->N;
    A.stratified = stratified != 0;
    A.seed_lo = h->rng_lo;
    A.seed_hi = h->rng_hi;
    hipLaunchKernelGGL(prio_draw_kernel, dim3(blocks_of(batch)), dim3(256), 0, h->stream, A);
    hipLaunchKernelGGL(prio_count_kernel, dim3(1), dim3(64), 0, h->stream, ps);
    CCX_HIP(hipGetLastError());
    return CCX_OK;
}

}  // extern "C"
