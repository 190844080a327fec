// ccx_nstep.hip -- CCX_NSTEP (include/ccx.h): n-step targets over the ring of CCX_REPLAY.  One byte per record says whether
// the env's episode ended with it, and ONE kernel walks each drawn record forward through its successors in the ring and
// writes the minibatch of ccx_replay_fetch with the discounted n-step reward, the per-row discount gamma^m and the span m.
// The rule (slots, availability, the two spans, the f64 chain, the dropped row) is ccx_nstep.h's; the empty record is
// ccx_replay.h's; the lane layout, the draw, the wave's tile and the emission of the rows are ccx_gather.h's, the ring as the ABI
// passes it and what the launch shares with ccx_replay_fetch's (checks, arguments, grid) ccx_internal.h's.
//
// nstep_push_kernel: one lane per (step, env) of the block the ring's push has just written: cut = the step ended the episode.
// nstep_cut_kernel: one lane per env: cut = 1 at the newest ring step for the envs of the mask.
// nstep_fetch_kernel<DRAW, PAIR>: a record-gather wave (ccx_gather.h) -- lane (g, i) is agent i of record b0 + g.  The
// slot of successor k is arithmetic on the index, S and E, so NO successor address depends on loaded data: the loads of
// cut, done, valid and reward of the n records of the window, and of record 0's obs_c and action, are all issued before the
// first wait -- in the code object too: the bytes live in 32-bit registers of their own and pass an empty asm fence behind the
// last load before any arithmetic sees them (DESIGN.md 3.25 says what the compiler did without).  m_env comes from head and
// the cut bytes, the same in every lane of a group: no cross-lane traffic.  The ONE dependent load is next_c / masks_next of
// record m_env - 1.  Every slot is reduced mod S: no access leaves the arrays whatever head, cut or index hold.
// nstep_draws_kernel: one plain lane adds 1 to the ring's draws BEHIND the launch that read it.
#include "ccx_internal.h"
#include "ccx_gather.h"
#include "ccx_nstep.h"

using ccxi::BatchOut;
using ccxi::blocks_of;
using ccxi::fail;
using ccxi::FetchArgs;
using ccxi::misaligned;
using ccxi::with_flags;

namespace {

static_assert(ccx_nstep::kMax == CCX_NSTEP_MAX, "one constant for the longest window");
static_assert(ccx_nstep::kCutFlags == (CCX_EF_ALL_TERMINATED | CCX_EF_ALL_TRUNCATED | CCX_EF_RESET), "the flags that end an env's episode");

__global__ __launch_bounds__(256) void nstep_push_kernel(uint8_t* cut, const long long* ring_state, const uint8_t* env_flags,
                                                         const long long K, const long long total, const int S, const int E) {
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t >= total) return;
    const long long s = t / E, e = t - s * E;
    const long long head = ccx_nstep::pushed_at(ring_state[0], K);        // the head the ring's push read: it has advanced by K since
    cut[ccx_replay::slot_of(head, s, S, E, e)] = ccx_nstep::cut_of(env_flags[t]);
}

__global__ __launch_bounds__(256) void nstep_cut_kernel(uint8_t* cut, const long long* ring_state, const uint8_t* env_mask, const int S,
                                                        const int E) {
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    if (e >= E) return;
    const long long head = ring_state[0];
    if (head == 0) return;
    if (env_mask != nullptr && env_mask[e] == 0) return;
    cut[ccx_nstep::newest_step(head, S) * E + e] = 1;
}

__global__ __launch_bounds__(64) void nstep_draws_kernel(long long* state) {
    if (threadIdx.x == 0u && blockIdx.x == 0u) state[1] += 1;
}

struct NsOut : BatchOut {              // the n-step minibatch: the ring's, and per row what its reward covers
    float* discount;                   // [B][N]
    uint8_t* span;                     // [B][N]
};

struct NsArgs : FetchArgs {
    const uint8_t* cut;                // the cut bytes, [R]
    float* discount;
    uint8_t* span;
    int n;
    float gamma;
};

template <bool DRAW, bool PAIR>
__global__ __launch_bounds__(256) void nstep_fetch_kernel(const ccx::KParams p, const NsArgs A) {
    constexpr int kMax = ccx_nstep::kMax;
    extern __shared__ __align__(16) unsigned char smem[];
    const ccx_gather::Lane l = ccx_gather::lane_of(p, A.glog, A.B);
    const int N = l.N, i = l.i;
    const long long b = l.b;
    const bool mine = l.mine;
    const ccx_gather::Tile tile = ccx_gather::tile_of(smem, p, l);
    const long long head = A.ring.state[0];
    // the record: every lane of a group works it out for itself
    long long idx = -1;
    if (mine) {
        if constexpr (DRAW) idx = ccx_gather::ring_draw(b, head, A.ring.state[1], A.S, A.E, A.seed_lo, A.seed_hi);
        else idx = A.index_in[b];
    }
    const bool read = mine && ccx_replay::in_ring(idx, A.R);
    const long long at0 = read ? idx : 0;                                // (a lane that reads nothing walks record 0's slots, unread)
    const uint32_t S = (uint32_t)A.S, E = (uint32_t)A.E, un = (uint32_t)N;                    // (R = S E < 2^31: slots are 32-bit,
    const uint32_t ps = (uint32_t)at0 / E, e = (uint32_t)at0 - ps * E;                        //  slot * N + i one 32 x 32 -> 64 multiply-add)
    const auto at = [&](uint32_t slot) { return (unsigned long long)slot * un + (uint32_t)i; };
    float4 me = make_float4(0.0f, 0.0f, 0.0f, 0.0f), nx = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    uint8_t act = ccx_replay::kEmptyAction, mn = ccx_replay::kEmptyMasks;
    uint32_t ct[kMax], dn[kMax], vl[kMax];                              // (a byte each, in a register of its own: nothing is packed between the loads)
    double rw[kMax];
#pragma unroll
    for (int k = 0; k < kMax; ++k) {
        ct[k] = 0;
        dn[k] = ccx_replay::kEmptyDone;
        vl[k] = ccx_replay::kEmptyValid;
        rw[k] = ccx_replay::kEmptyReward;
    }
    if (read) {                                                          // (every load of the window is issued before the first wait)
        if (A.out.obs) me = A.ring.obs_c[at((uint32_t)at0)];
        act = A.ring.actions[at((uint32_t)at0)];
#pragma unroll
        for (int k = 1; k < kMax; ++k) {
            if (k < A.n) {                                               // (n is the launch's: the branch is uniform)
                const uint32_t sk = ccx_nstep::slot_k<uint32_t>(ps, (uint32_t)k, S, E, e);
                ct[k] = A.cut[sk];
                dn[k] = A.ring.done[at(sk)];
                vl[k] = A.ring.valid[at(sk)];
                rw[k] = A.ring.reward[at(sk)];
            }
        }
        ct[0] = A.cut[at0];                                              // (n >= 1: record 0 itself is always read; it comes last
        dn[0] = A.ring.done[at((uint32_t)at0)];                          //  because its block is the one that ends in the fence's wait)
        vl[0] = A.ring.valid[at((uint32_t)at0)];
        rw[0] = A.ring.reward[at((uint32_t)at0)];
    }
    // The bytes become visible to the arithmetic only HERE, behind the last load of the window, newest load first (loads return
    // in order: the first wait is for all of them).  Without the fence the compiler narrows the comparisons below to the loaded
    // bytes themselves and widens record 0's in the block that loads them: a wait in front of every successor's loads.
#pragma unroll
    for (int k = kMax - 1; k >= 0; --k) asm volatile("" : "+v"(ct[k]), "+v"(dn[k]), "+v"(vl[k]));
    const long long av = read ? ccx_nstep::avail(head, (long long)ps, A.S) : 0;
    const int m_env = ccx_nstep::env_span(A.n, av, ct);
    if (read) {                                                          // the one dependent load: the record the window ends on
        const uint32_t sl = ccx_nstep::slot_k<uint32_t>(ps, (uint32_t)(m_env - 1), S, E, e);
        if (A.out.next_obs) nx = A.ring.next_c[at(sl)];
        mn = A.ring.masks_next[at(sl)];
    }
    const ccx_nstep::Span<uint32_t> sp = ccx_nstep::agent_span(m_env, dn, vl);
    const int m_a = sp.m;
    const ccx_nstep::Return ret = ccx_nstep::returns(m_a, rw, A.gamma);
    const uint32_t done_out = sp.done_out;
    const uint32_t valid_out = ccx_nstep::dropped(m_a, m_env, done_out) ? 0u : vl[0];
    if (mine) {
        const long long to = b * N + i;
        A.out.actions[to] = act;
        A.out.reward[to] = ret.G;
        A.out.done[to] = (uint8_t)done_out;
        A.out.valid[to] = (uint8_t)valid_out;
        A.out.masks_next[to] = mn;
        A.discount[to] = ret.discount;
        A.span[to] = (uint8_t)m_a;
        if (i == 0) A.out.index[b] = idx;
    }
    ccx_gather::emit_rows<PAIR>(tile, p, l, A.B, A.out.obs, A.out.next_obs, me, nx);
}

// S, the ring's state and the cut bytes: what the two small launches take
int check_cut(const char* who, const ccx_handle* h, int64_t ring_steps, const int64_t* ring_state, const uint8_t* cut) {
    if (int rc = ccxi::check_ring_steps(who, h, ring_steps)) return rc;
    if (!ring_state || !cut) return fail(CCX_EINVAL, "%s: NULL ring_state or cut", who);
    if (misaligned(8, ring_state)) return fail(CCX_EINVAL, "%s: ring_state must be 8-byte aligned", who);
    return CCX_OK;
}

int fetch(const char* who, ccx_handle* h, CCX_RING_PARAMS, const uint8_t* cut, int32_t n, float gamma, int64_t B, const int64_t* index_in,
          const NsOut& out, bool draw) {
    NsArgs A{};
    dim3 grid, block;
    if (int rc = ccxi::fetch_args(who, h, CCX_RING_ARGS, B, index_in, out, draw, A, grid, block)) return rc;
    if (!cut) return fail(CCX_EINVAL, "%s: NULL ring_state or cut", who);
    if (n < 1 || n > CCX_NSTEP_MAX || (int64_t)n > ring_steps)
        return fail(CCX_EINVAL, "%s: n = %d out of range (1 <= n <= min(ring_steps, %d))", who, (int)n, CCX_NSTEP_MAX);
    if (!(gamma >= 0.0f && gamma <= 1.0f)) return fail(CCX_EINVAL, "%s: gamma must be finite and lie in [0, 1], got %g", who, (double)gamma);
    if (!out.discount || !out.span) return fail(CCX_EINVAL, "%s: NULL output (only obs and next_obs may be NULL)", who);
    if (misaligned(4, out.discount)) return fail(CCX_EINVAL, "%s: discount must be 4-byte aligned", who);
    CCX_HIP(hipSetDevice(h->device));
    A.cut = cut;
    A.discount = out.discount;
    A.span = out.span;
    A.n = n;
    A.gamma = gamma;
    with_flags([&](auto drw, auto pair) {
        hipLaunchKernelGGL((nstep_fetch_kernel<decltype(drw)::value, decltype(pair)::value>), grid, block, h->shape.lds_bytes_observe,
                           h->stream, h->kp, A);
    }, draw, (h->N % 2) == 0);
    // (replay_head_kernel(state, 0, 1) does the same, but it is ccx_replay.hip's own: the resource tests count one of each name)
    if (draw) hipLaunchKernelGGL(nstep_draws_kernel, dim3(1), dim3(64), 0, h->stream, A.ring.state);
    CCX_HIP(hipGetLastError());
    return CCX_OK;
}

}  // namespace

extern "C" {

int ccx_nstep_push(ccx_handle* h, int64_t ring_steps, const int64_t* ring_state, int64_t K, const uint8_t* env_flags, uint8_t* cut) {
    if (int rc = check_cut("ccx_nstep_push", h, ring_steps, ring_state, cut)) return rc;
    if (!env_flags) return fail(CCX_EINVAL, "ccx_nstep_push: NULL env_flags");
    if (K < 1 || K > ring_steps)
        return fail(CCX_EINVAL, "ccx_nstep_push: K = %lld out of range (1 <= K <= ring_steps = %lld)", (long long)K, (long long)ring_steps);
    CCX_HIP(hipSetDevice(h->device));
    const long long total = K * (int64_t)h->E;                            // <= R < 2^31
    hipLaunchKernelGGL(nstep_push_kernel, dim3(blocks_of(total)), dim3(256), 0, h->stream, cut, reinterpret_cast<const long long*>(ring_state),
                       env_flags, (long long)K, total, (int)ring_steps, (int)h->E);
    CCX_HIP(hipGetLastError());
    return CCX_OK;
}

int ccx_nstep_mark_cut(ccx_handle* h, int64_t ring_steps, const int64_t* ring_state, const uint8_t* env_mask_or_null, uint8_t* cut) {
    if (int rc = check_cut("ccx_nstep_mark_cut", h, ring_steps, ring_state, cut)) return rc;
    CCX_HIP(hipSetDevice(h->device));
    hipLaunchKernelGGL(nstep_cut_kernel, dim3(blocks_of(h->E)), dim3(256), 0, h->stream, cut, reinterpret_cast<const long long*>(ring_state),
                       env_mask_or_null, (int)ring_steps, (int)h->E);
    CCX_HIP(hipGetLastError());
    return CCX_OK;
}

int ccx_nstep_sample(ccx_handle* h, CCX_RING_PARAMS, const uint8_t* cut, int32_t n, float gamma, int64_t batch, float* obs_or_null,
                     float* next_obs_or_null, uint8_t* actions, double* reward, uint8_t* done, uint8_t* valid, uint8_t* masks_next,
                     int64_t* index, float* discount, uint8_t* span) {
    return fetch("ccx_nstep_sample", h, CCX_RING_ARGS, cut, n, gamma, batch, nullptr,
                 NsOut{{obs_or_null, next_obs_or_null, actions, reward, done, valid, masks_next, index}, discount, span}, true);
}

int ccx_nstep_fetch(ccx_handle* h, CCX_RING_PARAMS, const uint8_t* cut, int32_t n, float gamma, int64_t batch, const int64_t* index_in,
                    float* obs_or_null, float* next_obs_or_null, uint8_t* actions, double* reward, uint8_t* done, uint8_t* valid,
                    uint8_t* masks_next, int64_t* index, float* discount, uint8_t* span) {
    return fetch("ccx_nstep_fetch", h, CCX_RING_ARGS, cut, n, gamma, batch, index_in,
                 NsOut{{obs_or_null, next_obs_or_null, actions, reward, done, valid, masks_next, index}, discount, span}, false);
}

}  // extern "C"
