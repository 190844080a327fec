// ccx_nstep.hip -- CCX_NSTEP (include/ccx.h): n-step targets over the ring of CCX_REPLAY.  One byte per record says whether
// the env's episode ended with it, and ONE kernel walks each drawn record forward through its successors in the ring and
// writes the minibatch of ccx_replay_fetch with the discounted n-step reward, the per-row discount gamma^m and the span m.
// The rule (slots, availability, the two spans, the f64 chain, the dropped row) is ccx_nstep.h's; the draw and the empty
// record are ccx_replay.h's; the word is ccx_kernels.h's; the rows are written by ccx_rollout_dev.h's build_obs_table / emit_obs.
//
// nstep_push_kernel: one lane per (step, env) of the block the ring's push has just written: cut = the step ended the episode.
// nstep_cut_kernel: one lane per env: cut = 1 at the newest ring step for the envs of the mask.
// nstep_fetch_kernel<DRAW, PAIR>: the lane layout of replay_fetch_kernel -- lane (g, i) is agent i of record b0 + g.  The
// slot of successor k is arithmetic on the index, S and E, so NO successor address depends on loaded data: the loads of
// cut, done, valid and reward of the n records of the window, and of record 0's obs_c and action, are all issued before the
// first wait -- in the code object too: the bytes live in 32-bit registers of their own and pass an empty asm fence behind the
// last load before any arithmetic sees them (DESIGN.md 3.25 says what the compiler did without).  m_env comes from head and
// the cut bytes, the same in every lane of a group: no cross-lane traffic.  The ONE dependent load is next_c / masks_next of
// record m_env - 1.  Every slot is reduced mod S: no access leaves the arrays whatever head, cut or index hold.
// nstep_draws_kernel: one plain lane adds 1 to the ring's draws BEHIND the launch that read it.
#include "ccx_internal.h"
#include "ccx_nstep.h"
#include "ccx_replay.h"
#include "ccx_rollout_dev.h"

using ccxi::fail;
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

struct NsRing {                        // the ring's own storage, [R][N] (compact: [R][N] float4), and the cut bytes [R]
    const float4* obs_c;
    const float4* next_c;
    const uint8_t* actions;
    const double* reward;
    const uint8_t* done;
    const uint8_t* valid;
    const uint8_t* masks_next;
    const long long* state;            // {head, draws, 0, 0}
    const uint8_t* cut;
};

struct NsArgs {
    NsRing ring;
    const long long* index_in;         // [B]: read where !DRAW
    float* obs;                        // [B][N][L] or null
    float* next_obs;                   // [B][N][L] or null
    uint8_t* actions;                  // [B][N]
    double* reward;
    uint8_t* done;
    uint8_t* valid;
    uint8_t* masks_next;
    long long* index;                  // [B]
    float* discount;                   // [B][N]
    uint8_t* span;                     // [B][N]
    long long B, R;
    int S, E, glog, n;
    float gamma;
    uint32_t seed_lo, seed_hi;
};

template <bool DRAW, bool PAIR>
__global__ __launch_bounds__(256) void nstep_fetch_kernel(const ccx::KParams p, const NsArgs A) {
    using namespace ccx;
    constexpr int kMax = ccx_nstep::kMax;
    extern __shared__ __align__(16) unsigned char smem[];
    const int lane = threadIdx.x & 63;
    const int wib = threadIdx.x >> 6;
    const long long wave = (long long)blockIdx.x * p.waves_per_block + wib;
    const int g = lane >> A.glog, i = lane & ((1 << A.glog) - 1);
    const long long b0 = wave * p.EW, b = b0 + g;
    const int N = p.N, L = 6 + 4 * N;
    const bool mine = (g < p.EW) && (b < A.B) && (i < N);
    WaveLds* wl = reinterpret_cast<WaveLds*>(smem) + wib;
    uint16_t* table = reinterpret_cast<uint16_t*>(smem + sizeof(WaveLds) * p.waves_per_block);
    build_obs_table<0>(table, p);
    init_wave_consts(wl, p, lane);
    const long long head = A.ring.state[0];
    // the record: every lane of a group works it out for itself
    long long idx = -1;
    if (mine) {
        if constexpr (DRAW) {
            const unsigned long long F = ccx_replay::filled(head, A.S, A.E);
            const ccx_replay::Key k = ccx_replay::key_of((unsigned long long)b, (unsigned long long)A.ring.state[1]);
            const uint32_t w0 = random_word(A.seed_lo, A.seed_hi ^ kReplayStream, k.genv, k.episode, k.step, 0u);
            const uint32_t w1 = random_word(A.seed_lo, A.seed_hi ^ kReplayStream, k.genv, k.episode, k.step, 1u);
            idx = ccx_replay::index_of(w0, w1, F);
        } else {
            idx = A.index_in[b];
        }
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
        if (A.obs) me = A.ring.obs_c[at((uint32_t)at0)];
        act = A.ring.actions[at((uint32_t)at0)];
#pragma unroll
        for (int k = 1; k < kMax; ++k) {
            if (k < A.n) {                                               // (n is the launch's: the branch is uniform)
                const uint32_t sk = ccx_nstep::slot_k<uint32_t>(ps, (uint32_t)k, S, E, e);
                ct[k] = A.ring.cut[sk];
                dn[k] = A.ring.done[at(sk)];
                vl[k] = A.ring.valid[at(sk)];
                rw[k] = A.ring.reward[at(sk)];
            }
        }
        ct[0] = A.ring.cut[at0];                                         // (n >= 1: record 0 itself is always read; it comes last
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
        if (A.next_obs) nx = A.ring.next_c[at(sl)];
        mn = A.ring.masks_next[at(sl)];
    }
    const ccx_nstep::Span<uint32_t> sp = ccx_nstep::agent_span(m_env, dn, vl);
    const int m_a = sp.m;
    const ccx_nstep::Return ret = ccx_nstep::returns(m_a, rw, A.gamma);
    const uint32_t done_out = sp.done_out;
    const uint32_t valid_out = ccx_nstep::dropped(m_a, m_env, done_out) ? 0u : vl[0];
    if (mine) {
        const long long to = b * N + i;
        A.actions[to] = act;
        A.reward[to] = ret.G;
        A.done[to] = (uint8_t)done_out;
        A.valid[to] = (uint8_t)valid_out;
        A.masks_next[to] = mn;
        A.discount[to] = ret.discount;
        A.span[to] = (uint8_t)m_a;
        if (i == 0) A.index[b] = idx;
    }
    long long here = A.B - b0;
    here = here < 0 ? 0 : (here > p.EW ? p.EW : here);
    const int units = (int)here * N * (3 + 2 * N);
    const size_t region = (size_t)b0 * (size_t)N * (size_t)L;             // floats in front of this wave's rows
    if (A.obs) wl->slot[lane] = me;                                      // (two stores, not a select between two structs)
    else wl->slot[lane] = nx;
    __syncthreads();                                                     // the table and the tile are in LDS
    if (A.obs) {
        emit_obs<PAIR>(wl, table, reinterpret_cast<char*>(A.obs + region), 0, PAIR ? (units >> 1) : units, lane);
        if (A.next_obs) {
            wave_lds_sync();                                             // the tile has been read before it is rewritten
            wl->slot[lane] = nx;
            wave_lds_sync();
        }
    }
    if (A.next_obs) emit_obs<PAIR>(wl, table, reinterpret_cast<char*>(A.next_obs + region), 0, PAIR ? (units >> 1) : units, lane);
}

// S, the ring's state and the cut bytes: what the two small launches take
int check_cut(const char* who, const ccx_handle* h, int64_t ring_steps, const int64_t* ring_state, const uint8_t* cut) {
    if (!h) return fail(CCX_EINVAL, "NULL handle");
    if (!ring_state || !cut) return fail(CCX_EINVAL, "%s: NULL ring_state or cut", who);
    if (ring_steps < 1 || ring_steps >= (1ll << 31) || ring_steps * (int64_t)h->E >= (1ll << 31))
        return fail(CCX_EINVAL, "%s: ring_steps = %lld out of range (1 <= S, S * E < 2^31)", who, (long long)ring_steps);
    if (misaligned(8, ring_state)) return fail(CCX_EINVAL, "%s: ring_state must be 8-byte aligned", who);
    return CCX_OK;
}

unsigned blocks_of(int64_t n) { return (unsigned)((n + 255) / 256); }     // n < 2^31

// the ring as the ABI passes it: ring_steps and the eight arrays, in ccx_replay_fetch's order
#define CCX_NS_RING_PARAMS int64_t ring_steps, float* ring_obs_c, float* ring_next_c, uint8_t* ring_actions, double* ring_reward, \
                           uint8_t* ring_done, uint8_t* ring_valid, uint8_t* ring_masks_next, int64_t* ring_state
#define CCX_NS_RING_ARGS ring_steps, ring_obs_c, ring_next_c, ring_actions, ring_reward, ring_done, ring_valid, ring_masks_next, ring_state

struct NsOut {
    float* obs;
    float* next_obs;
    uint8_t* actions;
    double* reward;
    uint8_t* done;
    uint8_t* valid;
    uint8_t* masks_next;
    int64_t* index;
    float* discount;
    uint8_t* span;
};

int fetch(const char* who, ccx_handle* h, CCX_NS_RING_PARAMS, const uint8_t* cut, int32_t n, float gamma, int64_t B,
          const int64_t* index_in, const NsOut* out, bool draw) {
    NsArgs A{};
    if (int rc = check_cut(who, h, ring_steps, ring_state, cut)) return rc;
    if (!ring_obs_c || !ring_next_c || !ring_actions || !ring_reward || !ring_done || !ring_valid || !ring_masks_next)
        return fail(CCX_EINVAL, "%s: NULL ring array", who);
    if (misaligned(16, ring_obs_c, ring_next_c)) return fail(CCX_EINVAL, "%s: the ring's compact arrays must be 16-byte aligned", who);
    if (misaligned(8, ring_reward)) return fail(CCX_EINVAL, "%s: the ring's reward must be 8-byte aligned", who);
    if (n < 1 || n > CCX_NSTEP_MAX || (int64_t)n > ring_steps)
        return fail(CCX_EINVAL, "%s: n = %d out of range (1 <= n <= min(ring_steps, %d))", who, (int)n, CCX_NSTEP_MAX);
    if (!(gamma >= 0.0f && gamma <= 1.0f)) return fail(CCX_EINVAL, "%s: gamma must be finite and lie in [0, 1], got %g", who, (double)gamma);
    if (!out->actions || !out->reward || !out->done || !out->valid || !out->masks_next || !out->index || !out->discount || !out->span)
        return fail(CCX_EINVAL, "%s: NULL output (only obs and next_obs may be NULL)", who);
    if (!draw && !index_in) return fail(CCX_EINVAL, "%s: NULL index", who);
    if (B < 1 || B * (int64_t)h->N > (1ll << 31)) return fail(CCX_EINVAL, "%s: batch = %lld out of range (1 <= B <= 2^31 / N)", who, (long long)B);
    if (misaligned(16, out->obs, out->next_obs)) return fail(CCX_EINVAL, "%s: obs and next_obs must be 16-byte aligned", who);
    if (misaligned(8, out->reward, out->index, index_in))
        return fail(CCX_EINVAL, "%s: reward and index must be 8-byte aligned", who);
    if (misaligned(4, out->discount)) return fail(CCX_EINVAL, "%s: discount must be 4-byte aligned", who);
    CCX_HIP(hipSetDevice(h->device));
    const ccx::LaunchShape& ls = h->shape;
    const ccx::KParams& p = h->kp;
    const int64_t per_block = (int64_t)p.EW * p.waves_per_block;
    const int64_t blocks = (B + per_block - 1) / per_block;
    if (blocks > 0x7FFFFFFFll) return fail(CCX_EINVAL, "%s: batch = %lld needs too many workgroups", who, (long long)B);
    A.ring = NsRing{reinterpret_cast<const float4*>(ring_obs_c), reinterpret_cast<const float4*>(ring_next_c), ring_actions, ring_reward,
                    ring_done, ring_valid, ring_masks_next, reinterpret_cast<const long long*>(ring_state), cut};
    A.index_in = reinterpret_cast<const long long*>(index_in);
    A.obs = out->obs;
    A.next_obs = out->next_obs;
    A.actions = out->actions;
    A.reward = out->reward;
    A.done = out->done;
    A.valid = out->valid;
    A.masks_next = out->masks_next;
    A.index = reinterpret_cast<long long*>(out->index);
    A.discount = out->discount;
    A.span = out->span;
    A.B = B;
    A.R = ring_steps * (int64_t)h->E;
    A.S = (int)ring_steps;
    A.E = h->E;
    A.glog = ls.glog;
    A.n = n;
    A.gamma = gamma;
    A.seed_lo = h->rng_lo;
    A.seed_hi = h->rng_hi;
    const dim3 grid((unsigned)blocks), block(64 * ls.waves_per_block);
    with_flags([&](auto drw, auto pair) {
        hipLaunchKernelGGL((nstep_fetch_kernel<decltype(drw)::value, decltype(pair)::value>), grid, block, ls.lds_bytes_observe,
                           h->stream, p, A);
    }, draw, (h->N % 2) == 0);
    if (draw) hipLaunchKernelGGL(nstep_draws_kernel, dim3(1), dim3(64), 0, h->stream, reinterpret_cast<long long*>(ring_state));
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

int ccx_nstep_sample(ccx_handle* h, CCX_NS_RING_PARAMS, const uint8_t* cut, int32_t n, float gamma, int64_t batch, float* obs_or_null,
                     float* next_obs_or_null, uint8_t* actions, double* reward, uint8_t* done, uint8_t* valid, uint8_t* masks_next,
                     int64_t* index, float* discount, uint8_t* span) {
    const NsOut out{obs_or_null, next_obs_or_null, actions, reward, done, valid, masks_next, index, discount, span};
    return fetch("ccx_nstep_sample", h, CCX_NS_RING_ARGS, cut, n, gamma, batch, nullptr, &out, true);
}

int ccx_nstep_fetch(ccx_handle* h, CCX_NS_RING_PARAMS, const uint8_t* cut, int32_t n, float gamma, int64_t batch, const int64_t* index_in,
                    float* obs_or_null, float* next_obs_or_null, uint8_t* actions, double* reward, uint8_t* done, uint8_t* valid,
                    uint8_t* masks_next, int64_t* index, float* discount, uint8_t* span) {
    const NsOut out{obs_or_null, next_obs_or_null, actions, reward, done, valid, masks_next, index, discount, span};
    return fetch("ccx_nstep_fetch", h, CCX_NS_RING_ARGS, cut, n, gamma, batch, index_in, &out, false);
}

}  // extern "C"
