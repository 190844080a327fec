// ccx_replay.hip -- CCX_REPLAY (include/ccx.h): a ring of compact env-step records with its cursor on the device, and ONE
// kernel that draws B records and writes the minibatch as DefaultObservation rows and the small arrays CCX_QLEARN's TD loss
// takes.  The slot map, the draw and the empty record are ccx_replay.h's; the word is ccx_kernels.h's; the rows are written by
// the gather of ccx_observe / ccx_expand_observations (ccx_rollout_dev.h: build_obs_table, emit_obs), called, not restated.
//
// replay_push_kernel: one lane per (step s, env e, agent a) of the block; 16-byte loads and stores for the two compact
// float4s, the small fields next to them.  `head` is read from the device: a captured push advances with every replay.
// replay_fetch_kernel<DRAW, PAIR>: the lane layout of observe_kernel with records in the place of envs -- a wave takes the EW
// records b0 .. b0 + EW - 1 of the minibatch, lane (g, i) agent i of record b0 + g.  Every lane of a group works out the
// record's index (DRAW: the two words and the 128-bit product; else the caller's index[b]), loads its float4 of obs_c and
// of next_c THROUGH the index -- both loads are in flight before the first wait --, and copies the record's small fields.
// The wave's tile then takes the obs_c float4s, the rows of its EW records (ONE contiguous region of obs) leave it through
// emit_obs -- 16-byte stores for an even agent count, 8-byte ones for an odd one --, and the same tile serves next_c.
// replay_head_kernel: one lane adds to head / draws BEHIND the launch that read them: stream order is the only order needed;
// no atomic, no last-block-done counter, no host synchronisation.
#include "ccx_internal.h"
#include "ccx_replay.h"
#include "ccx_rollout_dev.h"

using ccxi::fail;
using ccxi::misaligned;
using ccxi::with_flags;

namespace {

static_assert(ccx_replay::kStream == ccx::kReplayStream, "one constant for the replay stream");
static_assert(ccx_replay::kEmptyAction == CCX_ACTION_ABSENT, "the empty record's action is the absent one");

struct RingArrays {                    // the ring's own storage, [R][N] (compact: [R][N] float4)
    float4* obs_c;
    float4* next_c;
    uint8_t* actions;
    double* reward;
    uint8_t* done;
    uint8_t* valid;
    uint8_t* masks_next;
    long long* state;                  // {head, draws, 0, 0}
};

struct PushArgs {
    RingArrays ring;
    const float4* obs0;                // [E][N]
    const uint8_t* actions;            // [K][E][N]
    const double* reward;              // [K][E][N]
    const uint8_t* agent_flags;        // [K][E][N]
    const uint8_t* env_flags;          // [K][E]
    const float4* obs_compact;         // [K][E][N]
    const float4* final_compact;       // [K][E][N] or null
    const uint8_t* masks_next;         // [K][E][N] or null
    long long total;                   // K E N
    int S, E, N;
};

__global__ __launch_bounds__(256) void replay_push_kernel(const PushArgs A) {
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t >= A.total) return;
    const long long EN = (long long)A.E * A.N;
    const long long s = t / EN, rem = t - s * EN;
    const long long e = rem / A.N, a = rem - e * A.N;
    const long long head = A.ring.state[0];
    const long long at = ccx_replay::slot_of(head, s, A.S, A.E, e) * A.N + a;
    const bool reset = A.final_compact != nullptr && (A.env_flags[s * A.E + e] & CCX_EF_RESET) != 0;
    const float4 first = s == 0 ? A.obs0[rem] : A.obs_compact[t - EN];
    const float4 next = reset ? A.final_compact[t] : A.obs_compact[t];
    const uint32_t af = A.agent_flags[t];
    const uint8_t mn = (reset || A.masks_next == nullptr) ? ccx_replay::kMasksAll : A.masks_next[t];
    A.ring.obs_c[at] = first;
    A.ring.next_c[at] = next;
    A.ring.actions[at] = A.actions[t];
    A.ring.reward[at] = A.reward[t];
    A.ring.done[at] = (uint8_t)(af & CCX_AF_TERMINATED);
    A.ring.valid[at] = (uint8_t)(af & CCX_AF_LIVE);
    A.ring.masks_next[at] = mn;
}

__global__ __launch_bounds__(64) void replay_head_kernel(long long* state, const long long steps, const long long draws) {
    if (threadIdx.x == 0u && blockIdx.x == 0u) {
        state[0] += steps;
        state[1] += draws;
    }
}

struct FetchArgs {
    RingArrays ring;
    const long long* index_in;         // [B]: read where !DRAW
    float* obs;                        // [B][N][L] or null
    float* next_obs;                   // [B][N][L] or null
    uint8_t* actions;                  // [B][N]
    double* reward;
    uint8_t* done;
    uint8_t* valid;
    uint8_t* masks_next;
    long long* index;                  // [B]
    long long B, R;
    int S, E, glog;
    uint32_t seed_lo, seed_hi;
};

template <bool DRAW, bool PAIR>
__global__ __launch_bounds__(256) void replay_fetch_kernel(const ccx::KParams p, const FetchArgs A) {
    using namespace ccx;
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
    // the record: every lane of a group works it out for itself
    long long idx = -1;
    if (mine) {
        if constexpr (DRAW) {
            const unsigned long long F = ccx_replay::filled(A.ring.state[0], A.S, A.E);
            const ccx_replay::Key k = ccx_replay::key_of((unsigned long long)b, (unsigned long long)A.ring.state[1]);
            const uint32_t w0 = random_word(A.seed_lo, A.seed_hi ^ kReplayStream, k.genv, k.episode, k.step, 0u);
            const uint32_t w1 = random_word(A.seed_lo, A.seed_hi ^ kReplayStream, k.genv, k.episode, k.step, 1u);
            idx = ccx_replay::index_of(w0, w1, F);
        } else {
            idx = A.index_in[b];
        }
    }
    const bool read = mine && ccx_replay::in_ring(idx, A.R);
    float4 me = make_float4(0.0f, 0.0f, 0.0f, 0.0f), nx = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    uint8_t act = ccx_replay::kEmptyAction, dn = ccx_replay::kEmptyDone, vl = ccx_replay::kEmptyValid, mn = ccx_replay::kEmptyMasks;
    double rw = ccx_replay::kEmptyReward;
    if (read) {                                                          // (every load is issued before the first wait)
        const long long at = idx * N + i;
        if (A.obs) me = A.ring.obs_c[at];
        if (A.next_obs) nx = A.ring.next_c[at];
        act = A.ring.actions[at];
        rw = A.ring.reward[at];
        dn = A.ring.done[at];
        vl = A.ring.valid[at];
        mn = A.ring.masks_next[at];
    }
    if (mine) {
        const long long to = b * N + i;
        A.actions[to] = act;
        A.reward[to] = rw;
        A.done[to] = dn;
        A.valid[to] = vl;
        A.masks_next[to] = mn;
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

// the ring as the ABI passes it: ring_steps and the eight arrays, in the order of RingArrays
#define CCX_RING_PARAMS int64_t ring_steps, float* ring_obs_c, float* ring_next_c, uint8_t* ring_actions, double* ring_reward, \
                        uint8_t* ring_done, uint8_t* ring_valid, uint8_t* ring_masks_next, int64_t* ring_state
#define CCX_RING_ARGS ring_steps, ring_obs_c, ring_next_c, ring_actions, ring_reward, ring_done, ring_valid, ring_masks_next, ring_state

int check_ring(const char* who, const ccx_handle* h, CCX_RING_PARAMS, RingArrays& a) {
    if (!h) return fail(CCX_EINVAL, "NULL handle");
    if (!ring_obs_c || !ring_next_c || !ring_actions || !ring_reward || !ring_done || !ring_valid || !ring_masks_next || !ring_state)
        return fail(CCX_EINVAL, "%s: NULL ring array", who);
    if (ring_steps < 1 || ring_steps >= (1ll << 31) || ring_steps * (int64_t)h->E >= (1ll << 31))
        return fail(CCX_EINVAL, "%s: ring_steps = %lld out of range (1 <= S, S * E < 2^31)", who, (long long)ring_steps);
    if (misaligned(16, ring_obs_c, ring_next_c)) return fail(CCX_EINVAL, "%s: the ring's compact arrays must be 16-byte aligned", who);
    if (misaligned(8, ring_reward, ring_state))
        return fail(CCX_EINVAL, "%s: the ring's reward and state must be 8-byte aligned", who);
    a.obs_c = reinterpret_cast<float4*>(ring_obs_c);
    a.next_c = reinterpret_cast<float4*>(ring_next_c);
    a.actions = ring_actions;
    a.reward = ring_reward;
    a.done = ring_done;
    a.valid = ring_valid;
    a.masks_next = ring_masks_next;
    a.state = reinterpret_cast<long long*>(ring_state);
    return CCX_OK;
}

struct BatchOut {
    float* obs;
    float* next_obs;
    uint8_t* actions;
    double* reward;
    uint8_t* done;
    uint8_t* valid;
    uint8_t* masks_next;
    int64_t* index;
};

int fetch(const char* who, ccx_handle* h, CCX_RING_PARAMS, int64_t B, const int64_t* index_in, const BatchOut* out, bool draw) {
    FetchArgs A{};
    if (int rc = check_ring(who, h, CCX_RING_ARGS, A.ring)) return rc;
    if (!out->actions || !out->reward || !out->done || !out->valid || !out->masks_next || !out->index)
        return fail(CCX_EINVAL, "%s: NULL output (only obs and next_obs may be NULL)", who);
    if (!draw && !index_in) return fail(CCX_EINVAL, "%s: NULL index", who);
    if (B < 1 || B * (int64_t)h->N > (1ll << 31)) return fail(CCX_EINVAL, "%s: batch = %lld out of range (1 <= B <= 2^31 / N)", who, (long long)B);
    if (misaligned(16, out->obs, out->next_obs)) return fail(CCX_EINVAL, "%s: obs and next_obs must be 16-byte aligned", who);
    if (misaligned(8, out->reward, out->index, index_in))
        return fail(CCX_EINVAL, "%s: reward and index must be 8-byte aligned", who);
    CCX_HIP(hipSetDevice(h->device));
    const ccx::LaunchShape& ls = h->shape;
    const ccx::KParams& p = h->kp;
    const int64_t per_block = (int64_t)p.EW * p.waves_per_block;
    const int64_t blocks = (B + per_block - 1) / per_block;
    if (blocks > 0x7FFFFFFFll) return fail(CCX_EINVAL, "%s: batch = %lld needs too many workgroups", who, (long long)B);
    A.index_in = reinterpret_cast<const long long*>(index_in);
    A.obs = out->obs;
    A.next_obs = out->next_obs;
    A.actions = out->actions;
    A.reward = out->reward;
    A.done = out->done;
    A.valid = out->valid;
    A.masks_next = out->masks_next;
    A.index = reinterpret_cast<long long*>(out->index);
    A.B = B;
    A.R = ring_steps * (int64_t)h->E;
    A.S = (int)ring_steps;
    A.E = h->E;
    A.glog = ls.glog;
    A.seed_lo = h->rng_lo;
    A.seed_hi = h->rng_hi;
    const dim3 grid((unsigned)blocks), block(64 * ls.waves_per_block);
    with_flags([&](auto drw, auto pair) {
        hipLaunchKernelGGL((replay_fetch_kernel<decltype(drw)::value, decltype(pair)::value>), grid, block, ls.lds_bytes_observe,
                           h->stream, p, A);
    }, draw, (h->N % 2) == 0);
    if (draw) hipLaunchKernelGGL(replay_head_kernel, dim3(1), dim3(64), 0, h->stream, A.ring.state, 0ll, 1ll);
    CCX_HIP(hipGetLastError());
    return CCX_OK;
}

}  // namespace

extern "C" {

int ccx_replay_push(ccx_handle* h, CCX_RING_PARAMS, int64_t K, const float* obs0_compact, const uint8_t* actions,
                    const double* reward, const uint8_t* agent_flags, const uint8_t* env_flags, const float* obs_compact,
                    const float* final_compact_or_null, const uint8_t* masks_next_or_null) {
    PushArgs A{};
    if (int rc = check_ring("ccx_replay_push", h, CCX_RING_ARGS, A.ring)) return rc;
    if (!obs0_compact || !actions || !reward || !agent_flags || !env_flags || !obs_compact)
        return fail(CCX_EINVAL, "ccx_replay_push: NULL argument (only final_compact and masks_next may be NULL)");
    if (K < 1 || K > ring_steps)
        return fail(CCX_EINVAL, "ccx_replay_push: K = %lld out of range (1 <= K <= ring_steps = %lld)", (long long)K, (long long)ring_steps);
    if (misaligned(16, obs0_compact, obs_compact, final_compact_or_null))
        return fail(CCX_EINVAL, "ccx_replay_push: obs0_compact, obs_compact and final_compact must be 16-byte aligned");
    if (misaligned(8, reward)) return fail(CCX_EINVAL, "ccx_replay_push: reward must be 8-byte aligned");
    CCX_HIP(hipSetDevice(h->device));
    A.obs0 = reinterpret_cast<const float4*>(obs0_compact);
    A.actions = actions;
    A.reward = reward;
    A.agent_flags = agent_flags;
    A.env_flags = env_flags;
    A.obs_compact = reinterpret_cast<const float4*>(obs_compact);
    A.final_compact = reinterpret_cast<const float4*>(final_compact_or_null);
    A.masks_next = masks_next_or_null;
    A.total = K * (int64_t)h->E * (int64_t)h->N;                        // K E < 2^31, N <= 64
    A.S = (int)ring_steps;
    A.E = h->E;
    A.N = h->N;
    const unsigned blocks = (unsigned)((A.total + 255) / 256);           // below 2^29
    hipLaunchKernelGGL(replay_push_kernel, dim3(blocks), dim3(256), 0, h->stream, A);
    hipLaunchKernelGGL(replay_head_kernel, dim3(1), dim3(64), 0, h->stream, A.ring.state, (long long)K, 0ll);
    CCX_HIP(hipGetLastError());
    return CCX_OK;
}

int ccx_replay_sample(ccx_handle* h, CCX_RING_PARAMS, int64_t batch, float* obs_or_null, float* next_obs_or_null, uint8_t* actions,
                      double* reward, uint8_t* done, uint8_t* valid, uint8_t* masks_next, int64_t* index) {
    const BatchOut out{obs_or_null, next_obs_or_null, actions, reward, done, valid, masks_next, index};
    return fetch("ccx_replay_sample", h, CCX_RING_ARGS, batch, nullptr, &out, true);
}

int ccx_replay_fetch(ccx_handle* h, CCX_RING_PARAMS, int64_t batch, const int64_t* index_in, float* obs_or_null,
                     float* next_obs_or_null, uint8_t* actions, double* reward, uint8_t* done, uint8_t* valid, uint8_t* masks_next,
                     int64_t* index) {
    const BatchOut out{obs_or_null, next_obs_or_null, actions, reward, done, valid, masks_next, index};
    return fetch("ccx_replay_fetch", h, CCX_RING_ARGS, batch, index_in, &out, false);
}

}  // extern "C"
