// ccx_replay.hip -- CCX_REPLAY (include/ccx.h): a ring of compact env-step records with its cursor on the device, and ONE
// kernel that draws B records and writes the minibatch as DefaultObservation rows and the small arrays CCX_QLEARN's TD loss
// takes.  The slot map, the draw's rule and the empty record are ccx_replay.h's; the word is ccx_kernels.h's; the lane layout,
// the draw, the wave's tile and the emission of the rows are ccx_gather.h's, the ring as the ABI passes it and the launch's
// checks and grid ccx_internal.h's: called, not restated.
//
// replay_push_kernel: one lane per (step s, env e, agent a) of the block; 16-byte loads and stores for the two compact
// float4s, the small fields next to them.  `head` is read from the device: a captured push advances with every replay.
// replay_fetch_kernel<DRAW, PAIR>: a record-gather wave (ccx_gather.h).  Every lane of a group works out the record's index
// (DRAW: ring_draw; else the caller's index[b]), loads its float4 of obs_c and of next_c THROUGH the index -- both loads are
// in flight before the first wait --, and copies the record's small fields; emit_rows writes the rows of both outputs.
// replay_head_kernel: one lane adds to head / draws BEHIND the launch that read them: stream order is the only order needed;
// no atomic, no last-block-done counter, no host synchronisation.
#include "ccx_internal.h"
#include "ccx_gather.h"

using ccxi::BatchOut;
using ccxi::fail;
using ccxi::FetchArgs;
using ccxi::misaligned;
using ccxi::RingArrays;
using ccxi::with_flags;

namespace {

static_assert(ccx_replay::kStream == ccx::kReplayStream, "one constant for the replay stream");
static_assert(ccx_replay::kEmptyAction == CCX_ACTION_ABSENT, "the empty record's action is the absent one");

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

template <bool DRAW, bool PAIR>
__global__ __launch_bounds__(256) void replay_fetch_kernel(const ccx::KParams p, const FetchArgs A) {
    extern __shared__ __align__(16) unsigned char smem[];
    const ccx_gather::Lane l = ccx_gather::lane_of(p, A.glog, A.B);
    const int N = l.N, i = l.i;
    const long long b = l.b;
    const bool mine = l.mine;
    const ccx_gather::Tile tile = ccx_gather::tile_of(smem, p, l);
    // the record: every lane of a group works it out for itself
    long long idx = -1;
    if (mine) {
        if constexpr (DRAW) idx = ccx_gather::ring_draw(b, A.ring.state[0], A.ring.state[1], A.S, A.E, A.seed_lo, A.seed_hi);
        else idx = A.index_in[b];
    }
    const bool read = mine && ccx_replay::in_ring(idx, A.R);
    float4 me = make_float4(0.0f, 0.0f, 0.0f, 0.0f), nx = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    uint8_t act = ccx_replay::kEmptyAction, dn = ccx_replay::kEmptyDone, vl = ccx_replay::kEmptyValid, mn = ccx_replay::kEmptyMasks;
    double rw = ccx_replay::kEmptyReward;
    if (read) {                                                          // (every load is issued before the first wait)
        const long long at = idx * N + i;
        if (A.out.obs) me = A.ring.obs_c[at];
        if (A.out.next_obs) nx = A.ring.next_c[at];
        act = A.ring.actions[at];
        rw = A.ring.reward[at];
        dn = A.ring.done[at];
        vl = A.ring.valid[at];
        mn = A.ring.masks_next[at];
    }
    if (mine) {
        const long long to = b * N + i;
        A.out.actions[to] = act;
        A.out.reward[to] = rw;
        A.out.done[to] = dn;
        A.out.valid[to] = vl;
        A.out.masks_next[to] = mn;
        if (i == 0) A.out.index[b] = idx;
    }
    ccx_gather::emit_rows<PAIR>(tile, p, l, A.B, A.out.obs, A.out.next_obs, me, nx);
}

int fetch(const char* who, ccx_handle* h, CCX_RING_PARAMS, int64_t B, const int64_t* index_in, const BatchOut& out, bool draw) {
    FetchArgs A{};
    dim3 grid, block;
    if (int rc = ccxi::fetch_args(who, h, CCX_RING_ARGS, B, index_in, out, draw, A, grid, block)) return rc;
    CCX_HIP(hipSetDevice(h->device));
    with_flags([&](auto drw, auto pair) {
        hipLaunchKernelGGL((replay_fetch_kernel<decltype(drw)::value, decltype(pair)::value>), grid, block, h->shape.lds_bytes_observe,
                           h->stream, h->kp, A);
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
    if (int rc = ccxi::check_ring("ccx_replay_push", h, CCX_RING_ARGS, A.ring)) return rc;
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
    hipLaunchKernelGGL(replay_push_kernel, dim3(ccxi::blocks_of(A.total)), dim3(256), 0, h->stream, A);
    hipLaunchKernelGGL(replay_head_kernel, dim3(1), dim3(64), 0, h->stream, A.ring.state, (long long)K, 0ll);
    CCX_HIP(hipGetLastError());
    return CCX_OK;
}

int ccx_replay_sample(ccx_handle* h, CCX_RING_PARAMS, int64_t batch, float* obs_or_null, float* next_obs_or_null, uint8_t* actions,
                      double* reward, uint8_t* done, uint8_t* valid, uint8_t* masks_next, int64_t* index) {
    return fetch("ccx_replay_sample", h, CCX_RING_ARGS, batch, nullptr,
                 BatchOut{obs_or_null, next_obs_or_null, actions, reward, done, valid, masks_next, index}, true);
}

int ccx_replay_fetch(ccx_handle* h, CCX_RING_PARAMS, int64_t batch, const int64_t* index_in, float* obs_or_null,
                     float* next_obs_or_null, uint8_t* actions, double* reward, uint8_t* done, uint8_t* valid, uint8_t* masks_next,
                     int64_t* index) {
    return fetch("ccx_replay_fetch", h, CCX_RING_ARGS, batch, index_in,
                 BatchOut{obs_or_null, next_obs_or_null, actions, reward, done, valid, masks_next, index}, false);
}

}  // extern "C"
