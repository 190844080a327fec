// ccx_episode_stats.hip -- CCX_EPISODE_STATS (include/ccx.h): per-episode returns and lengths accumulated on the device from
// the reward / flag arrays a step or a rollout wrote, plus an optional log of finished episodes.
//
// The sum of one (env, agent) column is a chain of f64 adds in step order (the reference's `total_reward += reward`,
// examples/waiting_policy_demo.py:52-85): it cannot be reassociated, so the chain is serial by contract.  The LOADS are not:
// one lane owns one column (adjacent lanes = adjacent columns: a wave reads one contiguous piece of a step's reward slab,
// whole lines wherever the agent count divides 64) and keeps
// STATS_CHUNK steps of its column in registers while it consumes the chunk before -- 2 x STATS_CHUNK independent loads per
// stream and lane are in flight, and the add chain never waits for a single HBM miss per step.  Step indices past the end
// of the update are clamped to the last step instead of predicated, so every load of a chunk is unconditional (a
// predicated load makes the compiler wait for each one).  Env-level values (steps, the latch, the record count) are
// computed redundantly by every lane of the env from the same env_flags byte; lane a == 0 writes them.  A wave carries
// WHOLE envs only (64 / N of them; libccx has at most 64 agents per env), so the lanes that read an env's steps / closed /
// finished at entry and the lane that stores them at exit run in lockstep in one wave: no other wave, of this launch or
// a later round of the grid, ever touches them.
//
// With a log an update is three launches: stats_count (records per env, from env_flags and the latch alone), stats_scan
// (exclusive scan over the envs + the log's fill level -> first record slot of every env, stored / dropped counts), then the
// accumulate kernel writes each record to its slot.  No atomics: the log order is env-major by construction.
#include "ccx_internal.h"

using ccxi::fail;

namespace {

constexpr int STATS_CHUNK = 16;       // steps of one column held in registers per chunk (tests: K = 15, 16, 17)
constexpr int COUNT_CHUNK = 32;       // env_flags bytes per chunk of the count kernel
constexpr int SCAN_THREADS = 1024;

struct StatsArgs {
    ccx_episode_stats v;
    int32_t E, N;
    int32_t envs_per_wave;             // 64 / N
    long long EN;
    long long env_offset;
};

__device__ __forceinline__ long long clamped(int s, int K) { return s < K ? s : K - 1; }

// One step of the CCX_EPISODE_STATS rule for one column.  Env-level registers (steps, closed, finished, nrec) take the same
// values in every lane of the env.  The common step -- no flag raised in env_flags -- is branch-free: the add is computed
// and kept or dropped by a select (a reward that is not live never reaches `ret`); everything else sits behind ONE test
// of the env_flags byte.
#define STATS_STEP(R, AF, EF)                                                                          \
    do {                                                                                               \
        const bool add_ = !closed && ((AF) & CCX_AF_LIVE);                                             \
        const double sum_ = ret + (R);                                                                 \
        ret = add_ ? sum_ : ret;                                                                       \
        live += add_ ? 1 : 0;                                                                          \
        steps += closed ? 0 : 1;                                                                       \
        if ((EF) & (CCX_EF_ALL_TERMINATED | CCX_EF_ALL_TRUNCATED | CCX_EF_RESET)) {                    \
            if (((EF) & (CCX_EF_ALL_TERMINATED | CCX_EF_ALL_TRUNCATED)) && !closed) {                  \
                if (LOG) {                                                                             \
                    const long long pos = base + nrec;                                                 \
                    if (pos < A.v.log_capacity) {                                                      \
                        A.v.log_ret[pos * A.N + a] = ret;                                              \
                        A.v.log_live_steps[pos * A.N + a] = live;                                      \
                        if (a == 0) {                                                                  \
                            A.v.log_env[pos] = A.env_offset + e;                                       \
                            A.v.log_episode[pos] = finished;                                           \
                            A.v.log_steps[pos] = steps;                                                \
                            A.v.log_end[pos] = (uint8_t)((EF) & 3u);                                   \
                        }                                                                              \
                    }                                                                                  \
                }                                                                                      \
                l_ret = ret; l_live = live; l_steps = steps; l_end = (uint8_t)((EF) & 3u);             \
                finished += 1; nrec += 1; closed = 1;                                                  \
            }                                                                                          \
            if ((EF) & CCX_EF_RESET) { ret = 0.0; live = 0; steps = 0; closed = 0; }                   \
        }                                                                                              \
    } while (0)

template <bool LOG, bool NAIVE>
__global__ __launch_bounds__(64) void stats_accumulate(const StatsArgs A, const int K, const double* __restrict__ reward,
                                                       const uint8_t* __restrict__ aflags,
                                                       const uint8_t* __restrict__ eflags,
                                                       const long long* __restrict__ log_base) {
    // whole envs per wave: lane t carries agent t % N of the wave's env t / N; the last 64 % N lanes carry nothing
    const int t = (int)threadIdx.x;
    const int el = t / A.N;
    const long long e64 = (long long)blockIdx.x * A.envs_per_wave + el;
    if (el >= A.envs_per_wave || e64 >= A.E) return;
    const int e = (int)e64;
    const int a = t - el * A.N;
    const long long col = e64 * A.N + a;
    double ret = A.v.ret[col];
    int32_t live = A.v.live_steps[col];
    int32_t steps = A.v.steps[e];
    int32_t closed = A.v.closed[e];
    int32_t finished = A.v.finished[e];
    const long long base = LOG ? log_base[e] : 0;
    int32_t nrec = 0;
    double l_ret = 0.0;
    int32_t l_live = 0, l_steps = 0;
    uint8_t l_end = 0;

    const double* rp = reward + col;
    const uint8_t* ap = aflags + col;
    const uint8_t* ep = eflags + e;
    if (K == 1) {                                               // the step-wise loop: nothing to pipeline
        const double r = rp[0];
        const uint8_t af = ap[0];
        const uint8_t ef = ep[0];
        STATS_STEP(r, af, ef);
    } else if constexpr (NAIVE) {
        // the loop the header warns about: one dependent trip to memory per step (kept for the timing table only,
        // tunable "stats_naive")
#pragma unroll 1
        for (int s = 0; s < K; ++s) {
            const double r = rp[(long long)s * A.EN];
            const uint8_t af = ap[(long long)s * A.EN];
            const uint8_t ef = ep[(long long)s * A.E];
            STATS_STEP(r, af, ef);
        }
    } else {
        // Two register chunks, the loop unrolled by two by hand: while chunk A is consumed the loads of chunk B are in
        // flight and the other way round (a copy B -> A at the end of an iteration would be a USE of every loaded register
        // and make the wave wait for all of them there).
        double rA[STATS_CHUNK], rB[STATS_CHUNK];
        uint8_t afA[STATS_CHUNK], afB[STATS_CHUNK], efA[STATS_CHUNK], efB[STATS_CHUNK];
#define STATS_LOAD(RR, AA, EE, S0)                                                                     \
    _Pragma("unroll") for (int i = 0; i < STATS_CHUNK; ++i) {                                          \
        const long long s = clamped((S0) + i, K);                                                      \
        RR[i] = rp[s * A.EN];                                                                          \
        AA[i] = ap[s * A.EN];                                                                          \
        EE[i] = ep[s * A.E];                                                                           \
    }
#define STATS_CONSUME(RR, AA, EE, S0)                                                                  \
    if ((S0) + STATS_CHUNK <= K) {                                                                     \
        _Pragma("unroll") for (int i = 0; i < STATS_CHUNK; ++i) STATS_STEP(RR[i], AA[i], EE[i]);       \
    } else {                                                                                           \
        _Pragma("unroll") for (int i = 0; i < STATS_CHUNK; ++i)                                        \
            if ((S0) + i < K) STATS_STEP(RR[i], AA[i], EE[i]);                                         \
    }
        STATS_LOAD(rA, afA, efA, 0)
        for (int s0 = 0; s0 < K; s0 += 2 * STATS_CHUNK) {
            // (the loads are unconditional -- past the end they hit the last step's lines again -- so that the number of
            // loads in flight is known at every wait and the compiler waits for the consumed chunk only)
            STATS_LOAD(rB, afB, efB, s0 + STATS_CHUNK)
            STATS_CONSUME(rA, afA, efA, s0)
            STATS_LOAD(rA, afA, efA, s0 + 2 * STATS_CHUNK)
            if (s0 + STATS_CHUNK < K) { STATS_CONSUME(rB, afB, efB, s0 + STATS_CHUNK) }
        }
#undef STATS_LOAD
#undef STATS_CONSUME
    }

    A.v.ret[col] = ret;
    A.v.live_steps[col] = live;
    if (nrec) {
        A.v.last_ret[col] = l_ret;
        A.v.last_live_steps[col] = l_live;
    }
    if (a == 0) {
        A.v.steps[e] = steps;
        A.v.closed[e] = (uint8_t)closed;
        if (nrec) {
            A.v.finished[e] = finished;
            A.v.last_steps[e] = l_steps;
            A.v.last_end[e] = l_end;
        }
    }
}

// records env e emits in this update: the latch automaton on env_flags alone
__global__ __launch_bounds__(64) void stats_count(const int E, const int K, const uint8_t* __restrict__ eflags,
                                                  const uint8_t* __restrict__ closed_in, int32_t* __restrict__ count) {
    const int e = blockIdx.x * 64 + threadIdx.x;
    if (e >= E) return;
    int32_t closed = closed_in[e], n = 0;
    const uint8_t* ep = eflags + e;
    for (int s0 = 0; s0 < K; s0 += COUNT_CHUNK) {
        uint8_t ef[COUNT_CHUNK];
#pragma unroll
        for (int i = 0; i < COUNT_CHUNK; ++i) ef[i] = ep[clamped(s0 + i, K) * E];
#pragma unroll
        for (int i = 0; i < COUNT_CHUNK; ++i) {
            if (s0 + i < K) {
                if ((ef[i] & (CCX_EF_ALL_TERMINATED | CCX_EF_ALL_TRUNCATED)) && !closed) { n += 1; closed = 1; }
                if (ef[i] & CCX_EF_RESET) closed = 0;
            }
        }
    }
    count[e] = n;
}

// base[e] = stored + sum of count[0..e); then stored / dropped take the update's records.  One workgroup: thread t owns the
// contiguous envs [t * per, (t + 1) * per).
__global__ __launch_bounds__(SCAN_THREADS) void stats_scan(const int E, const int32_t* __restrict__ count,
                                                           long long* __restrict__ base,
                                                           unsigned long long* __restrict__ log_count,
                                                           const long long capacity) {
    __shared__ long long part[SCAN_THREADS];
    const int t = threadIdx.x;
    const unsigned long long stored = log_count[0];
    const int per = (E + SCAN_THREADS - 1) / SCAN_THREADS;
    const int lo = t * per < E ? t * per : E;
    const int hi = lo + per < E ? lo + per : E;
    long long sum = 0;
    for (int e = lo; e < hi; ++e) sum += count[e];
    part[t] = sum;
    __syncthreads();
    for (int d = 1; d < SCAN_THREADS; d <<= 1) {                 // inclusive scan of the per-thread sums
        const long long add = t >= d ? part[t - d] : 0;
        __syncthreads();
        part[t] += add;
        __syncthreads();
    }
    long long run = (long long)stored + part[t] - sum;
    for (int e = lo; e < hi; ++e) {
        base[e] = run;
        run += count[e];
    }
    if (t == 0) {
        const unsigned long long total = stored + (unsigned long long)part[SCAN_THREADS - 1];
        const unsigned long long kept = total < (unsigned long long)capacity ? total : (unsigned long long)capacity;
        log_count[0] = kept;
        log_count[1] += total - kept;
    }
}

__global__ __launch_bounds__(64) void stats_reset(const StatsArgs A, const uint8_t* __restrict__ mask) {
    const long long col = (long long)blockIdx.x * 64 + threadIdx.x;
    if (col >= A.EN) return;
    const int e = (int)(col / A.N);
    if (mask && !mask[e]) return;
    A.v.ret[col] = 0.0;
    A.v.live_steps[col] = 0;
    if (col == (long long)e * A.N) {
        A.v.steps[e] = 0;
        A.v.closed[e] = 0;
    }
}

StatsArgs stats_args(const ccx_handle* h) {
    StatsArgs A;
    A.v = h->stats;
    A.E = h->E;
    A.N = h->N;
    A.envs_per_wave = 64 / h->N;
    A.EN = (long long)h->E * h->N;
    A.env_offset = h->env_offset;
    return A;
}

// What one update enqueues, in order.  ccx_episode_stats_update walks this list and ccx_episode_stats_launches counts it,
// so the documented launch count cannot drift from the launches made.
enum StatsStage { STAGE_COUNT, STAGE_SCAN, STAGE_ACCUMULATE };
struct StatsPlan {
    StatsStage stage[3];
    int n = 0;
    bool log = false;
};
StatsPlan stats_plan(const ccx_handle* h) {
    StatsPlan p;
    p.log = h->stats.log_capacity > 0;
    if (p.log) {
        p.stage[p.n++] = STAGE_COUNT;
        p.stage[p.n++] = STAGE_SCAN;
    }
    p.stage[p.n++] = STAGE_ACCUMULATE;
    return p;
}

void stats_free(ccx_handle* h) {
    (void)hipFree(h->stats_slab);
    h->stats_slab = nullptr;
    h->stats = ccx_episode_stats{};
    h->stats_count = nullptr;
    h->stats_base = nullptr;
    h->stats_on = false;
}

}  // namespace

namespace ccxi {

int episode_stats_reset(ccx_handle* h, const uint8_t* env_mask) {
    const StatsArgs A = stats_args(h);
    const unsigned blocks = (unsigned)((A.EN + 63) / 64);
    hipLaunchKernelGGL(stats_reset, dim3(blocks), dim3(64), 0, h->stream, A, env_mask);
    CCX_HIP(hipGetLastError());
    return CCX_OK;
}

void episode_stats_destroy(ccx_handle* h) { stats_free(h); }

}  // namespace ccxi

extern "C" {

int ccx_episode_stats_enable(ccx_handle* h, int64_t log_capacity) {
    if (!h) return fail(CCX_EINVAL, "NULL handle");
    if (log_capacity < 0) return fail(CCX_EINVAL, "log_capacity %lld is negative", (long long)log_capacity);
    CCX_HIP(hipSetDevice(h->device));
    CCX_HIP(hipStreamSynchronize(h->stream));
    stats_free(h);
    const size_t E = (size_t)h->E, EN = E * (size_t)h->N, C = (size_t)log_capacity, CN = C * (size_t)h->N;
    size_t total = 0;
    auto take = [&total](size_t bytes) {
        const size_t at = total;
        total += (bytes + 255) & ~(size_t)255;
        return at;
    };
    const size_t o_ret = take(EN * 8), o_live = take(EN * 4), o_steps = take(E * 4), o_closed = take(E),
                 o_fin = take(E * 4), o_lret = take(EN * 8), o_llive = take(EN * 4), o_lsteps = take(E * 4),
                 o_lend = take(E), o_count = take(16), o_cnt = take(E * 4), o_base = take(E * 8),
                 o_genv = take(C * 8), o_gep = take(C * 4), o_gsteps = take(C * 4), o_gend = take(C),
                 o_gret = take(CN * 8), o_glive = take(CN * 4);
    uint8_t* slab = nullptr;
    if (hipMalloc(&slab, total) != hipSuccess) {
        (void)hipGetLastError();
        return fail(CCX_ENOMEM, "episode stats: %zu bytes of device memory (log_capacity %lld)", total,
                    (long long)log_capacity);
    }
    hipError_t e = hipMemsetAsync(slab, 0, total, h->stream);      // on the handle's own stream, then wait for that stream
    if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
    if (e != hipSuccess) {
        (void)hipFree(slab);
        return fail(CCX_EHIP, "zeroing the episode stats failed: %s", hipGetErrorString(e));
    }
    h->stats_slab = slab;
    ccx_episode_stats& v = h->stats;
    v.ret = (double*)(slab + o_ret);
    v.live_steps = (int32_t*)(slab + o_live);
    v.steps = (int32_t*)(slab + o_steps);
    v.closed = slab + o_closed;
    v.finished = (int32_t*)(slab + o_fin);
    v.last_ret = (double*)(slab + o_lret);
    v.last_live_steps = (int32_t*)(slab + o_llive);
    v.last_steps = (int32_t*)(slab + o_lsteps);
    v.last_end = slab + o_lend;
    v.log_count = (uint64_t*)(slab + o_count);
    v.log_env = C ? (int64_t*)(slab + o_genv) : nullptr;
    v.log_episode = C ? (int32_t*)(slab + o_gep) : nullptr;
    v.log_steps = C ? (int32_t*)(slab + o_gsteps) : nullptr;
    v.log_end = C ? slab + o_gend : nullptr;
    v.log_ret = C ? (double*)(slab + o_gret) : nullptr;
    v.log_live_steps = C ? (int32_t*)(slab + o_glive) : nullptr;
    v.log_capacity = log_capacity;
    h->stats_count = (int32_t*)(slab + o_cnt);
    h->stats_base = (long long*)(slab + o_base);
    h->stats_on = true;
    return CCX_OK;
}

int ccx_episode_stats_disable(ccx_handle* h) {
    if (!h) return fail(CCX_EINVAL, "NULL handle");
    CCX_HIP(hipSetDevice(h->device));
    CCX_HIP(hipStreamSynchronize(h->stream));
    stats_free(h);
    return CCX_OK;
}

int ccx_episode_stats_view(ccx_handle* h, ccx_episode_stats* out) {
    if (!h || !out) return fail(CCX_EINVAL, "NULL argument");
    if (!h->stats_on) return fail(CCX_EINVAL, "episode stats are not enabled (ccx_episode_stats_enable)");
    *out = h->stats;
    return CCX_OK;
}

int ccx_episode_stats_launches(ccx_handle* h, int32_t* launches) {
    if (!h || !launches) return fail(CCX_EINVAL, "NULL argument");
    if (!h->stats_on) return fail(CCX_EINVAL, "episode stats are not enabled (ccx_episode_stats_enable)");
    *launches = stats_plan(h).n;
    return CCX_OK;
}

int ccx_episode_stats_update(ccx_handle* h, int32_t num_steps, const double* reward, const uint8_t* agent_flags,
                             const uint8_t* env_flags) {
    if (!h || !reward || !agent_flags || !env_flags) return fail(CCX_EINVAL, "NULL argument");
    if (!h->stats_on) return fail(CCX_EINVAL, "episode stats are not enabled (ccx_episode_stats_enable)");
    if (num_steps < 1) return fail(CCX_EINVAL, "num_steps = %d", num_steps);
    CCX_HIP(hipSetDevice(h->device));
    const StatsArgs A = stats_args(h);
    const unsigned blocks = (unsigned)((h->E + A.envs_per_wave - 1) / A.envs_per_wave);
    const bool naive = h->tun_stats_naive != 0;
    const StatsPlan plan = stats_plan(h);
    const long long* base = plan.log ? (const long long*)h->stats_base : nullptr;
    for (int i = 0; i < plan.n; ++i) {
        switch (plan.stage[i]) {
        case STAGE_COUNT:
            hipLaunchKernelGGL(stats_count, dim3((unsigned)((h->E + 63) / 64)), dim3(64), 0, h->stream, h->E, num_steps,
                               env_flags, (const uint8_t*)h->stats.closed, h->stats_count);
            break;
        case STAGE_SCAN:
            hipLaunchKernelGGL(stats_scan, dim3(1), dim3(SCAN_THREADS), 0, h->stream, h->E, (const int32_t*)h->stats_count,
                               h->stats_base, (unsigned long long*)h->stats.log_count, (long long)h->stats.log_capacity);
            break;
        case STAGE_ACCUMULATE:
            ccxi::with_flags([&](auto log, auto nv) {
                hipLaunchKernelGGL((stats_accumulate<decltype(log)::value, decltype(nv)::value>), dim3(blocks), dim3(64), 0,
                                   h->stream, A, num_steps, reward, agent_flags, env_flags, base);
            }, plan.log, naive);
            break;
        }
    }
    CCX_HIP(hipGetLastError());
    return CCX_OK;
}

int ccx_episode_stats_reset(ccx_handle* h, const uint8_t* env_mask) {
    if (!h) return fail(CCX_EINVAL, "NULL handle");
    if (!h->stats_on) return fail(CCX_EINVAL, "episode stats are not enabled (ccx_episode_stats_enable)");
    CCX_HIP(hipSetDevice(h->device));
    return ccxi::episode_stats_reset(h, env_mask);
}

int ccx_episode_log_clear(ccx_handle* h) {
    if (!h) return fail(CCX_EINVAL, "NULL handle");
    if (!h->stats_on) return fail(CCX_EINVAL, "episode stats are not enabled (ccx_episode_stats_enable)");
    CCX_HIP(hipSetDevice(h->device));
    CCX_HIP(hipMemsetAsync(h->stats.log_count, 0, 16, h->stream));
    return CCX_OK;
}

}  // extern "C"
