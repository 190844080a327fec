// ccx_gae.hip -- CCX_GAE (include/ccx.h): generalised advantage estimates and value targets of a rollout's reward / flag
// arrays and a critic's values, walked backwards over the steps.
//
// The recurrence of one (env, agent) column -- adv[s] = delta[s] + gl * adv[s+1], cut wherever an episode ends -- is a chain
// of f32 operations in step order: serial by contract, like the sums of ccx_episode_stats.hip, and built the same way.  One
// lane owns one column, adjacent lanes own adjacent columns (flat column index: a wave reads contiguous pieces of every
// step's slabs; nothing on the output side is per env, so a wave need not hold whole envs).  A lane keeps GAE_CHUNK steps of
// its four input streams (reward, agent_flags, env_flags, values) in registers while it consumes the chunk before: the loads
// of two chunks are in flight and the chain never waits for one HBM miss per step.  Step indices below 0 are clamped to step
// 0 instead of predicated, so every load of a chunk is unconditional and the compiler waits for the consumed chunk only.
// values[s+1] is the register the step consumed before held (it starts as last_values, where the carry is +0.0 anyway: the
// rule's `s == K-1` case needs no test).  final_values is read at cut steps only, under the (rare) branch.
// Everything a step does not read is SELECTED away before any arithmetic: a NaN at such a place never reaches a result.
#include "ccx_internal.h"

using ccxi::fail;

namespace {

#ifndef CCX_GAE_CHUNK
// Steps of one column held in registers per chunk (tests: K = 7, 8, 9, 15, 16, 17, 34).  A wave's counter of memory
// operations in flight has 6 bits: four loads per step x two chunks of 8 are 64, so the wait in front of the first step of a
// chunk (60 younger operations) can still be expressed; with chunks of 16 it saturates and the wave waits for the chunk it
// has just requested.  The choice rests on the wait counts in the assembly.
#define CCX_GAE_CHUNK 8
#endif
#ifndef CCX_GAE_LANES
#define CCX_GAE_LANES 64              // columns a wave carries (experiment: 32 spreads the same columns over twice the waves)
#endif
constexpr int GAE_CHUNK = CCX_GAE_CHUNK;
constexpr int GAE_LANES = CCX_GAE_LANES;
static_assert(GAE_LANES >= 1 && GAE_LANES <= 64, "a wave has 64 lanes");

struct GaeArgs {
    const double* reward;
    const uint8_t* aflags;
    const uint8_t* eflags;
    const float* values;
    const float* last_values;
    const float* final_values;         // read only where FINAL
    float* adv;
    float* ret;
    uint8_t* valid;                    // written only where VALID
    long long EN;
    int32_t E, N, K;
    float gamma, gl;
};

__device__ __forceinline__ long long floored(int s) { return s > 0 ? s : 0; }

// One step of the CCX_GAE rule for one column; S is the step's index, vnext the value register of step S + 1.
#define GAE_STEP(S, R, AF, EF, V)                                                                      \
    do {                                                                                               \
        const long long at_ = (long long)(S) * A.EN;                                                   \
        const bool live_ = ((AF) & CCX_AF_LIVE) != 0;                                                  \
        const bool term_ = ((AF) & CCX_AF_TERMINATED) != 0;                                            \
        const bool cut_ = ((AF) & CCX_AF_TRUNCATED) ||                                                 \
                          ((EF) & (CCX_EF_ALL_TERMINATED | CCX_EF_ALL_TRUNCATED | CCX_EF_RESET));      \
        float boot_ = 0.0f;                                                                            \
        if (FINAL) {                                                                                   \
            if (live_ && cut_ && !term_) boot_ = fp[at_];                                              \
        }                                                                                              \
        const bool ends_ = term_ || cut_;                                                              \
        const float nv_ = term_ ? 0.0f : (cut_ ? boot_ : vnext);                                       \
        const float c_ = ends_ ? 0.0f : carry;                                                         \
        const float r_ = (float)(R);                                                                   \
        const float delta_ = (r_ + A.gamma * nv_) - (V);                                               \
        const float adv_ = delta_ + A.gl * c_;                                                         \
        const float ret_ = adv_ + (V);                                                                 \
        carry = live_ ? adv_ : 0.0f;                                                                   \
        vnext = (V);                                                                                   \
        advp[at_] = carry;                                                                             \
        retp[at_] = live_ ? ret_ : 0.0f;                                                               \
        if (VALID) validp[at_] = live_ ? 1 : 0;                                                        \
    } while (0)

template <bool FINAL, bool VALID>
__global__ __launch_bounds__(64) void gae_kernel(const GaeArgs A) {
    const int t = (int)threadIdx.x;
    const long long col = (long long)blockIdx.x * GAE_LANES + t;
    if (t >= GAE_LANES || col >= A.EN) return;
    const long long e = col / A.N;
    const int K = A.K;
    const double* rp = A.reward + col;
    const uint8_t* ap = A.aflags + col;
    const uint8_t* ep = A.eflags + e;
    const float* vp = A.values + col;
    const float* fp = FINAL ? A.final_values + col : nullptr;
    float* advp = A.adv + col;
    float* retp = A.ret + col;
    uint8_t* validp = VALID ? A.valid + col : nullptr;
    float vnext = A.last_values[col];
    float carry = 0.0f;

    if (K == 1) {                                               // one step: nothing to pipeline
        const double r = rp[0];
        const uint8_t af = ap[0];
        const uint8_t ef = ep[0];
        const float v = vp[0];
        GAE_STEP(0, r, af, ef, v);
        return;
    }
    // Two register chunks, the loop unrolled by two by hand (ccx_episode_stats.hip): while chunk A is consumed the loads
    // of chunk B are in flight and the other way round.  Element i of a chunk that starts at S0 is step S0 - i.
    double rA[GAE_CHUNK], rB[GAE_CHUNK];
    float vA[GAE_CHUNK], vB[GAE_CHUNK];
    uint8_t afA[GAE_CHUNK], afB[GAE_CHUNK], efA[GAE_CHUNK], efB[GAE_CHUNK];
#define GAE_LOAD(RR, AA, EE, VV, S0)                                                                   \
    _Pragma("unroll") for (int i = 0; i < GAE_CHUNK; ++i) {                                            \
        const long long s = floored((S0) - i);                                                         \
        RR[i] = rp[s * A.EN];                                                                          \
        AA[i] = ap[s * A.EN];                                                                          \
        EE[i] = ep[s * A.E];                                                                           \
        VV[i] = vp[s * A.EN];                                                                          \
    }
#define GAE_CONSUME(RR, AA, EE, VV, S0)                                                                \
    if ((S0) - (GAE_CHUNK - 1) >= 0) {                                                                 \
        _Pragma("unroll") for (int i = 0; i < GAE_CHUNK; ++i) GAE_STEP((S0) - i, RR[i], AA[i], EE[i], VV[i]); \
    } else {                                                                                           \
        _Pragma("unroll") for (int i = 0; i < GAE_CHUNK; ++i)                                          \
            if ((S0) - i >= 0) GAE_STEP((S0) - i, RR[i], AA[i], EE[i], VV[i]);                         \
    }
    GAE_LOAD(rA, afA, efA, vA, K - 1)
    for (int s0 = K - 1; s0 >= 0; s0 -= 2 * GAE_CHUNK) {
        // (the loads are unconditional -- below step 0 they hit step 0's lines again -- so that the number of loads in
        // flight is known at every wait)
        GAE_LOAD(rB, afB, efB, vB, s0 - GAE_CHUNK)
        GAE_CONSUME(rA, afA, efA, vA, s0)
        GAE_LOAD(rA, afA, efA, vA, s0 - 2 * GAE_CHUNK)
        if (s0 - GAE_CHUNK >= 0) { GAE_CONSUME(rB, afB, efB, vB, s0 - GAE_CHUNK) }
    }
#undef GAE_LOAD
#undef GAE_CONSUME
}

bool unit_interval(float x) { return x >= 0.0f && x <= 1.0f; }      // false for NaN

}  // namespace

extern "C" {

int ccx_gae(ccx_handle* h, int32_t num_steps, const double* reward, const uint8_t* agent_flags, const uint8_t* env_flags,
            const float* values, const float* last_values, const float* final_values_or_null, float gamma, float lam,
            float* advantages, float* returns, uint8_t* valid_or_null) {
    if (!h) return fail(CCX_EINVAL, "NULL handle");
    if (!reward || !agent_flags || !env_flags || !values || !last_values || !advantages || !returns)
        return fail(CCX_EINVAL, "ccx_gae: NULL argument (only final_values and valid may be NULL)");
    if (num_steps < 1) return fail(CCX_EINVAL, "num_steps = %d", num_steps);
    if (!unit_interval(gamma)) return fail(CCX_EINVAL, "ccx_gae: gamma = %g is not in [0, 1]", (double)gamma);
    if (!unit_interval(lam)) return fail(CCX_EINVAL, "ccx_gae: lam = %g is not in [0, 1]", (double)lam);
    CCX_HIP(hipSetDevice(h->device));
    GaeArgs A;
    A.reward = reward;
    A.aflags = agent_flags;
    A.eflags = env_flags;
    A.values = values;
    A.last_values = last_values;
    A.final_values = final_values_or_null;
    A.adv = advantages;
    A.ret = returns;
    A.valid = valid_or_null;
    A.EN = (long long)h->E * h->N;
    A.E = h->E;
    A.N = h->N;
    A.K = num_steps;
    A.gamma = gamma;
    A.gl = gamma * lam;                                             // one f32 multiply (-ffp-contract=off)
    const unsigned blocks = (unsigned)((A.EN + GAE_LANES - 1) / GAE_LANES);
    ccxi::with_flags([&](auto fin, auto val) {
        hipLaunchKernelGGL((gae_kernel<decltype(fin)::value, decltype(val)::value>), dim3(blocks), dim3(64), 0, h->stream, A);
    }, final_values_or_null != nullptr, valid_or_null != nullptr);
    CCX_HIP(hipGetLastError());
    return CCX_OK;
}

}  // extern "C"
