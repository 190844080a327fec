// ccx_draw.h -- the slot rule of CCX_SAMPLE (include/ccx.h) around ccx_softmax.h's sample_slot: which (env, agent) a lane's
// slot is, what it reads besides its five logits, which key it draws with, and what a dead slot gets.  Shared by
// ccx_sample.hip (logits from memory) and the fused kernel of ccx_mlp.hip (logits from the tile): "mlp_sample_actions is
// sample_actions(head(obs))" holds because both run this.  Device code, and the one host function that fills DrawArgs.
//
// One lane owns one slot of the flat [E N] index; workgroup b's FIRST wave takes slots 64 b .. 64 b + 63.  Nothing is per
// env except the two counters of the key (step_count, episode), read once per lane at e = slot / N.
#pragma once
#include "ccx_internal.h"
#include "ccx_softmax.h"

namespace ccx_draw {

struct DrawArgs {
    const uint8_t* masks;              // may be null (everything legal)
    const uint8_t* terminated;
    const uint8_t* truncated;
    const int32_t* step_count;
    const int32_t* episode;
    uint8_t* actions;
    float* logp;                       // STATS: either may be null
    float* entropy;
    long long EN;
    int32_t E;
    uint32_t N, genv0, seed_lo, seed_hi;   // genv0: low word of env_offset; seed_hi already carries kSampleStream
};

inline DrawArgs draw_args(const ccx_handle* h, const uint8_t* masks_or_null, uint8_t* actions, float* logp_or_null,
                          float* entropy_or_null) {
    DrawArgs D;
    D.masks = masks_or_null;
    D.terminated = h->st.terminated;
    D.truncated = h->st.truncated;
    D.step_count = h->st.step_count;
    D.episode = h->st.episode;
    D.actions = actions;
    D.logp = logp_or_null;
    D.entropy = entropy_or_null;
    D.EN = (long long)h->E * h->N;
    D.E = h->E;
    D.N = (uint32_t)h->N;
    D.genv0 = (uint32_t)h->env_offset;
    D.seed_lo = h->rng_lo;
    D.seed_hi = h->rng_hi ^ ccx::kSampleStream;
    return D;
}

struct Slot {
    long long slot, e;                 // slot may lie behind the last one (the tail wave's surplus lanes); e = slot / N
    uint32_t a;                        // slot % N
};

// e = slot / N without a 64-bit division: the workgroup index splits as q N + r (one u32 division, wave-uniform), so
// 64 b = 64 q N + 64 r, and the rest, 64 r + lane < 64 N + 64 <= 4160, is a second u32 division
__device__ __forceinline__ Slot slot_of(const DrawArgs& D, uint32_t lane) {
    const uint32_t bq = blockIdx.x / D.N, br = blockIdx.x - bq * D.N;
    const uint32_t rest = br * 64u + lane, rq = rest / D.N;
    return Slot{(long long)blockIdx.x * 64 + lane, (long long)bq * 64 + rq, rest - rq * D.N};
}

struct Small {
    uint8_t term = 0, trunc = 0;
    uint32_t mbyte = 0x1Fu, episode = 0, step = 0;
};

// What a slot reads besides its logits.  Every load is unconditional, at a clamped index (the tail wave's surplus lanes load
// what the last slot loads), so all of them can be issued before the first wait; the key's counters are read only where a
// draw follows.
template <bool DET>
__device__ __forceinline__ Small small_loads(const DrawArgs& D, const Slot& s, bool masked) {
    const long long sl = s.slot < D.EN ? s.slot : D.EN - 1;
    Small v;
    v.term = D.terminated[sl];
    v.trunc = D.truncated[sl];
    if (masked) v.mbyte = (uint32_t)D.masks[sl];
    if (!DET) {
        const long long el = s.e < D.E ? s.e : D.E - 1;
        v.episode = (uint32_t)D.episode[el];
        v.step = (uint32_t)D.step_count[el];
    }
    return v;
}

// From the five logits of a slot < EN to its three stores.  A dead slot (terminated or truncated) gets action 255 and
// logp = entropy = +0, SELECTED: whatever its logits hold never reaches a result.
template <bool DET, bool STATS>
__device__ __forceinline__ void finish(const DrawArgs& D, const Slot& s, const Small& v, float (&l)[5]) {
    const bool dead = (v.term | v.trunc) != 0;
    const uint32_t m = (v.mbyte & 0x1Fu) | 0x10u;
    uint32_t u = 0;
    if (!DET) u = ccx::random_word(D.seed_lo, D.seed_hi, D.genv0 + (uint32_t)s.e, v.episode, v.step, s.a);
    uint32_t action;
    float logp = 0.0f, entropy = 0.0f;
    ccx_softmax::sample_slot<DET, STATS>(l, m, u, STATS && D.logp != nullptr, STATS && D.entropy != nullptr, action, logp, entropy);
    D.actions[s.slot] = dead ? (uint8_t)CCX_ACTION_ABSENT : (uint8_t)action;
    if (STATS) {
        if (D.logp) D.logp[s.slot] = dead ? 0.0f : logp;
        if (D.entropy) D.entropy[s.slot] = dead ? 0.0f : entropy;
    }
}

}  // namespace ccx_draw
