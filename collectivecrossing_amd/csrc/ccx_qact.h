// ccx_qact.h -- steps 1-6 of ccx_q_actions (include/ccx.h CCX_QLEARN) for one slot, from its five Q-values to its two stores,
// and the DrawArgs of such a launch.  Shared by q_act_kernel (ccx_qlearn.hip: Q-values from memory) and the fused actor
// kernels obs_q_kernel (ccx_dueling.hip) and obs_q_groups_kernel (ccx_sides.hip: Q-values from the tile, through the dueling
// combine where the head has six outputs): "ccx_mlp_q_actions is ccx_q_actions(head(obs))" holds because all three run this.  Device
// code, and the one host function that fills DrawArgs.
#pragma once
#include "ccx_draw.h"
#include "ccx_dueling.h"
#include "ccx_qlearn.h"

namespace ccx_qact {

// ccx_draw.h's arguments with the seed as it is: choose() adds its two streams itself
inline ccx_draw::DrawArgs draw_args(const ccx_handle* h, const uint8_t* masks_or_null, uint8_t* actions) {
    ccx_draw::DrawArgs D = ccx_draw::draw_args(h, masks_or_null, actions, nullptr, nullptr);
    D.seed_hi = h->rng_hi;
    return D;
}

// From the five Q-values of a slot < EN to its stores.  v: small_loads<!EPS>; eps: epsilon[0] (read only where EPS).
template <bool EPS>
__device__ __forceinline__ void choose(const ccx_draw::DrawArgs& D, const ccx_draw::Slot& s, const ccx_draw::Small& v,
                                       const float (&l)[5], float eps, uint8_t* explored) {
    const bool dead = (v.term | v.trunc) != 0;
    const uint32_t m = ccx_qlearn::legal_set(v.mbyte);
    uint32_t action = ccx_qlearn::greedy(l, m);
    bool explore = false;
    if (EPS) {
        const uint32_t g = D.genv0 + (uint32_t)s.e;
        const uint32_t u1 = ccx::random_word(D.seed_lo, D.seed_hi ^ ccx::kQExploreStream, g, v.episode, v.step, s.a);
        const uint32_t u2 = ccx::random_word(D.seed_lo, D.seed_hi ^ ccx::kQChoiceStream, g, v.episode, v.step, s.a);
        explore = ccx_qlearn::explores(u1, eps);
        const uint32_t ch = ccx_qlearn::choice(u2, m);
        action = explore ? ch : action;
    }
    D.actions[s.slot] = dead ? (uint8_t)CCX_ACTION_ABSENT : (uint8_t)action;
    if (explored) explored[s.slot] = (!dead && explore) ? (uint8_t)1 : (uint8_t)0;
}

// The fused kernels' tail for wave 0's lane: its row of the tile's y (O = DUEL ? 6 : 5 floats at y + O lane, in LDS), the
// dueling combine where DUEL, then choose().  With DUEL the combined row goes to q_row (the slot's five floats, or null)
// from here; without it the tile has stored y itself.
template <bool EPS, bool DUEL>
__device__ __forceinline__ void from_tile(const ccx_draw::DrawArgs& D, const ccx_draw::Slot& s, const ccx_draw::Small& v,
                                          const float* y, uint32_t lane, float eps, uint8_t* explored, float* q_row) {
    float l[5];
    if (DUEL) {
        float va[6];
#pragma unroll
        for (int k = 0; k < 6; ++k) va[k] = y[6 * lane + k];
        ccx_dueling::forward(va, l);
        if (q_row) {
#pragma unroll
            for (int k = 0; k < 5; ++k) q_row[k] = l[k];
        }
    } else {
#pragma unroll
        for (int k = 0; k < 5; ++k) l[k] = y[5 * lane + k];
    }
    choose<EPS>(D, s, v, l, eps, explored);
}

}  // namespace ccx_qact
