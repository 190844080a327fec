// ccx_qlearn.h -- CCX_QLEARN (include/ccx.h) as inline functions: the greedy action over a legal set (ONE function, shared by
// the actor's epsilon-greedy choice and the bootstrap action of the TD target), the exploration draw and the uniform choice
// over the legal set, the per-row TD terms (taken Q-value, target, Huber), the per-row gradient, and the final values.  The
// reduction tree is ccx_tree.h's, called, not restated.  Included by ccx_qlearn.hip; it also compiles with a plain host C++
// compiler (tests/test_qlearn_host_rule.py runs it against the NumPy spec bit for bit).
// The discipline is ccx_softmax.h's: every line is ONE operation of the stated type, the including units are compiled with
// -ffp-contract=off, `/` is the correctly rounded division, and what a rule does not read is SELECTED away before any
// arithmetic, never multiplied by zero.
#pragma once
#include "ccx_softmax.h"
#include "ccx_tree.h"

namespace ccx_qlearn {

constexpr int kSums = 6;                                                  // count, term, |d|, qa, y, bad
constexpr uint32_t kLegalAll = 0x1Fu;

// step 2 of CCX_SAMPLE: bit k set = action k is legal; wait always is
CCX_HD uint32_t legal_set(uint32_t mbyte) { return (mbyte & 0x1Fu) | 0x10u; }

// THE greedy action: the lowest legal k to start with, then for legal k ascending a strictly greater value takes over.  A
// NaN never wins (the comparison is false), a row of NaNs gives the lowest legal k, ties go to the lowest index.  A value at
// an illegal k is compared but the outcome is selected away.
CCX_HD uint32_t greedy(const float (&q)[5], uint32_t m) {
    uint32_t kg = 4u;
#pragma unroll
    for (int k = 3; k >= 0; --k) kg = ((m >> k) & 1u) ? (uint32_t)k : kg;   // the lowest legal k
    float mx = -__builtin_inff();
#pragma unroll
    for (int k = 0; k < 5; ++k) {
        const float v = q[k];                                             // (read unconditionally: the row stays in registers)
        const bool legal = ((m >> k) & 1u) != 0u, above = v > mx;
        const bool win = legal & above;
        mx = win ? v : mx;
        kg = win ? (uint32_t)k : kg;
    }
    return kg;
}

// r = (float)(u >> 8) * 2^-24 (exact, in [0, 1)); explore iff r < eps: a NaN eps never explores, eps >= 1 always does
CCX_HD bool explores(uint32_t u1, float eps) {
    const float r = (float)(u1 >> 8) * 0x1p-24f;
    return r < eps;
}

// the idx-th legal k ascending, idx = u2 * popcount(m) >> 32
CCX_HD uint32_t choice(uint32_t u2, uint32_t m) {
    const uint32_t n = (uint32_t)__builtin_popcount(m);
    const uint32_t idx = (uint32_t)(((unsigned long long)u2 * n) >> 32);
#pragma unroll
    for (uint32_t j = 0; j < 4u; ++j) m = j < idx ? (m & (m - 1u)) : m;    // drop the idx lowest legal actions
    return (uint32_t)__builtin_ctz(m);
}

// a row counts iff its valid byte is not zero and its action is one of 0..4 (255 = absent; 5..254 = bad, tallied)
CCX_HD bool row_counts(bool has_valid, uint32_t vbyte, uint32_t a) { return (!has_valid || vbyte != 0u) && a <= 4u; }
CCX_HD bool row_bad(bool has_valid, uint32_t vbyte, uint32_t a) {
    return (!has_valid || vbyte != 0u) && a > 4u && a != ccx_softmax::kActionAbsent;
}

// v[k], selected (k > 4 gives v[4]: such a row does not count)
CCX_HD float pick(const float (&v)[5], uint32_t k) {
    const float v0 = v[0], v1 = v[1], v2 = v[2], v3 = v[3], v4 = v[4];    // (read unconditionally, then selected by value)
    float x = k == 3u ? v3 : v4;
    x = k == 2u ? v2 : x;
    x = k == 1u ? v1 : x;
    x = k == 0u ? v0 : x;
    return x;
}

struct Row {
    float qa, boot, y, d, ad, h, term;
    uint32_t kstar;
};

// Steps 2-5 for one row.  q: the row's Q-values; qt: the target network's at the next state; qsel: what chooses the
// bootstrap action (the online network's at the next state for double-Q, else qt); c = 0.5f * delta, made once per call.
CCX_HD void forward_row(const float (&q)[5], uint32_t a, float r, bool done, const float (&qt)[5], const float (&qsel)[5],
                        uint32_t mbyte_next, float gamma, float delta, float c, bool has_w, float w, Row& t) {
    t.qa = pick(q, a);
    t.kstar = greedy(qsel, legal_set(mbyte_next));
    t.boot = pick(qt, t.kstar);
    const float gb = gamma * t.boot;
    const float nb = (done || gamma == 0.0f) ? 0.0f : gb;               // selected: a NaN in a terminal row's next-Q stays there
    t.y = r + nb;
    t.d = t.qa - t.y;
    t.ad = __builtin_fabsf(t.d);
    const float sq = t.d * t.d;
    const float h1 = 0.5f * sq;
    const float lin = t.ad - c;
    const float h2 = delta * lin;
    t.h = t.ad <= delta ? h1 : h2;
    const float wh = w * t.h;
    t.term = has_w ? wh : t.h;
}

// gw = weights ? sc * w_i : sc, with sc = g / stats[6] made once per call
CCX_HD float row_scale(bool has_w, float sc, float w) {
    const float sw = sc * w;
    return has_w ? sw : sc;
}

// the gradient of the loss at the row's taken Q-value
CCX_HD float backward_row(float d, float ad, float delta, float gw) {
    const bool isnan = d != d;
    const float nd = 0.0f - delta;                                        // (a sign flip: exact)
    const float lim = d < 0.0f ? nd : delta;
    const float dd = (ad <= delta || isnan) ? d : lim;                  // a NaN goes through loudly
    return gw * dd;
}

// S = the six sums (count, term, |d|, qa, y, bad); all arithmetic f64, each output rounded to f32 once
CCX_HD void td_finals(const double (&S)[kSums], float (&stats)[8]) {
    const double n = S[0];
    const double loss = S[1] / n;
    const double mad = S[2] / n;
    const double mq = S[3] / n;
    const double my = S[4] / n;
    const bool none = n == 0.0;
    stats[0] = none ? 0.0f : (float)loss;
    stats[1] = none ? 0.0f : (float)mad;
    stats[2] = none ? 0.0f : (float)mq;
    stats[3] = none ? 0.0f : (float)my;
    stats[4] = 0.0f;
    stats[5] = 0.0f;
    stats[6] = (float)n;
    stats[7] = (float)S[5];
}

}  // namespace ccx_qlearn
