// ccx_softmax.h -- the masked five-way distribution of CCX_SAMPLE / CCX_EVALUATE (include/ccx.h) as inline functions of one
// row: exp_spec, log_spec, steps 2-6 of CCX_SAMPLE (legal set, maximum, degenerate, d, w, c, S), its entropy (step 10), the rule
// of one live slot (sample_slot, steps 2-10: shared by ccx_sample.hip and the fused kernel of ccx_mlp.hip), and
// the per-row forward and backward rules of CCX_EVALUATE.  Included by ccx_sample.hip, ccx_evaluate.hip and ccx_ppo.h; it also compiles
// with a plain host C++ compiler (tests/test_evaluate_host_rule.py runs it against the NumPy specs bit for bit).
// Every line is ONE f32 operation: the units that include this are compiled with -ffp-contract=off, and `/` must be the
// correctly rounded division.  What a rule does not read is SELECTED away before any arithmetic, never multiplied by zero.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define CCX_HD __host__ __device__ __forceinline__
#else
#define CCX_HD inline
#endif

namespace ccx_softmax {

constexpr float kLog2e = 0x1.715476p+0f, kLn2Hi = 0x1.62e4p-1f, kLn2Lo = 0x1.7f7d1cp-20f, kSqrtHalf = 0x1.6a09e6p-1f;
constexpr float kDMin = -80.0f;
constexpr uint32_t kActionAbsent = 255u;                                  // CCX_ACTION_ABSENT

// x in [-80, 80] (CCX_SAMPLE / CCX_EVALUATE use [-80, 0], CCX_PPO_LOSS the whole of it)
CCX_HD float exp_spec(float x) {
    const float n = rintf(x * kLog2e);
    const float r = (x - n * kLn2Hi) - n * kLn2Lo;
    float p = 0x1.a01a02p-13f;
    p = p * r + 0x1.6c16c2p-10f;
    p = p * r + 0x1.111112p-7f;
    p = p * r + 0x1.555556p-5f;
    p = p * r + 0x1.555556p-3f;
    p = p * r + 0x1p-1f;
    p = p * r + 1.0f;
    p = p * r + 1.0f;
    return p * __builtin_bit_cast(float, ((int)n + 127) << 23);           // exact: |n| <= 116, the product is a normal number
}

// s in [1, 64] (CCX_SAMPLE / CCX_EVALUATE use [1, 5], CCX_C51 the whole of it: within 2.6e-7 absolute of f64 log over
// [1, 64], measured on the CPU over 2e6 points)
CCX_HD float log_spec(float s) {
    const int bits = __builtin_bit_cast(int, s);
    float m = __builtin_bit_cast(float, (bits & 0x007FFFFF) | 0x3F000000);  // s = m * 2^e, m in [0.5, 1)
    int e = (bits >> 23) - 126;
    const bool small = m < kSqrtHalf;
    m = small ? m + m : m;
    e = small ? e - 1 : e;
    const float ef = (float)e;
    const float t = m - 1.0f;
    const float q = t / (2.0f + t);
    const float z = q * q;
    float p = 0x1.c71c72p-4f;
    p = p * z + 0x1.24924ap-3f;
    p = p * z + 0x1.99999ap-3f;
    p = p * z + 0x1.555556p-2f;
    const float u = q + q;
    const float lf = u + u * (z * p);
    return ef * kLn2Hi + (lf + ef * kLn2Lo);
}

// Steps 2-4 of CCX_SAMPLE and the differences of step 5, from a row's five logits and its legal set m (bit 4 set).  Illegal
// logits are replaced by -inf in l; d is +0.0 at illegal k and in a degenerate row.
CCX_HD void legal_max_d(float (&l)[5], uint32_t m, bool (&legal)[5], float& mx, bool& degenerate, float (&d)[5]) {
    const float ninf = -__builtin_inff();
    mx = ninf;
    bool bad = false;
#pragma unroll
    for (int k = 0; k < 5; ++k) {
        legal[k] = (m >> k) & 1u;
        l[k] = legal[k] ? l[k] : ninf;                                  // illegal logits leave here
        mx = l[k] > mx ? l[k] : mx;
        bad = bad || l[k] != l[k] || l[k] == __builtin_inff();
    }
    degenerate = bad || mx == ninf;
#pragma unroll
    for (int k = 0; k < 5; ++k) d[k] = (legal[k] && !degenerate) ? l[k] - mx : 0.0f;
}

// Steps 5-6: the weights and their prefix sums; returns S = c[4], 1 <= S <= 5.
CCX_HD float weights(const bool (&legal)[5], const float (&d)[5], float (&w)[5], float (&c)[5]) {
#pragma unroll
    for (int k = 0; k < 5; ++k) {
        const bool cut = d[k] < kDMin;
        w[k] = (legal[k] && !cut) ? exp_spec(cut ? 0.0f : d[k]) : 0.0f;
        c[k] = k ? c[k - 1] + w[k] : w[0];
    }
    return c[4];
}

// Step 10, ls = log_spec(S).
CCX_HD float entropy_spec(const float (&w)[5], const float (&d)[5], float S, float ls) {
    float T = 0.0f;
#pragma unroll
    for (int k = 0; k < 5; ++k) {
        const float term = w[k] == 0.0f ? 0.0f : w[k] * d[k];
        T = k ? T + term : term;
    }
    return ls - T / S;
}

// The rule of one live slot (steps 2-10 of the header paragraph) from its five logits, its legal set m and its draw u.
// Shared by ccx_sample.hip and the fused kernel of ccx_mlp.hip.
template <bool DET, bool STATS>
CCX_HD void sample_slot(float (&l)[5], uint32_t m, uint32_t u, bool want_logp, bool want_entropy,
                        uint32_t& action, float& logp, float& entropy) {
    bool legal[5], degenerate;
    float mx, d[5];
    legal_max_d(l, m, legal, mx, degenerate, d);
    action = 4u;
    float S = 1.0f, w[5];
    if (DET) {
#pragma unroll
        for (int k = 4; k >= 0; --k) action = (legal[k] && (degenerate || l[k] == mx)) ? (uint32_t)k : action;
    }
    if (!DET || STATS) {
        float c[5];
        S = weights(legal, d, w, c);
        if (!DET) {
            const float thr = ((float)(u >> 8) * 0x1p-24f) * S;
#pragma unroll
            for (int k = 4; k >= 0; --k) action = (legal[k] && c[k] > thr) ? (uint32_t)k : action;
        }
    }
    if (STATS) {
        const float ls = log_spec(S);
        if (want_logp) {
            float da = d[4];
#pragma unroll
            for (int k = 3; k >= 0; --k) da = action == (uint32_t)k ? d[k] : da;
            logp = da - ls;
        }
        if (want_entropy) {
            entropy = entropy_spec(w, d, S, ls);
        }
    }
}

// CCX_EVALUATE, forward, one row: its five logits (changed: illegal ones become -inf), its mask byte and its stored action.
template <bool ENT>
CCX_HD void evaluate_row(float (&l)[5], uint32_t mbyte, uint32_t a, float& logp, float& entropy) {
    const uint32_t m = (mbyte & 0x1Fu) | 0x10u;
    bool legal[5], degenerate;
    float mx, d[5], w[5], c[5];
    legal_max_d(l, m, legal, mx, degenerate, d);
    const float S = weights(legal, d, w, c);
    const float ls = log_spec(S);
    const bool absent = a == kActionAbsent;
    bool a_legal = false;
    float da = 0.0f;
#pragma unroll
    for (int k = 0; k < 5; ++k) {
        const bool hit = a == (uint32_t)k;
        a_legal = hit ? legal[k] : a_legal;
        da = hit ? d[k] : da;
    }
    const float lp = a_legal ? da - ls : -__builtin_inff();
    logp = absent ? 0.0f : lp;
    if (ENT) {
        const float H = entropy_spec(w, d, S, ls);
        entropy = absent ? 0.0f : H;
    }
}

// CCX_EVALUATE, backward, one row: the forward quantities recomputed from the logits, then the gradient with respect to
// the five logits.  glp / gent are read only where GLP / GENT.
template <bool GLP, bool GENT>
CCX_HD void evaluate_row_backward(float (&l)[5], uint32_t mbyte, uint32_t a, float glp, float gent, float (&grad)[5]) {
    const uint32_t m = (mbyte & 0x1Fu) | 0x10u;
    bool legal[5], degenerate;
    float mx, d[5], w[5], c[5];
    legal_max_d(l, m, legal, mx, degenerate, d);
    const float S = weights(legal, d, w, c);
    const float ls = log_spec(S);
    const bool none = a == kActionAbsent || degenerate;
    bool a_legal = false;
#pragma unroll
    for (int k = 0; k < 5; ++k) a_legal = a == (uint32_t)k ? legal[k] : a_legal;
    float H = 0.0f;
    if (GENT) H = entropy_spec(w, d, S, ls);
#pragma unroll
    for (int k = 0; k < 5; ++k) {
        const float p = w[k] / S;
        float A = 0.0f, B = 0.0f, g;
        if (GLP) {
            const float t1 = (a == (uint32_t)k ? 1.0f : 0.0f) - p;
            const float prod = glp * t1;
            A = a_legal ? prod : 0.0f;
        }
        if (GENT) {
            const float lpk = d[k] - ls;
            const float inner = p * (lpk + H);
            const float t2 = w[k] == 0.0f ? 0.0f : inner;
            B = gent * t2;
        }
        if (GLP && GENT) g = A - B;
        else if (GLP) g = A;
        else g = 0.0f - B;
        grad[k] = (legal[k] && !none) ? g : 0.0f;
    }
}

}  // namespace ccx_softmax
