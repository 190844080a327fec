// ccx_ppo.h -- CCX_PPO_LOSS (include/ccx.h) as inline functions: which rows count, the per-row forward terms and gradients
// (built on ccx_softmax.h's evaluate_row / evaluate_row_backward, which are called, not restated), and the final values of
// the loss and of the masked moments.  The sums between the two go through ccx_tree.h's fixed f64 reduction tree.  Included
// by ccx_ppo_loss.hip; it also compiles with a plain host C++ compiler (tests/test_ppo_loss_host_rule.py runs it against the
// NumPy spec bit for bit).
// The discipline is ccx_softmax.h's: every line is ONE operation of the stated type, the including units are compiled with
// -ffp-contract=off, `/` and sqrt are the correctly rounded ones, and what a rule does not read is SELECTED away before any
// arithmetic, never multiplied by zero.
#pragma once
#include "ccx_softmax.h"
#include "ccx_tree.h"

namespace ccx_ppo {

constexpr float kXMax = 80.0f;                                            // |logp - logp_old| is clamped here: exp_spec's domain
constexpr int kSums = 6;                                                  // count, surr, vl, H, kl, cf
constexpr int kMomentSums = 3;                                            // count, x, x * x

CCX_HD bool row_counts(bool has_valid, uint32_t vbyte, uint32_t a) {
    return (!has_valid || vbyte != 0u) && a != ccx_softmax::kActionAbsent;
}

// step 3: the advantage as the surrogate sees it; denom = norm[1] + adv_eps (one f32 add, made once per call)
CCX_HD float normalised(bool has_norm, float adv, float mean, float denom) {
    if (!has_norm) return adv;
    const float c = adv - mean;
    return c / denom;
}

struct Row {
    float x, xc, ratio, s1, s2, surr, ve, vl, H, kl, cf;
    bool clipped;
};

// Steps 1, 2, 4, 5, 6 of the forward for a row that counts.  l: its five logits (changed: illegal ones become -inf).
CCX_HD void forward_row(float (&l)[5], uint32_t mbyte, uint32_t a, float logp_old, float an, float ret, float val, float lo,
                        float hi, Row& t) {
    float logp, H;
    ccx_softmax::evaluate_row<true>(l, mbyte, a, logp, H);
    t.H = H;
    t.x = logp - logp_old;
    t.xc = t.x < -kXMax ? -kXMax : (t.x > kXMax ? kXMax : t.x);
    const bool isnan = t.xc != t.xc;                                      // the caller's NaN: it goes through, not into exp_spec
    const float e = ccx_softmax::exp_spec(isnan ? 0.0f : t.xc);
    t.ratio = isnan ? t.xc : e;
    t.s1 = t.ratio * an;
    const float rc = t.ratio < lo ? lo : (t.ratio > hi ? hi : t.ratio);
    t.s2 = rc * an;
    t.surr = t.s2 < t.s1 ? t.s2 : t.s1;
    t.ve = val - ret;
    t.vl = t.ve * t.ve;
    const float r1 = t.ratio - 1.0f;
    t.kl = r1 - t.xc;
    t.clipped = t.ratio < lo || t.ratio > hi;
    t.cf = t.clipped ? 1.0f : 0.0f;
}

// Backward for a row that counts: steps 1-5 recomputed, then the gradient with respect to its five logits.
// sc = g / stats[6], gent = 0.0f - sc * ent_coef (both made once per call).
CCX_HD void backward_row_logits(float (&l)[5], uint32_t mbyte, uint32_t a, float logp_old, float an, float ret, float val,
                                float lo, float hi, float sc, float gent, float (&grad)[5]) {
    Row t;
    forward_row(l, mbyte, a, logp_old, an, ret, val, lo, hi, t);
    const bool pass = !t.clipped || t.s1 < t.s2;
    const float prod = sc * t.s1;
    const float glp = (pass && t.x == t.xc) ? 0.0f - prod : 0.0f;
    ccx_softmax::evaluate_row_backward<true, true>(l, mbyte, a, glp, gent, grad);
}

// scv = sc * vf_coef (made once per call)
CCX_HD float backward_row_value(float ret, float val, float scv) {
    const float ve = val - ret;
    const float two = ve + ve;
    return scv * two;
}

// ---- final values.  S = the six sums (count, surr, vl, H, kl, cf); all arithmetic f64, each output rounded to f32 once.
CCX_HD void loss_finals(const double (&S)[kSums], float vf_coef, float ent_coef, float (&stats)[8]) {
    const double n = S[0];
    const double ms = S[1] / n;
    const double policy = -ms;                                            // (a sign flip: exact)
    const double value = S[2] / n;
    const double entropy = S[3] / n;
    const double tv = (double)vf_coef * value;
    const double te = (double)ent_coef * entropy;
    const double pv = policy + tv;
    const double loss = pv - te;
    const double kl = S[4] / n;
    const double cf = S[5] / n;
    const bool none = n == 0.0;
    stats[0] = none ? 0.0f : (float)loss;
    stats[1] = none ? 0.0f : (float)policy;
    stats[2] = none ? 0.0f : (float)value;
    stats[3] = none ? 0.0f : (float)entropy;
    stats[4] = none ? 0.0f : (float)kl;
    stats[5] = none ? 0.0f : (float)cf;
    stats[6] = (float)n;
    stats[7] = 0.0f;
}

// S = (count, sum x, sum x * x); f64 throughout, sqrt the correctly rounded f64 one, mean and std rounded to f32 once each.
CCX_HD void moments_finals(const double (&S)[kMomentSums], float (&out)[4]) {
    const double n = S[0];
    const double mean = S[1] / n;
    const double sm = S[1] * mean;
    const double dev = S[2] - sm;
    const double n1 = n - 1.0;
    const double q = dev / n1;
    const double var = q < 0.0 ? 0.0 : q;
    const double sd = __builtin_sqrt(var);
    const bool few = n < 2.0;
    out[0] = (float)n;
    out[1] = few ? 0.0f : (float)mean;
    out[2] = few ? 1.0f : (float)sd;
    out[3] = 0.0f;
}

}  // namespace ccx_ppo
