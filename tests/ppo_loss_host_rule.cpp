// The per-row rule and the final values of csrc/ccx_ppo.h and the tree of csrc/ccx_tree.h compiled for the host
// (tests/test_ppo_loss_host_rule.py: -O2 -ffp-contract=off), behind a C interface for ctypes.  The loops here only walk rows;
// every arithmetic operation is one of the two headers'.
#include <vector>

#include "ccx_ppo.h"

namespace {

struct Norm {
    bool has;
    float mean, denom;
};

Norm norm_of(const float* norm_or_null, float adv_eps) {
    Norm n{norm_or_null != nullptr, 0.0f, 1.0f};
    if (n.has) {
        n.mean = norm_or_null[0];
        n.denom = norm_or_null[1] + adv_eps;
    }
    return n;
}

}  // namespace

extern "C" {

void host_ppo_loss(long long M, const float* logits, const unsigned char* actions, const unsigned char* masks_or_null,
                   const float* logp_old, const float* advantages, const float* returns, const float* values,
                   const unsigned char* valid_or_null, const float* norm_or_null, float clip, float vf_coef, float ent_coef,
                   float adv_eps, float* stats) {
    const float lo = 1.0f - clip, hi = 1.0f + clip;
    const Norm nm = norm_of(norm_or_null, adv_eps);
    std::vector<double> terms[ccx_ppo::kSums];
    for (auto& t : terms) t.assign(M, 0.0);
    for (long long i = 0; i < M; ++i) {
        if (!ccx_ppo::row_counts(valid_or_null != nullptr, valid_or_null ? valid_or_null[i] : 1u, actions[i])) continue;
        float l[5];
        for (int k = 0; k < 5; ++k) l[k] = logits[i * 5 + k];
        const float an = ccx_ppo::normalised(nm.has, advantages[i], nm.mean, nm.denom);
        ccx_ppo::Row t;
        ccx_ppo::forward_row(l, masks_or_null ? masks_or_null[i] : 0x1Fu, actions[i], logp_old[i], an, returns[i], values[i], lo, hi, t);
        const double v[ccx_ppo::kSums] = {1.0, (double)t.surr, (double)t.vl, (double)t.H, (double)t.kl, (double)t.cf};
        for (int q = 0; q < ccx_ppo::kSums; ++q) terms[q][i] = v[q];
    }
    double S[ccx_ppo::kSums];
    for (int q = 0; q < ccx_ppo::kSums; ++q) S[q] = ccx_tree::sum_host(terms[q].data(), M);
    float st[8];
    ccx_ppo::loss_finals(S, vf_coef, ent_coef, st);
    for (int k = 0; k < 8; ++k) stats[k] = st[k];
}

void host_ppo_loss_backward(long long M, const float* logits, const unsigned char* actions, const unsigned char* masks_or_null,
                            const float* logp_old, const float* advantages, const float* returns, const float* values,
                            const unsigned char* valid_or_null, const float* norm_or_null, float clip, float vf_coef,
                            float ent_coef, float adv_eps, const float* stats, const float* grad_loss_or_null,
                            float* grad_logits_or_null, float* grad_values_or_null) {
    const float lo = 1.0f - clip, hi = 1.0f + clip;
    const Norm nm = norm_of(norm_or_null, adv_eps);
    const float n = stats[6];
    const float g = grad_loss_or_null ? grad_loss_or_null[0] : 1.0f;
    const float sc = g / n;
    const float se = sc * ent_coef;
    const float gent = 0.0f - se;
    const float scv = sc * vf_coef;
    for (long long i = 0; i < M; ++i) {
        const bool counts = n != 0.0f && ccx_ppo::row_counts(valid_or_null != nullptr, valid_or_null ? valid_or_null[i] : 1u, actions[i]);
        if (grad_logits_or_null) {
            float l[5], gr[5];
            for (int k = 0; k < 5; ++k) l[k] = logits[i * 5 + k];
            const float an = ccx_ppo::normalised(nm.has, advantages[i], nm.mean, nm.denom);
            ccx_ppo::backward_row_logits(l, masks_or_null ? masks_or_null[i] : 0x1Fu, actions[i], logp_old[i], an, returns[i],
                                         values[i], lo, hi, sc, gent, gr);
            for (int k = 0; k < 5; ++k) grad_logits_or_null[i * 5 + k] = counts ? gr[k] : 0.0f;
        }
        if (grad_values_or_null) {
            const float gv = ccx_ppo::backward_row_value(returns[i], values[i], scv);
            grad_values_or_null[i] = counts ? gv : 0.0f;
        }
    }
}

void host_masked_moments(long long M, const float* x, const unsigned char* valid_or_null, float* out) {
    std::vector<double> terms[ccx_ppo::kMomentSums];
    for (auto& t : terms) t.assign(M, 0.0);
    for (long long i = 0; i < M; ++i) {
        if (valid_or_null && valid_or_null[i] == 0) continue;
        const double xd = (double)x[i];
        terms[0][i] = 1.0;
        terms[1][i] = xd;
        terms[2][i] = xd * xd;
    }
    double S[ccx_ppo::kMomentSums];
    for (int q = 0; q < ccx_ppo::kMomentSums; ++q) S[q] = ccx_tree::sum_host(terms[q].data(), M);
    float o[4];
    ccx_ppo::moments_finals(S, o);
    for (int k = 0; k < 4; ++k) out[k] = o[k];
}

double host_tree(long long M, const double* terms) { return ccx_tree::sum_host(terms, M); }

float host_exp_spec(float x) { return ccx_softmax::exp_spec(x); }

}  // extern "C"
