// The rules of csrc/ccx_qlearn.h compiled for the host (tests/test_qlearn_host_rule.py: -O2 -ffp-contract=off), behind a C
// interface for ctypes.  The loops here only walk slots and rows in the order the header states; every
// arithmetic operation is one of ccx_qlearn.h's or ccx_tree.h's, and the word is ccx_kernels.h's formula restated in four lines
// (that header needs the HIP runtime).
#include <vector>

#include "ccx_qlearn.h"

namespace {

constexpr uint32_t kQExploreStream = 0x68E31DA4u, kQChoiceStream = 0xB5297A4Du;

uint32_t mix32(uint32_t k) {
    k ^= k >> 16; k *= 0x7FEB352Du; k ^= k >> 15; k *= 0x846CA68Bu; k ^= k >> 16;
    return k;
}
uint32_t random_word(uint32_t seed_lo, uint32_t seed_hi, uint32_t genv, uint32_t episode, uint32_t step, uint32_t agent) {
    const uint32_t k = genv * 0x9E3779B1u + episode * 0x85EBCA77u + step * 0xC2B2AE3Du + agent * 0x27D4EB2Fu + seed_lo;
    return mix32(mix32(k) ^ seed_hi);
}

struct RowIn {
    float q[5], qt[5], qo[5];
};

void load(RowIn& r, long long i, const float* q, const float* qt, const float* qo) {
    for (int k = 0; k < 5; ++k) {
        r.q[k] = q[i * 5 + k];
        r.qt[k] = qt[i * 5 + k];
        r.qo[k] = qo ? qo[i * 5 + k] : 0.0f;
    }
}

void forward(const RowIn& r, bool dbl, uint32_t a, double reward, bool done, uint32_t mbyte, float gamma, float delta, float c,
             bool has_w, float w, ccx_qlearn::Row& t) {
    if (dbl) ccx_qlearn::forward_row(r.q, a, (float)reward, done, r.qt, r.qo, mbyte, gamma, delta, c, has_w, w, t);
    else ccx_qlearn::forward_row(r.q, a, (float)reward, done, r.qt, r.qt, mbyte, gamma, delta, c, has_w, w, t);
}

}  // namespace

extern "C" {

void host_q_actions(long long E, int N, const float* q, const unsigned char* masks_or_null, const unsigned char* terminated,
                    const unsigned char* truncated, const int* step_count, const int* episode, unsigned long long env_offset,
                    unsigned long long seed, const float* epsilon_or_null, unsigned char* actions, unsigned char* explored_or_null) {
    const uint32_t lo = (uint32_t)seed, hi = (uint32_t)(seed >> 32);
    for (long long e = 0; e < E; ++e)
        for (int a = 0; a < N; ++a) {
            const long long s = e * N + a;
            const bool dead = (terminated[s] | truncated[s]) != 0;
            float l[5];
            for (int k = 0; k < 5; ++k) l[k] = q[s * 5 + k];
            const uint32_t m = ccx_qlearn::legal_set(masks_or_null ? masks_or_null[s] : ccx_qlearn::kLegalAll);
            uint32_t action = ccx_qlearn::greedy(l, m);
            bool explore = false;
            if (epsilon_or_null) {
                const uint32_t g = (uint32_t)env_offset + (uint32_t)e;
                const uint32_t u1 = random_word(lo, hi ^ kQExploreStream, g, (uint32_t)episode[e], (uint32_t)step_count[e], (uint32_t)a);
                const uint32_t u2 = random_word(lo, hi ^ kQChoiceStream, g, (uint32_t)episode[e], (uint32_t)step_count[e], (uint32_t)a);
                explore = ccx_qlearn::explores(u1, epsilon_or_null[0]);
                const uint32_t ch = ccx_qlearn::choice(u2, m);
                action = explore ? ch : action;
            }
            actions[s] = dead ? 255 : (unsigned char)action;
            if (explored_or_null) explored_or_null[s] = (!dead && explore) ? 1 : 0;
        }
}

void host_td_loss(long long M, const float* q, const unsigned char* actions, const double* reward, const unsigned char* done,
                  const float* qt, const float* qo_or_null, const unsigned char* masks_or_null, const unsigned char* valid_or_null,
                  const float* weights_or_null, float gamma, float delta, float* stats, float* td_error_or_null) {
    const float c = 0.5f * delta;
    std::vector<double> terms[ccx_qlearn::kSums];
    for (auto& t : terms) t.assign(M, 0.0);
    for (long long i = 0; i < M; ++i) {
        const uint32_t a = actions[i], vb = valid_or_null ? valid_or_null[i] : 1u;
        const bool counts = ccx_qlearn::row_counts(valid_or_null != nullptr, vb, a);
        if (ccx_qlearn::row_bad(valid_or_null != nullptr, vb, a)) terms[5][i] = 1.0;
        RowIn r;
        load(r, i, q, qt, qo_or_null);
        ccx_qlearn::Row t;
        forward(r, qo_or_null != nullptr, a, reward[i], done[i] != 0, masks_or_null ? masks_or_null[i] : ccx_qlearn::kLegalAll, gamma,
                delta, c, weights_or_null != nullptr, weights_or_null ? weights_or_null[i] : 1.0f, t);
        if (td_error_or_null) td_error_or_null[i] = counts ? t.d : 0.0f;
        if (!counts) continue;
        const double v[5] = {1.0, (double)t.term, (double)t.ad, (double)t.qa, (double)t.y};
        for (int k = 0; k < 5; ++k) terms[k][i] = v[k];
    }
    double S[ccx_qlearn::kSums];
    for (int k = 0; k < ccx_qlearn::kSums; ++k) S[k] = ccx_tree::sum_host(terms[k].data(), M);
    float st[8];
    ccx_qlearn::td_finals(S, st);
    for (int k = 0; k < 8; ++k) stats[k] = st[k];
}

void host_td_loss_backward(long long M, const float* q, const unsigned char* actions, const double* reward, const unsigned char* done,
                           const float* qt, const float* qo_or_null, const unsigned char* masks_or_null,
                           const unsigned char* valid_or_null, const float* weights_or_null, float gamma, float delta,
                           const float* stats, const float* grad_loss_or_null, float* grad_q) {
    const float c = 0.5f * delta;
    const float n = stats[6];
    const float g = grad_loss_or_null ? grad_loss_or_null[0] : 1.0f;
    const float sc = g / n;
    for (long long i = 0; i < M; ++i) {
        const uint32_t a = actions[i], vb = valid_or_null ? valid_or_null[i] : 1u;
        const bool counts = n != 0.0f && ccx_qlearn::row_counts(valid_or_null != nullptr, vb, a);
        const bool has_w = weights_or_null != nullptr;
        const float w = has_w ? weights_or_null[i] : 1.0f;
        const float gw = ccx_qlearn::row_scale(has_w, sc, w);
        RowIn r;
        load(r, i, q, qt, qo_or_null);
        ccx_qlearn::Row t;
        forward(r, qo_or_null != nullptr, a, reward[i], done[i] != 0, masks_or_null ? masks_or_null[i] : ccx_qlearn::kLegalAll, gamma,
                delta, c, has_w, w, t);
        const float ga = ccx_qlearn::backward_row(t.d, t.ad, delta, gw);
        for (int k = 0; k < 5; ++k) grad_q[i * 5 + k] = (counts && a == (uint32_t)k) ? ga : 0.0f;
    }
}

}  // extern "C"
