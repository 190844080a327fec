// The rules of csrc/ccx_c51.h compiled for the host (tests/test_c51_host_rule.py: -O2 -ffp-contract=off), behind a C
// interface for ctypes.  The loops here only walk rows and hand the per-row terms to ccx_tree.h's sum_host; every arithmetic
// operation is one of ccx_c51.h's, ccx_qlearn.h's or ccx_tree.h's.
// With -DC51_HOST_MAIN the same source is a program of its own (built with -fsanitize=address,undefined by the test): it
// runs the three rules over heap arrays of exactly the rows' size and checks identities of the rule.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "ccx_c51.h"

extern "C" {

void host_c51_q_values(long long rows, int A, float vmin, float vmax, const float* logits, float* q) {
    const ccx_c51::Support Z = ccx_c51::support_of(A, vmin, vmax);
    for (long long i = 0; i < rows * 5; ++i) {
        ccx_c51::DistHost D;
        ccx_c51::dist_host(logits + i * A, A, D);
        q[i] = ccx_c51::expected_host(D, Z);
    }
}

void host_c51_loss(long long rows, int A, float vmin, float vmax, const float* logits, const uint8_t* actions, const double* reward,
                   const uint8_t* done, const float* next_target, const float* next_online, const uint8_t* masks_next,
                   const uint8_t* valid, const float* weights, const float* discount, float gamma, float* stats, float* row_loss,
                   float* proj) {
    const ccx_c51::Support Z = ccx_c51::support_of(A, vmin, vmax);
    std::vector<double> terms[ccx_c51::kSums];
    for (auto& t : terms) t.assign((size_t)rows, 0.0);
    for (long long i = 0; i < rows; ++i) {
        const uint32_t a = actions[i], vbyte = valid ? valid[i] : 1u;
        const bool counts = ccx_qlearn::row_counts(valid != nullptr, vbyte, a);
        terms[5][i] = ccx_qlearn::row_bad(valid != nullptr, vbyte, a) ? 1.0 : 0.0;
        if (!counts) {                                                    // nothing of the row is read
            row_loss[i] = 0.0f;
            for (int j = 0; j < A; ++j) proj[i * A + j] = 0.0f;
            continue;
        }
        const float* nt = next_target + i * 5 * A;
        const float* nsel = next_online ? next_online + i * 5 * A : nt;
        ccx_c51::RowHost t;
        ccx_c51::forward_row_host(Z, logits + (i * 5 + a) * A, (float)reward[i], done[i] != 0, discount ? discount[i] : gamma, nt, nsel,
                                  masks_next ? (uint32_t)masks_next[i] : ccx_qlearn::kLegalAll, weights != nullptr,
                                  weights ? weights[i] : 1.0f, proj + i * A, t);
        row_loss[i] = t.ce;
        terms[0][i] = 1.0;
        terms[1][i] = (double)t.term;
        terms[2][i] = (double)t.ce;
        terms[3][i] = (double)t.qa;
        terms[4][i] = (double)t.y;
    }
    double S[ccx_c51::kSums];
    for (int q = 0; q < ccx_c51::kSums; ++q) S[q] = ccx_tree::sum_host(terms[q].data(), rows);
    float st[8];
    ccx_qlearn::td_finals(S, st);
    for (int k = 0; k < 8; ++k) stats[k] = st[k];
}

void host_c51_backward(long long rows, int A, const float* logits, const uint8_t* actions, const float* proj, const uint8_t* valid,
                       const float* weights, const float* stats, const float* grad_loss, float* grad_logits) {
    const float n = stats[6];
    const float g = grad_loss ? grad_loss[0] : 1.0f;
    const float sc = g / n;
    for (long long i = 0; i < rows; ++i) {
        const uint32_t a = actions[i], vbyte = valid ? valid[i] : 1u;
        const bool counts = n != 0.0f && ccx_qlearn::row_counts(valid != nullptr, vbyte, a);
        for (int j = 0; j < 5 * A; ++j) grad_logits[i * 5 * A + j] = 0.0f;
        if (!counts) continue;
        const float gw = ccx_qlearn::row_scale(weights != nullptr, sc, weights ? weights[i] : 1.0f);
        ccx_c51::backward_row_host(A, logits + (i * 5 + a) * A, proj + i * A, gw, grad_logits + (i * 5 + a) * A);
    }
}

}  // extern "C"

#ifdef C51_HOST_MAIN
namespace {

uint32_t bits(float f) {
    uint32_t u;
    std::memcpy(&u, &f, 4);
    return u;
}

uint32_t next(uint32_t& s) {
    s ^= s << 13; s ^= s >> 17; s ^= s << 5;
    return s;
}

}  // namespace

int main() {
    uint32_t seed = 0x9E3779B9u;
    long long total = 0;
    for (int A : {2, 3, 33, 51, 64}) {
        for (long long rows : {1ll, 2ll, 63ll, 65ll, 257ll}) {
            std::vector<float> lg(rows * 5 * A), nt(rows * 5 * A), no(rows * 5 * A), q(rows * 5), row_loss(rows), proj(rows * A),
                grad(rows * 5 * A), w(rows), disc(rows);
            std::vector<uint8_t> act(rows), done(rows), masks(rows), valid(rows);
            std::vector<double> reward(rows);
            for (auto* v : {&lg, &nt, &no})
                for (auto& x : *v) x = (float)((int)(next(seed) % 2001u) - 1000) * 0.004f;
            for (long long i = 0; i < rows; ++i) {
                act[i] = (uint8_t)(next(seed) % 5u);
                done[i] = (uint8_t)(next(seed) % 5u == 0u);
                masks[i] = (uint8_t)(next(seed) & 0xFFu);
                valid[i] = 1;
                reward[i] = (double)((int)(next(seed) % 2001u) - 1000) * 0.0123;
                w[i] = 1.0f + (float)(next(seed) % 100u) * 0.01f;
                disc[i] = 0.97f;
            }
            if (rows > 2) {
                act[1] = 255;                                             // row 1 does not count and is full of NaN
                for (int j = 0; j < 5 * A; ++j) lg[5 * A + j] = nt[5 * A + j] = no[5 * A + j] = NAN;
                reward[1] = NAN;
                reward[2] = NAN;                                          // row 2 counts: its NaN reward is loud
                act[2] = 3;
            }
            float stats[8];
            host_c51_q_values(rows, A, -10.0f, 10.0f, lg.data(), q.data());
            host_c51_loss(rows, A, -10.0f, 10.0f, lg.data(), act.data(), reward.data(), done.data(), nt.data(), no.data(), masks.data(),
                          valid.data(), w.data(), disc.data(), 0.0f, stats, row_loss.data(), proj.data());
            host_c51_backward(rows, A, lg.data(), act.data(), proj.data(), valid.data(), w.data(), stats, nullptr, grad.data());
            for (long long i = 0; i < rows; ++i) {
                const bool nan_row = rows > 2 && i == 2, dead = rows > 2 && i == 1;
                if (std::isnan(row_loss[i]) != nan_row) {
                    std::printf("A %d row %lld of %lld: NaN where none belongs, or none where one does\n", A, i, rows);
                    return 1;
                }
                float sum = 0.0f;
                for (int j = 0; j < A; ++j) sum += proj[i * A + j];
                if (!nan_row && !dead && !(std::fabs(sum - 1.0f) < 1e-5f)) {
                    std::printf("A %d row %lld of %lld: the projected target sums to %g\n", A, i, rows, (double)sum);
                    return 1;
                }
                if (dead) {
                    uint32_t any = bits(row_loss[i]);
                    for (int j = 0; j < A; ++j) any |= bits(proj[i * A + j]);
                    for (int j = 0; j < 5 * A; ++j) any |= bits(grad[i * 5 * A + j]);
                    if (any != 0u) {
                        std::printf("a row that does not count did not get +0.0 everywhere\n");
                        return 1;
                    }
                }
            }
            if ((rows > 2) != std::isnan(stats[0]) || stats[6] != (float)(rows > 2 ? rows - 1 : rows)) {
                std::printf("A %d rows %lld: stats %g %g\n", A, rows, (double)stats[0], (double)stats[6]);
                return 1;
            }
            total += rows;
        }
    }
    std::printf("%lld rows projected\n", total);
    return 0;
}
#endif
