// The rules of csrc/ccx_dueling.h compiled for the host (tests/test_dueling_host_rule.py: -O2 -ffp-contract=off), behind a C
// interface for ctypes.  The loops here only walk rows; every arithmetic operation is one of ccx_dueling.h's.
// With -DDUELING_HOST_MAIN the same source is a program of its own (built with -fsanitize=address,undefined by the test): it
// runs both rules over heap arrays of exactly the rows' size and checks the identities of the rule.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "ccx_dueling.h"

extern "C" {

void host_dueling_forward(long long rows, const float* va, float* q) {
    for (long long i = 0; i < rows; ++i) {
        float in[6], out[5];
        for (int k = 0; k < 6; ++k) in[k] = va[i * 6 + k];
        ccx_dueling::forward(in, out);
        for (int k = 0; k < 5; ++k) q[i * 5 + k] = out[k];
    }
}

void host_dueling_backward(long long rows, const float* grad_q, float* grad_va) {
    for (long long i = 0; i < rows; ++i) {
        float in[5], out[6];
        for (int k = 0; k < 5; ++k) in[k] = grad_q[i * 5 + k];
        ccx_dueling::backward(in, out);
        for (int k = 0; k < 6; ++k) grad_va[i * 6 + k] = out[k];
    }
}

}  // extern "C"

#ifdef DUELING_HOST_MAIN
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
    for (long long rows : {1ll, 2ll, 63ll, 64ll, 65ll, 257ll, 1000ll}) {
        std::vector<float> va(rows * 6), q(rows * 5), g(rows * 5), gva(rows * 6);
        for (auto& x : va) x = (float)((int)(next(seed) % 2001u) - 1000) * 0.125f;
        for (auto& x : g) x = (float)((int)(next(seed) % 2001u) - 1000) * 0.0625f;
        if (rows > 2) {
            va[6 * 1 + 3] = NAN;                                           // row 1: a NaN advantage
            for (int k = 0; k < 5; ++k) g[5 * 2 + k] = 0.0f;              // row 2: a gradient of zeros
        }
        host_dueling_forward(rows, va.data(), q.data());
        host_dueling_backward(rows, g.data(), gva.data());
        for (long long i = 0; i < rows; ++i) {
            const bool nan_row = rows > 2 && i == 1;
            for (int k = 0; k < 5; ++k)
                if (std::isnan(q[i * 5 + k]) != nan_row) {
                    std::printf("row %lld of %lld: NaN where none belongs, or none where one does\n", i, rows);
                    return 1;
                }
        }
        if (rows > 2)
            for (int k = 0; k < 6; ++k)
                if (bits(gva[6 * 2 + k]) != 0u) {
                    std::printf("a gradient of zeros did not give +0.0\n");
                    return 1;
                }
        total += rows;
    }
    std::printf("%lld rows combined\n", total);
    return 0;
}
#endif
