// ccx_mlp.h -- the per-row rule of CCX_MLP (include/ccx.h) as inline functions: the activation (tanh_spec, relu), one step of
// the layer-1 chain for a group of 16 hidden units, the layer-2 partial of one group and the sum of the partials in group
// order.  Included by ccx_mlp.hip, whose kernels inline exactly these functions; it also compiles with a plain host C++
// compiler (tests/test_mlp_host_rule.py runs mlp_row against the NumPy spec bit for bit).
// Every line is ONE f32 operation: the units that include this are compiled with -ffp-contract=off, and `/` must be the
// correctly rounded division.
#pragma once
#include <stddef.h>

#include "ccx_softmax.h"

namespace ccx_mlp {

constexpr int kGroup = 16;                                               // hidden units per group: the unit of the layer-2 order
constexpr int kMaxL = 512, kMaxH = 256, kMaxO = 8;
constexpr float kTanhClamp = 40.0f;
enum : int { kTanh = 0, kRelu = 1 };

// true when (L, H, O, activation) lies inside CCX_MLP's limits
CCX_HD bool shape_ok(int L, int H, int O, int activation) {
    return L >= 1 && L <= kMaxL && H >= kGroup && H <= kMaxH && H % kGroup == 0 && O >= 1 && O <= kMaxO &&
           (activation == kTanh || activation == kRelu);
}

// LDS floats a workgroup of the forward needs (ccx_mlp_tile.h): the x tile of 64 rows at its odd row stride, later overlaid
// by the partials (and y in the fused kernels, `draw`); a multiple of 64.  Above 65536 bytes (L > 255) the launch opts in.
inline size_t lds_floats(int L, int H, int O, bool draw) {
    const size_t tile = (size_t)64 * (size_t)(L | 1), sums = (size_t)(H / kGroup + (draw ? 1 : 0)) * 64 * (size_t)O;
    return tile > sums ? tile : sums;
}

CCX_HD float relu_spec(float a) { return a < 0.0f ? 0.0f : a; }          // NaN stays NaN, -0.0 stays -0.0

CCX_HD float tanh_spec(float a) {
    const float m0 = __builtin_fabsf(a);
    const float m = m0 < kTanhClamp ? m0 : kTanhClamp;                    // (NaN: 40, selected away below)
    const float t = ccx_softmax::exp_spec(-(m + m));                      // on exp_spec's own domain [-80, 0]
    const float r = (1.0f - t) / (1.0f + t);
    const float s = __builtin_copysignf(r, a);
    return a != a ? a : s;
}

CCX_HD float activate(int activation, float a) { return activation == kRelu ? relu_spec(a) : tanh_spec(a); }

// Layer 1, one k of the chain for the 16 units of a group: a_j = a_j + x_k * w1t[k][16 g + j]; w points at w1t[k][16 g].
CCX_HD void layer1_step(float (&a)[kGroup], float xk, const float* w) {
#pragma unroll
    for (int j = 0; j < kGroup; ++j) a[j] = a[j] + xk * w[j];
}

// Layer 2, the partial of one group for one output: w points at w2[o][16 g].
CCX_HD float layer2_partial(const float (&h)[kGroup], const float* w) {
    float p = h[0] * w[0];
#pragma unroll
    for (int i = 1; i < kGroup; ++i) p = p + h[i] * w[i];
    return p;
}

// Layer 2, the sum: y = b2[o], then the G partials in group order; partial g lies at p[g * stride].
CCX_HD float layer2_sum(float bias, const float* p, int G, int stride) {
    float y = bias;
    for (int g = 0; g < G; ++g) y = y + p[g * stride];
    return y;
}

// One row from end to end, as the kernels compute it: y[O], and hidden[H] where it is not null.
CCX_HD void mlp_row(int L, int H, int O, int activation, const float* x, const float* w1t, const float* b1, const float* w2,
                    const float* b2, float* y, float* hidden_or_null) {
    const int G = H / kGroup;
    float part[kMaxO][kMaxH / kGroup];
    for (int g = 0; g < G; ++g) {
        float a[kGroup];
#pragma unroll
        for (int j = 0; j < kGroup; ++j) a[j] = b1[kGroup * g + j];
        for (int k = 0; k < L; ++k) layer1_step(a, x[k], w1t + (long long)k * H + kGroup * g);
#pragma unroll
        for (int j = 0; j < kGroup; ++j) a[j] = activate(activation, a[j]);
        if (hidden_or_null) {
#pragma unroll
            for (int j = 0; j < kGroup; ++j) hidden_or_null[kGroup * g + j] = a[j];
        }
        for (int o = 0; o < O; ++o) part[o][g] = layer2_partial(a, w2 + o * H + kGroup * g);
    }
    for (int o = 0; o < O; ++o) y[o] = layer2_sum(b2[o], part[o], G, 1);
}

}  // namespace ccx_mlp
