// ccx_mlp_grad.h -- the backward rule of CCX_MLP (include/ccx.h) as inline functions: the per-row f32 part (gh, ga), one
// term of a block's f64 chain, the place of every output element in the workspace, the launch shape of the blocks kernels
// (the LDS image of a row, the rows of a sub-tile, the tile grid), and the final step over the block
// partials, which is ccx_tree.h's (strided_partials, then the halving): the project keeps one tree.  Included by
// ccx_mlp_backward.hip, whose kernels inline exactly these functions; it also compiles with a plain host C++ compiler
// (tests/test_mlp_backward_host_rule.py runs backward_host against the NumPy spec bit for bit).
// The discipline is ccx_mlp.h's and ccx_tree.h's: every line is ONE operation of the stated type, and the including units are
// compiled with -ffp-contract=off.
#pragma once
#include <stddef.h>

#include "ccx_mlp.h"
#include "ccx_tree.h"

namespace ccx_mlp_grad {

constexpr int kBlockRows = ccx_tree::kBlockRows;                          // 256 consecutive rows to a block partial
constexpr int kTile = 4;                                                 // a thread's register tile: 4 x 4 output elements

// The output elements of one call in the order of the workspace: the (L + 1) x H elements of [x | 1]^T ga -- grad_w1t [L][H],
// then grad_b1 [H] as row L -- and behind them the O x (H + 1) elements of grad_y^T [hidden | 1]: row o is grad_w2[o][0 .. H-1],
// then grad_b2[o] as column H.
CCX_HD long long elements_of(int L, int H, int O) { return (long long)(L + 1) * H + (long long)O * (H + 1); }
CCX_HD long long second_part(int L, int H) { return (long long)(L + 1) * H; }

// where element e goes: the output array (0 grad_w1t, 1 grad_b1, 2 grad_w2, 3 grad_b2) and the index in it
CCX_HD int place_of(long long e, int L, int H, long long& index) {
    if (e < (long long)L * H) return index = e, 0;
    if (e < second_part(L, H)) return index = e - (long long)L * H, 1;
    const long long u = e - second_part(L, H), o = u / (H + 1), c = u - o * (H + 1);
    if (c < H) return index = o * H + c, 2;
    return index = o, 3;
}

// B x elements doubles ([element][B]); 0 for rows < 1 or a shape outside CCX_MLP's limits (the activation is not a size)
CCX_HD long long workspace_bytes(long long rows, int L, int H, int O) {
    if (rows < 1 || !ccx_mlp::shape_ok(L, H, O, ccx_mlp::kTanh)) return 0;
    return ccx_tree::blocks_of(rows) * elements_of(L, H, O) * (long long)sizeof(double);
}

// step 1 for one hidden unit: gy the row's O gradients, w = &w2[0][j], stride = H
CCX_HD float gh_unit(int O, const float* gy, const float* w, int stride) {
    float gh = gy[0] * w[0];
    for (int o = 1; o < O; ++o) gh = gh + gy[o] * w[o * stride];
    return gh;
}

// step 2
CCX_HD float ga_tanh(float gh, float h) {
    const float hh = h * h;
    const float d = 1.0f - hh;
    return gh * d;
}
CCX_HD float ga_relu(float gh, float h) { return h > 0.0f ? gh : 0.0f; }  // a select: NaN h gives +0.0f
CCX_HD float ga_unit(int activation, float gh, float h) { return activation == ccx_mlp::kRelu ? ga_relu(gh, h) : ga_tanh(gh, h); }

// One term onto a chain.  The product of two f32 values is exact in f64, so the fused form and the exact multiply followed
// by one add round the same value once: the device takes the first, the host the second, and the tests compare them.
CCX_HD double chain_add(double acc, float a, float b) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_fma((double)a, (double)b, acc);
#else
    const double p = (double)a * (double)b;
    return acc + p;
#endif
}

// one row onto a thread's 4 x 4 tile: acc[i][j] takes a[i] * b[j]
CCX_HD void tile_row(double (&acc)[kTile][kTile], const float (&a)[kTile], const float (&b)[kTile]) {
#pragma unroll
    for (int i = 0; i < kTile; ++i) {
#pragma unroll
        for (int j = 0; j < kTile; ++j) acc[i][j] = chain_add(acc[i][j], a[i], b[j]);
    }
}

// ---- the launch shape of the blocks kernels (ccx_mlp_backward.hip), stated where a host compiler reaches it too
// (tests/test_mlp_shape_classes.py asserts from these which shapes take which branch).
// the LDS image of one row, in floats: x at 0 (the constant 1 at L), ga, hidden (the constant 1 behind it), grad_y
struct RowImage {
    int ga, hid, gy, stride;
};
CCX_HD RowImage row_image(int L, int H, int O) {
    RowImage m;
    m.ga = (L + 4) & ~3;
    m.hid = m.ga + H;
    m.gy = m.hid + H + 4;
    m.stride = m.gy + ((O + 3) & ~3);
    return m;
}

constexpr int kThreads = 256;                                            // of a blocks workgroup: one 4 x 4 tile per thread
constexpr size_t kLdsBudget = 65536;

// rows of a sub-tile: the most of 64, 32, 16, 8 whose images fit the budget beside w2 (8 always do: 33 KB + 8 KB at the limits)
// (`per_row`: further bytes per row behind w2 -- the flat rows of the sides kernel)
inline int sub_rows(int L, int H, int O, size_t& bytes, size_t per_row = 0) {
    const size_t row = (size_t)row_image(L, H, O).stride * sizeof(float) + per_row, fixed = (size_t)O * H * sizeof(float);
    int R = 64;
    while (R > 8 && R * row + fixed > kLdsBudget) R >>= 1;
    bytes = R * row + fixed;
    return R;
}

// the 4 x 4 tiles of one call's elements -- those of [x | 1]^T ga, then those of grad_y^T [hidden | 1] -- and the slices of
// 256 tiles they are cut into: grid.y of the blocks launch
inline int tiles_of(int L, int H, int O) { return (row_image(L, H, O).ga / 4) * (H / 4) + ((O + 3) / 4) * (H / 4 + 1); }
inline unsigned grid_y(int L, int H, int O) { return (unsigned)((tiles_of(L, H, O) + kThreads - 1) / kThreads); }

// ---- the whole rule on the host, one addition at a time.  ws: workspace_bytes(...) bytes; ga: [rows][H] scratch or output.
inline void backward_host(long long rows, int L, int H, int O, int activation, const float* x, const float* hidden,
                          const float* grad_y, const float* w2, double* ws, float* grad_w1t, float* grad_b1, float* grad_w2,
                          float* grad_b2, float* ga) {
    const long long B = ccx_tree::blocks_of(rows), NE = elements_of(L, H, O);
    for (long long r = 0; r < rows; ++r)
        for (int j = 0; j < H; ++j)
            ga[r * H + j] = ga_unit(activation, gh_unit(O, grad_y + r * O, w2 + j, H), hidden[r * H + j]);
    for (long long b = 0; b < B; ++b) {
        const long long r0 = b * kBlockRows, r1 = r0 + kBlockRows < rows ? r0 + kBlockRows : rows;
        for (long long e = 0; e < NE; ++e) {
            long long i;
            const int which = place_of(e, L, H, i);
            double acc = 0.0;
            for (long long r = r0; r < r1; ++r) {
                if (which == 0) acc = chain_add(acc, x[r * L + i / H], ga[r * H + i % H]);
                else if (which == 1) acc = chain_add(acc, 1.0f, ga[r * H + i]);
                else if (which == 2) acc = chain_add(acc, grad_y[r * O + i / H], hidden[r * H + i % H]);
                else acc = chain_add(acc, grad_y[r * O + i], 1.0f);
            }
            ws[e * B + b] = acc;
        }
    }
    for (long long e = 0; e < NE; ++e) {
        const float v = (float)ccx_tree::final_host(ws + e * B, B);
        long long i;
        const int which = place_of(e, L, H, i);
        (which == 0 ? grad_w1t : which == 1 ? grad_b1 : which == 2 ? grad_w2 : grad_b2)[i] = v;
    }
}

}  // namespace ccx_mlp_grad
