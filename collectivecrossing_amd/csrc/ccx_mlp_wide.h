// ccx_mlp_wide.h -- CCX_MLP_WIDE (include/ccx.h): CCX_MLP's rule with up to 320 outputs.  The rule is ccx_mlp.h's and
// ccx_mlp_grad.h's, taken as it is: this header adds only what a wide O needs around it -- the limits, a host row function
// with storage of its own (ccx_mlp::mlp_row keeps the partials of 8 outputs), the gh chain of ccx_mlp_grad::gh_unit cut at
// slab boundaries, and the launch shapes of the two kernels of ccx_mlp_wide.hip (the output chunks of the forward; the
// roles, sub-tile rows, w2 slabs and grid of the backward), stated where a host compiler reaches them too
// (tests/test_mlp_wide_shape_classes.py asserts from these which shapes take which branch).  It compiles with a plain host
// C++ compiler (tests/test_mlp_wide_host_rule.py).  The discipline is ccx_mlp.h's: every line is ONE operation of the
// stated type, and the including units are compiled with -ffp-contract=off.
#pragma once
#include <stddef.h>

#include "ccx_mlp_grad.h"

namespace ccx_wide {

constexpr int kGroup = ccx_mlp::kGroup;
constexpr int kMaxO = 320;                                               // 5 actions x 64 atoms (CCX_C51)

// true when (L, H, O, activation) lies inside CCX_MLP_WIDE's limits: CCX_MLP's, with O up to 320
CCX_HD bool shape_ok(int L, int H, int O, int activation) {
    return ccx_mlp::shape_ok(L, H, 1, activation) && O >= 1 && O <= kMaxO;
}

// One row from end to end: ccx_mlp::mlp_row with the activations of all groups kept and the partials of one output at a time.
CCX_HD void wide_row(int L, int H, int O, int activation, const float* x, const float* w1t, const float* b1, const float* w2,
                     const float* b2, float* y, float* hidden_or_null) {
    const int G = H / kGroup;
    float act[ccx_mlp::kMaxH / kGroup][kGroup];
    for (int g = 0; g < G; ++g) {
        float (&a)[kGroup] = act[g];
#pragma unroll
        for (int j = 0; j < kGroup; ++j) a[j] = b1[kGroup * g + j];
        for (int k = 0; k < L; ++k) ccx_mlp::layer1_step(a, x[k], w1t + (long long)k * H + kGroup * g);
#pragma unroll
        for (int j = 0; j < kGroup; ++j) a[j] = ccx_mlp::activate(activation, a[j]);
        if (hidden_or_null) {
#pragma unroll
            for (int j = 0; j < kGroup; ++j) hidden_or_null[kGroup * g + j] = a[j];
        }
    }
    for (int o = 0; o < O; ++o) {
        float part[ccx_mlp::kMaxH / kGroup];
        for (int g = 0; g < G; ++g) part[g] = ccx_mlp::layer2_partial(act[g], w2 + (long long)o * H + kGroup * g);
        y[o] = ccx_mlp::layer2_sum(b2[o], part, G, 1);
    }
}

// ---- the forward's launch shape (ccx_mlp_wide.hip: wide_forward_kernel).  Layer 2 runs over chunks of C consecutive
// outputs; a chunk's partials lie in LDS as [G][C][65] floats (the 64 rows of an output contiguous, one float of padding).
// C is the most outputs, in multiples of 32 -- a 128-byte line of a row of y --, whose partials fit 65536 bytes, and 32
// where even those do not (G > 7: the launch opts in, up to 133120 bytes at G = 16); no more than O.
constexpr int kRowPitch = 65;
constexpr size_t kLdsBudget = ccx_mlp_grad::kLdsBudget;
inline int chunk_outputs(int H, int O) {
    const int G = H / kGroup;
    int C = (int)(kLdsBudget / sizeof(float) / (size_t)(G * kRowPitch)) / 32 * 32;
    if (C < 32) C = 32;
    return C < O ? C : O;
}
inline int chunks_of(int H, int O) { return (O + chunk_outputs(H, O) - 1) / chunk_outputs(H, O); }
// LDS floats of a forward workgroup: the x tile of 64 rows at its odd stride, later overlaid by a chunk's partials
inline size_t lds_floats(int L, int H, int O) {
    const size_t tile = (size_t)64 * (size_t)(L | 1), sums = (size_t)(H / kGroup) * chunk_outputs(H, O) * kRowPitch;
    return tile > sums ? tile : sums;
}

// ---- the backward: the gh chain of ccx_mlp_grad::gh_unit cut at slab boundaries (o ascending, so slabs of consecutive o
// leave the order as it is).  gh_unit starts from the first product alone; a chain that is continued slab by slab starts
// from kChainStart = -0.0f instead, the identity of the f32 addition: (-0.0f) + p has the bits of p for every p that is no
// NaN (+0.0f would turn a product of -0.0f into +0.0f), so the first step leaves the first product and every slab is the
// same loop.  gy / w point at the slab's first output; four adjacent units (w at the first) run side by side, each chain in
// its own order.
constexpr float kChainStart = -0.0f;
CCX_HD float gh_more(float gh, int n, const float* gy, const float* w, int stride) {
    for (int o = 0; o < n; ++o) gh = gh + gy[o] * w[o * stride];
    return gh;
}
CCX_HD void gh_more4(float (&gh)[4], int n, const float* gy, const float* w, int stride) {
    for (int o = 0; o < n; ++o) {
#pragma unroll
        for (int c = 0; c < 4; ++c) gh[c] = gh_more(gh[c], 1, gy + o, w + o * stride + c, stride);
    }
}

// ---- the backward's launch shape (ccx_mlp_wide.hip: wide_grad_blocks_kernel).  The 4 x 4 tiles of the output elements are
// ccx_mlp_grad.h's; a workgroup takes 256 of ONE part: slices 0 .. Y1 - 1 the tiles of [x | 1]^T ga, slices Y1 .. the tiles
// of grad_y^T [hidden | 1].  Only the first need ga (and so the whole gh chain, w2 streamed through LDS in slabs of
// consecutive outputs); the second need hidden and the grad_y columns of their own tiles.
constexpr int kThreads = ccx_mlp_grad::kThreads;
constexpr int kSlabFloats = 4096;                                        // of w2 in LDS at a time: 16 KB
inline int slab_outputs(int H, int O) { return kSlabFloats / H < O ? kSlabFloats / H : O; }
inline int slabs_of(int H, int O) { return (O + slab_outputs(H, O) - 1) / slab_outputs(H, O); }

inline int first_tiles(int L, int H) { return ((L + 4) / 4) * (H / 4); }
inline int second_tiles(int H, int O) { return ((O + 3) / 4) * (H / 4 + 1); }
inline unsigned first_slices(int L, int H) { return (unsigned)((first_tiles(L, H) + kThreads - 1) / kThreads); }
inline unsigned second_slices(int H, int O) { return (unsigned)((second_tiles(H, O) + kThreads - 1) / kThreads); }
inline unsigned grid_y(int L, int H, int O) { return first_slices(L, H) + second_slices(H, O); }

// a row's LDS image in the first part, in floats: x at 0 (the constant 1 at L), ga (gh while the slabs pass), then the row's
// grad_y of the current slab
struct FirstImage {
    int ga, gy, stride;
};
CCX_HD FirstImage first_image(int L, int H, int slab) {
    FirstImage m;
    m.ga = (L + 4) & ~3;
    m.gy = m.ga + H;
    m.stride = m.gy + ((slab + 3) & ~3);
    return m;
}
// .. in the second part: hidden at 0 (the constant 1 at H), then the grad_y columns of the slice's tiles.  A slice of 256
// tiles touches at most ceil(255 / (H / 4 + 1)) + 1 rows of tiles, four columns each.
struct SecondImage {
    int gy, stride;
};
CCX_HD int second_columns(int H, int O) {
    const int JT = H / 4 + 1, most = 4 * ((kThreads - 1 + JT - 1) / JT + 1), all = (O + 3) & ~3;
    return most < all ? most : all;
}
CCX_HD SecondImage second_image(int H, int O) {
    SecondImage m;
    m.gy = H + 4;
    m.stride = m.gy + second_columns(H, O);
    return m;
}

// rows of a sub-tile: the most of 64, 32, 16, 8 whose images fit the budget (beside the w2 slab in the first part)
inline int first_rows(int L, int H, int O, size_t& bytes) {
    const int S = slab_outputs(H, O);
    const size_t row = (size_t)first_image(L, H, S).stride * sizeof(float), fixed = (size_t)S * H * sizeof(float);
    int R = 64;
    while (R > 8 && R * row + fixed > kLdsBudget) R >>= 1;
    bytes = R * row + fixed;
    return R;
}
inline int second_rows(int H, int O, size_t& bytes) {
    const size_t row = (size_t)second_image(H, O).stride * sizeof(float);
    int R = 64;
    while (R > 8 && R * row > kLdsBudget) R >>= 1;
    bytes = R * row;
    return R;
}
// dynamic LDS of a blocks workgroup: both roles run in one launch
inline size_t grad_lds_bytes(int L, int H, int O) {
    size_t a = 0, b = 0;
    first_rows(L, H, O, a);
    second_rows(H, O, b);
    return a > b ? a : b;
}

// B x elements doubles, as CCX_MLP's; 0 for rows < 1 or a shape outside the limits
CCX_HD long long workspace_bytes(long long rows, int L, int H, int O) {
    if (rows < 1 || !ccx_wide::shape_ok(L, H, O, ccx_mlp::kTanh)) return 0;
    return ccx_tree::blocks_of(rows) * ccx_mlp_grad::elements_of(L, H, O) * (long long)sizeof(double);
}

// ga of every row as the blocks kernel forms it: the gh chain slab by slab, then ccx_mlp_grad::ga_unit
inline void ga_slabs_host(long long rows, int H, int O, int activation, const float* hidden, const float* grad_y, const float* w2,
                          float* ga) {
    const int S = slab_outputs(H, O);
    for (long long r = 0; r < rows; ++r)
        for (int j = 0; j < H; ++j) {
            float gh = kChainStart;
            for (int o0 = 0; o0 < O; o0 += S) gh = gh_more(gh, O - o0 < S ? O - o0 : S, grad_y + r * O + o0, w2 + (long long)o0 * H + j, H);
            ga[r * H + j] = ccx_mlp_grad::ga_unit(activation, gh, hidden[r * H + j]);
        }
}

// the whole backward on the host: ccx_mlp_grad::backward_host is general in O
inline void backward_host(long long rows, int L, int H, int O, int activation, const float* x, const float* hidden,
                          const float* grad_y, const float* w2, double* ws, float* grad_w1t, float* grad_b1, float* grad_w2,
                          float* grad_b2, float* ga) {
    ccx_mlp_grad::backward_host(rows, L, H, O, activation, x, hidden, grad_y, w2, ws, grad_w1t, grad_b1, grad_w2, grad_b2, ga);
}

}  // namespace ccx_wide
