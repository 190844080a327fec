// ccx_mlp_deep.h -- CCX_MLP_DEEP (include/ccx.h): Linear(L, H1) -> act -> Linear(H1, H2) -> act -> Linear(H2, O).  The rule is
// CCX_MLP's with one more `Linear + act` layer in front: every operation here is a call of ccx_mlp.h's or ccx_mlp_grad.h's
// functions (the layer chain of 16 units, the activation, the layer-2 partials and their sum; gh_unit, ga_unit, chain_add,
// the final step of ccx_tree.h), on the arrays the header paragraph names.  Nothing of those is restated: this header adds
// the limits, one row from end to end, the backward on the host, the place of every output element in the workspace and
// the launch shapes of ccx_mlp_deep.hip's kernels (the LDS floats of a forward workgroup; the row image, the sub-tile rows
// and the slices of the backward), stated where a host compiler reaches them too (tests/test_mlp_deep_host_rule.py).  The
// discipline is ccx_mlp.h's: every line is ONE operation of the stated type, and the including units are compiled with
// -ffp-contract=off.
#pragma once
#include <stddef.h>

#include "ccx_mlp_grad.h"

namespace ccx_deep {

constexpr int kGroup = ccx_mlp::kGroup;
constexpr int kMaxO = ccx_mlp::kMaxO;

// true when (L, H1, H2, O, activation) lies inside CCX_MLP_DEEP's limits: CCX_MLP's for either layer pair
CCX_HD bool shape_ok(int L, int H1, int H2, int O, int activation) {
    return ccx_mlp::shape_ok(L, H1, 1, activation) && ccx_mlp::shape_ok(H1, H2, O, activation);
}

// One layer `Linear + act` for the 16 units of group g: a_j = b[16 g + j], the chain over the n inputs in order, act.
// (CCX_MLP's steps 1 and 2 with `in` in the place of x; wt is input-major, [n][H].)
CCX_HD void layer_group(float (&a)[kGroup], int activation, int n, int H, int g, const float* in, const float* wt, const float* b) {
#pragma unroll
    for (int j = 0; j < kGroup; ++j) a[j] = b[kGroup * g + j];
    for (int k = 0; k < n; ++k) ccx_mlp::layer1_step(a, in[k], wt + (long long)k * H + kGroup * g);
#pragma unroll
    for (int j = 0; j < kGroup; ++j) a[j] = ccx_mlp::activate(activation, a[j]);
}

// One row from end to end: y[O], and hidden1[H1] / hidden2[H2] where they are not null.  By the rule
// deep_row(x) == ccx_mlp::mlp_row(L := H1, H := H2, O; x := h1, w1t := w2t, b1 := b2, w2 := w3, b2 := b3) on the h1 that
// mlp_row writes as `hidden` for (x, w1t, b1).
CCX_HD void deep_row(int L, int H1, int H2, int O, int activation, const float* x, const float* w1t, const float* b1,
                     const float* w2t, const float* b2, const float* w3, const float* b3, float* y, float* hidden1_or_null,
                     float* hidden2_or_null) {
    float h1[ccx_mlp::kMaxH];
    for (int g = 0; g < H1 / kGroup; ++g) {
        float a[kGroup];
        layer_group(a, activation, L, H1, g, x, w1t, b1);
#pragma unroll
        for (int j = 0; j < kGroup; ++j) h1[kGroup * g + j] = a[j];
    }
    if (hidden1_or_null)
        for (int j = 0; j < H1; ++j) hidden1_or_null[j] = h1[j];
    const int G2 = H2 / kGroup;
    float part[kMaxO][ccx_mlp::kMaxH / kGroup];
    for (int g = 0; g < G2; ++g) {
        float a[kGroup];
        layer_group(a, activation, H1, H2, g, h1, w2t, b2);
        if (hidden2_or_null) {
#pragma unroll
            for (int j = 0; j < kGroup; ++j) hidden2_or_null[kGroup * g + j] = a[j];
        }
        for (int o = 0; o < O; ++o) part[o][g] = ccx_mlp::layer2_partial(a, w3 + o * H2 + kGroup * g);
    }
    for (int o = 0; o < O; ++o) y[o] = ccx_mlp::layer2_sum(b3[o], part[o], G2, 1);
}

// ---- the forward's launch shape (ccx_mlp_deep.hip: deep_tile).  LDS floats of a workgroup: the x tile of 64 rows at its
// odd row stride, overlaid by h1 of the 64 rows at ITS odd stride (H1 | 1), overlaid by the layer-3 partials [G2][64][O]
// (and the tile's y in the fused kernels, `draw`).  Above 65536 bytes the launch opts in; the most is 64 * 513 * 4 = 131328.
inline size_t lds_floats(int L, int H1, int H2, int O, bool draw) {
    const size_t x = (size_t)64 * (size_t)(L | 1), h = (size_t)64 * (size_t)(H1 | 1);
    const size_t sums = (size_t)(H2 / kGroup + (draw ? 1 : 0)) * 64 * (size_t)O;
    const size_t m = x > h ? x : h;
    return m > sums ? m : sums;
}
inline int waves_of(int H1, int H2) { return (H1 > H2 ? H1 : H2) / kGroup; }

// ---- the backward.  ga1 of one unit i of H1 from the row's ga2: the gh1 chain over j = 0 .. H2-1 ascending is
// ccx_mlp_grad::gh_unit on (ga2, w2t[i][..]) at stride 1, then step 2's activation rule on hidden1.
CCX_HD float ga1_unit(int activation, int H2, const float* ga2, const float* w2t_row, float h1) {
    return ccx_mlp_grad::ga_unit(activation, ccx_mlp_grad::gh_unit(H2, ga2, w2t_row, 1), h1);
}

// The output elements in the order of the workspace ([element][B] doubles): the (L + 1) x H1 elements of [x | 1]^T ga1
// (grad_w1t, grad_b1 as row L), then ccx_mlp_grad.h's elements of (L := H1, H := H2, O): the (H1 + 1) x H2 of
// [hidden1 | 1]^T ga2 (grad_w2t, grad_b2 as row H1) and the O x (H2 + 1) of grad_y^T [hidden2 | 1] (grad_w3, grad_b3 as
// column H2).  So each of the two stretches is finished by CCX_MLP's final kernel as it is.
CCX_HD long long first_elements(int L, int H1) { return (long long)(L + 1) * H1; }
CCX_HD long long elements_of(int L, int H1, int H2, int O) { return first_elements(L, H1) + ccx_mlp_grad::elements_of(H1, H2, O); }

// B x elements doubles; 0 for rows < 1 or a shape outside the limits
CCX_HD long long workspace_bytes(long long rows, int L, int H1, int H2, int O) {
    if (rows < 1 || !shape_ok(L, H1, H2, O, ccx_mlp::kTanh)) return 0;
    return ccx_tree::blocks_of(rows) * elements_of(L, H1, H2, O) * (long long)sizeof(double);
}

// the LDS image of one row of the blocks kernel, in floats; every part starts at a multiple of four: x (the constant 1 at
// L), ga1, hidden1 (1 at H1), ga2, hidden2 (1 at H2), grad_y (8 floats)
struct RowImage {
    int ga1, h1, ga2, h2, gy, stride;
};
CCX_HD RowImage row_image(int L, int H1, int H2) {
    RowImage m;
    m.ga1 = (L + 4) & ~3;
    m.h1 = m.ga1 + H1;
    m.ga2 = m.h1 + H1 + 4;
    m.h2 = m.ga2 + H2;
    m.gy = m.h2 + H2 + 4;
    m.stride = m.gy + kMaxO;
    return m;
}
constexpr int kThreads = ccx_mlp_grad::kThreads;
// rows of a sub-tile: the most of 64, 32, 16, 8 whose images fit 64 KB beside w3 (8 always do: 49792 + 8192 at the limits)
inline int sub_rows(int L, int H1, int H2, int O, size_t& bytes) {
    const size_t row = (size_t)row_image(L, H1, H2).stride * sizeof(float), fixed = (size_t)O * H2 * sizeof(float);
    int R = 64;
    while (R > 8 && R * row + fixed > ccx_mlp_grad::kLdsBudget) R >>= 1;
    bytes = R * row + fixed;
    return R;
}
// The first product's slices need ga1 = the gh1 chains along the rows of w2t: w2t passes through LDS in slabs of
// kSlabUnits consecutive units of H1 (whole rows of w2t: coalesced loads) at the odd pitch H2 + 1, so the lanes of a wave,
// which walk the chains of different units side by side, read different banks.  The slab lies behind the images and w3;
// above 65536 bytes in all the launch opts in (91 KB at the limits).
constexpr int kSlabUnits = 32;
inline int slab_units(int H1) { return H1 < kSlabUnits ? H1 : kSlabUnits; }
inline size_t grad_lds_bytes(int L, int H1, int H2, int O) {
    size_t bytes = 0;
    sub_rows(L, H1, H2, O, bytes);
    return bytes + (size_t)slab_units(H1) * (size_t)(H2 + 1) * sizeof(float);
}
// the slices of 256 4 x 4 tiles of the three products; a slice lies in ONE product
inline unsigned slices(int tiles) { return (unsigned)((tiles + kThreads - 1) / kThreads); }
inline unsigned slices1(int L, int H1) { return slices(((L + 4) / 4) * (H1 / 4)); }
inline unsigned slices2(int H1, int H2) { return slices(((H1 + 4) / 4) * (H2 / 4)); }
inline unsigned slices3(int H2, int O) { return slices(((O + 3) / 4) * (H2 / 4 + 1)); }
inline unsigned grid_y(int L, int H1, int H2, int O) { return slices1(L, H1) + slices2(H1, H2) + slices3(H2, O); }

// ---- the whole backward on the host, one addition at a time.  ws: workspace_bytes(...) bytes; ga1 [rows][H1] and
// ga2 [rows][H2]: scratch or outputs.  By the rule: (grad_w2t, grad_b2, grad_w3, grad_b3, ga2) is
// ccx_mlp_grad::backward_host(L := H1, H := H2, O; x := hidden1, hidden := hidden2, grad_y, w2 := w3), and
// (grad_w1t, grad_b1, ga1) is CCX_MLP_WIDE's backward of (L, H := H1, O := H2; x, hidden := hidden1, grad_y := ga2,
// w2 := w2t transposed).
inline void backward_host(long long rows, int L, int H1, int H2, int O, int activation, const float* x, const float* hidden1,
                          const float* hidden2, const float* grad_y, const float* w2t, const float* w3, double* ws, float* grad_w1t,
                          float* grad_b1, float* grad_w2t, float* grad_b2, float* grad_w3, float* grad_b3, float* ga1, float* ga2) {
    const long long B = ccx_tree::blocks_of(rows), E1 = first_elements(L, H1);
    // the last two layers: CCX_MLP's backward on (hidden1, hidden2, grad_y, w3), its partials behind the first stretch
    ccx_mlp_grad::backward_host(rows, H1, H2, O, activation, hidden1, hidden2, grad_y, w3, ws + E1 * B, grad_w2t, grad_b2, grad_w3,
                                grad_b3, ga2);
    for (long long r = 0; r < rows; ++r)
        for (int i = 0; i < H1; ++i) ga1[r * H1 + i] = ga1_unit(activation, H2, ga2 + r * H2, w2t + (long long)i * H2, hidden1[r * H1 + i]);
    for (long long b = 0; b < B; ++b) {
        const long long r0 = b * ccx_mlp_grad::kBlockRows, r1 = r0 + ccx_mlp_grad::kBlockRows < rows ? r0 + ccx_mlp_grad::kBlockRows : rows;
        for (long long e = 0; e < E1; ++e) {
            const long long k = e / H1, i = e - k * H1;
            double acc = 0.0;
            for (long long r = r0; r < r1; ++r) acc = ccx_mlp_grad::chain_add(acc, k < L ? x[r * L + k] : 1.0f, ga1[r * H1 + i]);
            ws[e * B + b] = acc;
        }
    }
    for (long long e = 0; e < E1; ++e) {
        const float v = (float)ccx_tree::final_host(ws + e * B, B);
        (e < (long long)L * H1 ? grad_w1t[e] : grad_b1[e - (long long)L * H1]) = v;
    }
}

}  // namespace ccx_deep
