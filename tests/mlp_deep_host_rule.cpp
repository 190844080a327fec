// The rules of csrc/ccx_mlp_deep.h compiled for the host (tests/test_mlp_deep_host_rule.py: -O2 -ffp-contract=off), behind a
// C interface for ctypes: the deep row function and backward, CCX_MLP's own row function and backward beside them (the
// identities of the rule are stated against those), and the launch-shape functions of the kernels.  With
// -DMLP_DEEP_HOST_MAIN the same source is a program of its own (run under the sanitizers): every array has exactly its size.
#include "ccx_mlp_deep.h"

#include <cstdio>
#include <cstring>
#include <vector>

namespace dp = ccx_deep;
namespace mg = ccx_mlp_grad;

extern "C" {

// y f32 [rows][O], hidden1 f32 [rows][H1] or null, hidden2 f32 [rows][H2] or null, by ccx_deep::deep_row; -1 outside the limits
int host_deep(long long rows, int L, int H1, int H2, int O, int activation, const float* x, const float* w1t, const float* b1,
              const float* w2t, const float* b2, const float* w3, const float* b3, float* y, float* h1_or_null, float* h2_or_null) {
    if (rows < 1 || !dp::shape_ok(L, H1, H2, O, activation)) return -1;
    for (long long r = 0; r < rows; ++r)
        dp::deep_row(L, H1, H2, O, activation, x + r * L, w1t, b1, w2t, b2, w3, b3, y + r * O, h1_or_null ? h1_or_null + r * H1 : nullptr,
                     h2_or_null ? h2_or_null + r * H2 : nullptr);
    return 0;
}

// CCX_MLP's row function (ccx_mlp::mlp_row)
int host_narrow(long long rows, int L, int H, int O, int activation, const float* x, const float* w1t, const float* b1,
                const float* w2, const float* b2, float* y, float* hidden_or_null) {
    if (rows < 1 || !ccx_mlp::shape_ok(L, H, O, activation)) return -1;
    for (long long r = 0; r < rows; ++r)
        ccx_mlp::mlp_row(L, H, O, activation, x + r * L, w1t, b1, w2, b2, y + r * O, hidden_or_null ? hidden_or_null + r * H : nullptr);
    return 0;
}

long long host_deep_workspace_bytes(long long rows, int L, int H1, int H2, int O) { return dp::workspace_bytes(rows, L, H1, H2, O); }

// the six gradients, ga1 f32 [rows][H1] and ga2 f32 [rows][H2] by ccx_deep::backward_host
int host_deep_backward(long long rows, int L, int H1, int H2, int O, int activation, const float* x, const float* hidden1,
                       const float* hidden2, const float* grad_y, const float* w2t, const float* w3, float* grad_w1t, float* grad_b1,
                       float* grad_w2t, float* grad_b2, float* grad_w3, float* grad_b3, float* ga1, float* ga2) {
    if (rows < 1 || !dp::shape_ok(L, H1, H2, O, activation)) return -1;
    std::vector<double> ws((size_t)(dp::workspace_bytes(rows, L, H1, H2, O) / (long long)sizeof(double)), -7.0);
    dp::backward_host(rows, L, H1, H2, O, activation, x, hidden1, hidden2, grad_y, w2t, w3, ws.data(), grad_w1t, grad_b1, grad_w2t, grad_b2,
                      grad_w3, grad_b3, ga1, ga2);
    return 0;
}

// CCX_MLP's backward (ccx_mlp_grad::backward_host: general in O, so it also serves the wide identity with O := H2)
int host_narrow_backward(long long rows, int L, int H, int O, int activation, const float* x, const float* hidden, const float* grad_y,
                         const float* w2, float* grad_w1t, float* grad_b1, float* grad_w2, float* grad_b2, float* ga) {
    if (rows < 1 || !ccx_mlp::shape_ok(L, H, 1, activation) || O < 1) return -1;
    std::vector<double> ws((size_t)(ccx_tree::blocks_of(rows) * mg::elements_of(L, H, O)), -7.0);
    mg::backward_host(rows, L, H, O, activation, x, hidden, grad_y, w2, ws.data(), grad_w1t, grad_b1, grad_w2, grad_b2, ga);
    return 0;
}

// the launch shapes: out[0..7] = forward LDS bytes, fused-forward LDS bytes, waves of a forward workgroup, rows of a backward
// sub-tile, backward LDS bytes, slices of the three products; returns 0, -1 outside the limits
int host_deep_shape(int L, int H1, int H2, int O, long long* out) {
    if (!dp::shape_ok(L, H1, H2, O, ccx_mlp::kTanh)) return -1;
    size_t bytes = 0;
    out[0] = (long long)(dp::lds_floats(L, H1, H2, O, false) * sizeof(float));
    out[1] = (long long)(dp::lds_floats(L, H1, H2, O, true) * sizeof(float));
    out[2] = dp::waves_of(H1, H2);
    out[3] = dp::sub_rows(L, H1, H2, O, bytes);
    out[4] = (long long)dp::grad_lds_bytes(L, H1, H2, O);
    out[5] = dp::slices1(L, H1);
    out[6] = dp::slices2(H1, H2);
    out[7] = dp::slices3(H2, O);
    return dp::grid_y(L, H1, H2, O) == out[5] + out[6] + out[7] ? 0 : -2;
}

}  // extern "C"

#ifdef MLP_DEEP_HOST_MAIN
// Every array is a vector of exactly its size; inputs are a fixed pseudo-random sequence.
static unsigned g_state = 12345u;
static float draw() {
    g_state = g_state * 1664525u + 1013904223u;
    return (float)((int)(g_state >> 9) % 2001 - 1000) / 500.0f;
}

int main() {
    const int shapes[][5] = {{1, 16, 16, 1, 0}, {38, 64, 64, 5, 0}, {18, 16, 32, 5, 1}, {38, 48, 16, 6, 0}, {262, 256, 256, 8, 1}, {512, 16, 256, 1, 0}};
    long long total = 0;
    for (const auto& s : shapes) {
        const int L = s[0], H1 = s[1], H2 = s[2], O = s[3], act = s[4];
        const long long rows = H1 * H2 > 4096 ? 9 : 259;
        std::vector<float> x((size_t)rows * L), w1t((size_t)L * H1), b1(H1), w2t((size_t)H1 * H2), b2(H2), w3((size_t)O * H2), b3(O),
            y((size_t)rows * O), h1((size_t)rows * H1), h2((size_t)rows * H2), gy((size_t)rows * O), gw1t((size_t)L * H1), gb1(H1),
            gw2t((size_t)H1 * H2), gb2(H2), gw3((size_t)O * H2), gb3(O), ga1((size_t)rows * H1), ga2((size_t)rows * H2);
        for (auto* v : {&x, &w1t, &b1, &w2t, &b2, &w3, &b3, &gy})
            for (float& f : *v) f = draw();
        if (host_deep(rows, L, H1, H2, O, act, x.data(), w1t.data(), b1.data(), w2t.data(), b2.data(), w3.data(), b3.data(), y.data(),
                      h1.data(), h2.data()))
            return 2;
        // the forward identity: CCX_MLP's row function on hidden1
        std::vector<float> y2(y.size()), h22(h2.size());
        if (host_narrow(rows, H1, H2, O, act, h1.data(), w2t.data(), b2.data(), w3.data(), b3.data(), y2.data(), h22.data())) return 3;
        if (std::memcmp(y.data(), y2.data(), y.size() * sizeof(float)) || std::memcmp(h2.data(), h22.data(), h2.size() * sizeof(float))) return 4;
        if (host_deep_backward(rows, L, H1, H2, O, act, x.data(), h1.data(), h2.data(), gy.data(), w2t.data(), w3.data(), gw1t.data(),
                               gb1.data(), gw2t.data(), gb2.data(), gw3.data(), gb3.data(), ga1.data(), ga2.data()))
            return 5;
        // the first backward identity: CCX_MLP's backward on (hidden1, hidden2, grad_y, w3)
        std::vector<float> nw(gw2t.size()), nb(gb2.size()), nw3(gw3.size()), nb3(gb3.size()), nga(ga2.size());
        if (host_narrow_backward(rows, H1, H2, O, act, h1.data(), h2.data(), gy.data(), w3.data(), nw.data(), nb.data(), nw3.data(),
                                 nb3.data(), nga.data()))
            return 6;
        if (std::memcmp(nw.data(), gw2t.data(), nw.size() * sizeof(float)) || std::memcmp(nga.data(), ga2.data(), nga.size() * sizeof(float)) ||
            std::memcmp(nw3.data(), gw3.data(), nw3.size() * sizeof(float)))
            return 7;
        long long shape[8];
        if (host_deep_shape(L, H1, H2, O, shape)) return 8;
        total += rows;
    }
    std::printf("%lld rows through the deep rule\n", total);
    return 0;
}
#endif
