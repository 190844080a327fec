// The rules of csrc/ccx_mlp_wide.h compiled for the host (tests/test_mlp_wide_host_rule.py: -O2 -ffp-contract=off), behind
// a C interface for ctypes: the wide row function and backward, the narrow ones of ccx_mlp.h / ccx_mlp_grad.h beside them
// (for O <= 8 the two must agree), and the launch-shape functions of the two kernels.  With -DMLP_WIDE_HOST_MAIN the same
// source is a program of its own (run under the sanitizers): every array has exactly its size.
#include "ccx_mlp_wide.h"

#include <cstdio>
#include <cstring>
#include <vector>

namespace wd = ccx_wide;
namespace mg = ccx_mlp_grad;

extern "C" {

// y f32 [rows][O], hidden f32 [rows][H] or null, by ccx_wide::wide_row; -1 for a shape outside CCX_MLP_WIDE's limits
int host_wide(long long rows, int L, int H, int O, int activation, const float* x, const float* w1t, const float* b1,
              const float* w2, const float* b2, float* y, float* hidden_or_null) {
    if (rows < 1 || !wd::shape_ok(L, H, O, activation)) return -1;
    for (long long r = 0; r < rows; ++r)
        wd::wide_row(L, H, O, activation, x + r * L, w1t, b1, w2, b2, y + r * O, hidden_or_null ? hidden_or_null + r * H : nullptr);
    return 0;
}

// .. by ccx_mlp::mlp_row (O <= 8)
int host_narrow(long long rows, int L, int H, int O, int activation, const float* x, const float* w1t, const float* b1,
                const float* w2, const float* b2, float* y, float* hidden_or_null) {
    if (rows < 1 || !ccx_mlp::shape_ok(L, H, O, activation)) return -1;
    for (long long r = 0; r < rows; ++r)
        ccx_mlp::mlp_row(L, H, O, activation, x + r * L, w1t, b1, w2, b2, y + r * O, hidden_or_null ? hidden_or_null + r * H : nullptr);
    return 0;
}

long long host_wide_workspace_bytes(long long rows, int L, int H, int O) { return wd::workspace_bytes(rows, L, H, O); }

// the four gradients and ga f32 [rows][H] by ccx_wide::backward_host; ga_slabs f32 [rows][H]: ga as the blocks kernel forms it,
// the gh chain slab by slab
int host_wide_backward(long long rows, int L, int H, int O, int activation, const float* x, const float* hidden, const float* grad_y,
                       const float* w2, float* grad_w1t, float* grad_b1, float* grad_w2, float* grad_b2, float* ga, float* ga_slabs) {
    if (rows < 1 || !wd::shape_ok(L, H, O, activation)) return -1;
    std::vector<double> ws((size_t)(wd::workspace_bytes(rows, L, H, O) / (long long)sizeof(double)), -7.0);
    wd::backward_host(rows, L, H, O, activation, x, hidden, grad_y, w2, ws.data(), grad_w1t, grad_b1, grad_w2, grad_b2, ga);
    wd::ga_slabs_host(rows, H, O, activation, hidden, grad_y, w2, ga_slabs);
    return 0;
}

// .. by ccx_mlp_grad::backward_host under CCX_MLP's own limits (O <= 8)
int host_narrow_backward(long long rows, int L, int H, int O, int activation, const float* x, const float* hidden, const float* grad_y,
                         const float* w2, float* grad_w1t, float* grad_b1, float* grad_w2, float* grad_b2, float* ga) {
    if (rows < 1 || !ccx_mlp::shape_ok(L, H, O, activation)) return -1;
    std::vector<double> ws((size_t)(mg::workspace_bytes(rows, L, H, O) / (long long)sizeof(double)), -7.0);
    mg::backward_host(rows, L, H, O, activation, x, hidden, grad_y, w2, ws.data(), grad_w1t, grad_b1, grad_w2, grad_b2, ga);
    return 0;
}

// the launch shapes: out[0..10] = chunk outputs, chunks, forward LDS bytes, slab outputs, slabs, first-part rows, first-part
// bytes, second-part rows, second-part bytes, first slices, grid.y; returns 0, -1 outside the limits
int host_wide_shape(int L, int H, int O, long long* out) {
    if (!wd::shape_ok(L, H, O, ccx_mlp::kTanh)) return -1;
    size_t b1 = 0, b2 = 0;
    const int R1 = wd::first_rows(L, H, O, b1), R2 = wd::second_rows(H, O, b2);
    out[0] = wd::chunk_outputs(H, O);
    out[1] = wd::chunks_of(H, O);
    out[2] = (long long)(wd::lds_floats(L, H, O) * sizeof(float));
    out[3] = wd::slab_outputs(H, O);
    out[4] = wd::slabs_of(H, O);
    out[5] = R1;
    out[6] = (long long)b1;
    out[7] = R2;
    out[8] = (long long)b2;
    out[9] = wd::first_slices(L, H);
    out[10] = wd::grid_y(L, H, O);
    return (long long)wd::grad_lds_bytes(L, H, O) == (out[6] > out[8] ? out[6] : out[8]) ? 0 : -2;
}

}  // extern "C"

#ifdef MLP_WIDE_HOST_MAIN
// Every array is a vector of exactly its size; inputs are a fixed pseudo-random sequence.
static unsigned g_state = 12345u;
static float draw() {
    g_state = g_state * 1664525u + 1013904223u;
    return (float)((int)(g_state >> 9) % 2001 - 1000) / 500.0f;
}

int main() {
    const int shapes[][4] = {{7, 16, 1, 0}, {38, 64, 255, 0}, {5, 48, 320, 1}, {512, 256, 9, 0}, {3, 256, 319, 1}, {38, 64, 8, 0}};
    long long total = 0;
    for (const auto& s : shapes) {
        const int L = s[0], H = s[1], O = s[2], act = s[3];
        const long long rows = L > 100 ? 9 : 259;
        std::vector<float> x((size_t)rows * L), w1t((size_t)L * H), b1(H), w2((size_t)O * H), b2(O), y((size_t)rows * O),
            hid((size_t)rows * H), gy((size_t)rows * O), gw1t((size_t)L * H), gb1(H), gw2((size_t)O * H), gb2(O), ga((size_t)rows * H),
            gas((size_t)rows * H);
        for (auto* v : {&x, &w1t, &b1, &w2, &b2, &gy})
            for (float& f : *v) f = draw();
        if (host_wide(rows, L, H, O, act, x.data(), w1t.data(), b1.data(), w2.data(), b2.data(), y.data(), hid.data())) return 2;
        if (host_wide_backward(rows, L, H, O, act, x.data(), hid.data(), gy.data(), w2.data(), gw1t.data(), gb1.data(), gw2.data(),
                               gb2.data(), ga.data(), gas.data()))
            return 3;
        if (std::memcmp(ga.data(), gas.data(), ga.size() * sizeof(float))) return 4;
        if (O <= 8) {
            std::vector<float> y2(y.size()), hid2(hid.size());
            if (host_narrow(rows, L, H, O, act, x.data(), w1t.data(), b1.data(), w2.data(), b2.data(), y2.data(), hid2.data())) return 5;
            if (std::memcmp(y.data(), y2.data(), y.size() * sizeof(float)) || std::memcmp(hid.data(), hid2.data(), hid.size() * sizeof(float)))
                return 6;
        }
        long long shape[11];
        if (host_wide_shape(L, H, O, shape)) return 7;
        total += rows;
    }
    std::printf("%lld rows through the wide rule\n", total);
    return 0;
}
#endif
