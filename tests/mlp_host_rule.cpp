// The per-row rule of csrc/ccx_mlp.h compiled for the host (tests/test_mlp_host_rule.py: -O2 -ffp-contract=off), behind a C
// interface for ctypes.
#include "ccx_mlp.h"

extern "C" {

// y f32 [rows][O], hidden f32 [rows][H] or null; returns 0, or -1 for a shape outside CCX_MLP's limits
int host_mlp(long long rows, int L, int H, int O, int activation, const float* x, const float* w1t, const float* b1,
             const float* w2, const float* b2, float* y, float* hidden_or_null) {
    if (!ccx_mlp::shape_ok(L, H, O, activation)) return -1;
    for (long long i = 0; i < rows; ++i)
        ccx_mlp::mlp_row(L, H, O, activation, x + i * L, w1t, b1, w2, b2, y + i * O, hidden_or_null ? hidden_or_null + i * H : nullptr);
    return 0;
}

// the LDS floats of a forward workgroup (`draw`: the fused kernels keep the tile's y); -1 for a shape outside CCX_MLP's limits
long long host_lds_floats(int L, int H, int O, int draw) {
    return ccx_mlp::shape_ok(L, H, O, ccx_mlp::kTanh) ? (long long)ccx_mlp::lds_floats(L, H, O, draw != 0) : -1;
}

void host_activations(long long n, const float* a, float* tanh_out, float* relu_out) {
    for (long long i = 0; i < n; ++i) {
        tanh_out[i] = ccx_mlp::tanh_spec(a[i]);
        relu_out[i] = ccx_mlp::relu_spec(a[i]);
    }
}

}  // extern "C"
