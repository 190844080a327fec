// The backward rule of csrc/ccx_mlp_grad.h compiled for the host (tests/test_mlp_backward_host_rule.py: -O2
// -ffp-contract=off), behind a C interface for ctypes.
#include "ccx_mlp_grad.h"

#include <vector>

extern "C" {

long long host_mlp_backward_workspace_bytes(long long rows, int L, int H, int O) {
    return ccx_mlp_grad::workspace_bytes(rows, L, H, O);
}

// the four gradients and ga f32 [rows][H]; returns 0, or -1 for rows < 1 or a shape outside CCX_MLP's limits
int host_mlp_backward(long long rows, int L, int H, int O, int activation, const float* x, const float* hidden, const float* grad_y,
                      const float* w2, float* grad_w1t, float* grad_b1, float* grad_w2, float* grad_b2, float* ga) {
    if (rows < 1 || !ccx_mlp::shape_ok(L, H, O, activation)) return -1;
    std::vector<double> ws((size_t)(ccx_mlp_grad::workspace_bytes(rows, L, H, O) / (long long)sizeof(double)), -7.0);
    ccx_mlp_grad::backward_host(rows, L, H, O, activation, x, hidden, grad_y, w2, ws.data(), grad_w1t, grad_b1, grad_w2, grad_b2, ga);
    return 0;
}

}  // extern "C"
