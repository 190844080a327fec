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

// the launch shape of the blocks kernels: the rows of a sub-tile and the dynamic LDS bytes of a workgroup (`per_row`: 0 for
// ccx_mlp_backward, 8 for ccx_sides_backward), and grid.y; -1 / 0 for a shape outside CCX_MLP's limits
int host_sub_rows(int L, int H, int O, int per_row, long long* bytes) {
    if (!ccx_mlp::shape_ok(L, H, O, ccx_mlp::kTanh) || per_row < 0) return -1;
    size_t b = 0;
    const int R = ccx_mlp_grad::sub_rows(L, H, O, b, (size_t)per_row);
    *bytes = (long long)b;
    return R;
}

int host_grad_grid_y(int L, int H, int O) {
    return ccx_mlp::shape_ok(L, H, O, ccx_mlp::kTanh) ? (int)ccx_mlp_grad::grid_y(L, H, O) : 0;
}

}  // extern "C"
