// The rule of csrc/ccx_adam.h compiled for the host (tests/test_adam_host_rule.py: -O2 -ffp-contract=off), behind a C interface
// for ctypes.  The loops here only walk blocks and places in the order the header states; every arithmetic operation
// is one of ccx_adam.h's or of ccx_tree.h's.
#include <vector>

#include "ccx_adam.h"

extern "C" {

// tab: T rows of {param, grad, m, v, numel} (host pointers); state: 64 bytes; stats: f32 [4]
void host_adam_step(int T, const ccx_adam::Tensor* tab, float lr, const float* lr_dev_or_null, float beta1, float beta2, float eps,
                    float weight_decay, float max_grad_norm, ccx_adam::State* state, float* stats) {
    // 1. the block partials of the padded sequence, then the final wave
    const long long B = ccx_adam::total_blocks(tab, T);
    std::vector<double> P(B);
    for (long long b = 0; b < B; ++b) {
        int t;
        long long bt;
        ccx_adam::locate(tab, T, b, t, bt);
        double v[ccx_adam::kBlockPlaces];
        for (int j = 0; j < ccx_adam::kBlockPlaces; ++j) {
            const long long place = bt * ccx_adam::kBlockPlaces + j;
            const bool exists = place < tab[t].numel;
            v[j] = ccx_adam::square_term(exists, tab[t].grad[exists ? place : tab[t].numel - 1]);
        }
        P[b] = ccx_tree::block_host(v, ccx_adam::kBlockPlaces);
    }
    const double S = ccx_tree::final_host(P.data(), B);
    // 2-4. the call's scalars and the state advance
    ccx_adam::Scalars sc{};
    float st[4];
    ccx_adam::finals(S, lr_dev_or_null ? lr_dev_or_null[0] : lr, beta1, beta2, weight_decay, max_grad_norm, *state, sc, st);
    for (int k = 0; k < 4; ++k) stats[k] = st[k];
    if (sc.skip) return;
    // 5. every element
    for (int t = 0; t < T; ++t)
        for (long long i = 0; i < tab[t].numel; ++i)
            ccx_adam::update_element(tab[t].grad[i], tab[t].param[i], tab[t].m[i], tab[t].v[i], sc, max_grad_norm > 0.0f,
                                     weight_decay != 0.0f, beta1, beta2, eps);
}

long long host_adam_blocks(int T, const ccx_adam::Tensor* tab) { return ccx_adam::total_blocks(tab, T); }

// the tensor and the block within it of every block of the sequence
void host_adam_locate(int T, const ccx_adam::Tensor* tab, int* tensor_of, long long* block_in_tensor) {
    const long long B = ccx_adam::total_blocks(tab, T);
    for (long long b = 0; b < B; ++b) ccx_adam::locate(tab, T, b, tensor_of[b], block_in_tensor[b]);
}

}  // extern "C"
