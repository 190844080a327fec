// The per-row rules of csrc/ccx_softmax.h compiled for the host (tests/test_evaluate_host_rule.py: -O2 -ffp-contract=off),
// behind a C interface for ctypes.  which_grads: bit 0 = grad_logp is given, bit 1 = grad_entropy is given.
#include "ccx_softmax.h"

extern "C" {

void host_evaluate(long long rows, const float* logits, const unsigned char* actions, const unsigned char* masks_or_null,
                   float* logp, float* entropy_or_null) {
    for (long long i = 0; i < rows; ++i) {
        float l[5], lp = 0.0f, ent = 0.0f;
        for (int k = 0; k < 5; ++k) l[k] = logits[i * 5 + k];
        const uint32_t mbyte = masks_or_null ? masks_or_null[i] : 0x1Fu;
        if (entropy_or_null) ccx_softmax::evaluate_row<true>(l, mbyte, actions[i], lp, ent);
        else ccx_softmax::evaluate_row<false>(l, mbyte, actions[i], lp, ent);
        logp[i] = lp;
        if (entropy_or_null) entropy_or_null[i] = ent;
    }
}

void host_evaluate_backward(long long rows, const float* logits, const unsigned char* actions, const unsigned char* masks_or_null,
                            const float* grad_logp_or_null, const float* grad_entropy_or_null, float* grad_logits) {
    for (long long i = 0; i < rows; ++i) {
        float l[5], g[5];
        for (int k = 0; k < 5; ++k) l[k] = logits[i * 5 + k];
        const uint32_t mbyte = masks_or_null ? masks_or_null[i] : 0x1Fu;
        const float glp = grad_logp_or_null ? grad_logp_or_null[i] : 0.0f;
        const float gent = grad_entropy_or_null ? grad_entropy_or_null[i] : 0.0f;
        if (grad_logp_or_null && grad_entropy_or_null) ccx_softmax::evaluate_row_backward<true, true>(l, mbyte, actions[i], glp, gent, g);
        else if (grad_logp_or_null) ccx_softmax::evaluate_row_backward<true, false>(l, mbyte, actions[i], glp, gent, g);
        else ccx_softmax::evaluate_row_backward<false, true>(l, mbyte, actions[i], glp, gent, g);
        for (int k = 0; k < 5; ++k) grad_logits[i * 5 + k] = g[k];
    }
}

// steps 2-6 of CCX_SAMPLE through the shared functions: legal u8 [rows][5], degenerate u8 [rows], d / w / c f32 [rows][5]
void host_steps_2_to_6(long long rows, const float* logits, const unsigned char* masks_or_null, unsigned char* legal_out,
                       unsigned char* degenerate_out, float* d_out, float* w_out, float* c_out) {
    for (long long i = 0; i < rows; ++i) {
        float l[5], mx, d[5], w[5], c[5];
        bool legal[5], degenerate;
        for (int k = 0; k < 5; ++k) l[k] = logits[i * 5 + k];
        const uint32_t m = ((masks_or_null ? masks_or_null[i] : 0x1Fu) & 0x1Fu) | 0x10u;
        ccx_softmax::legal_max_d(l, m, legal, mx, degenerate, d);
        ccx_softmax::weights(legal, d, w, c);
        degenerate_out[i] = degenerate;
        for (int k = 0; k < 5; ++k) {
            legal_out[i * 5 + k] = legal[k];
            d_out[i * 5 + k] = d[k];
            w_out[i * 5 + k] = w[k];
            c_out[i * 5 + k] = c[k];
        }
    }
}

}  // extern "C"
