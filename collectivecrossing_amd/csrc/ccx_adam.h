// ccx_adam.h -- CCX_ADAM (include/ccx.h) as inline functions: where a block of the padded sequence lies, the per-call
// scalars with the state advance (norm, skip, clip scale, bias corrections), and the per-element update.  The pieces of the
// f64 tree are ccx_tree.h's, called, not restated.  Included by ccx_adam.hip; it
// also compiles with a plain host C++ compiler (tests/test_adam_host_rule.py runs it against the NumPy spec bit for bit).
// The discipline is ccx_softmax.h's: every line is ONE operation of the stated type, the including units are compiled with
// -ffp-contract=off, `/` and sqrt are the correctly rounded ones, and a choice is a select, never a multiplication by zero.
#pragma once
#include "ccx_tree.h"

namespace ccx_adam {

constexpr int kMaxTensors = 32;                                           // CCX_ADAM_MAX_TENSORS
constexpr int kBlockPlaces = ccx_tree::kBlockRows;                         // a block of the sequence: 256 places of ONE tensor
constexpr float kNormEps = 1e-6f;                                         // den = gn + 1e-6f

// one row of the table: ccx_adam_tensor's layout (40 bytes)
struct Tensor {
    float* param;
    const float* grad;
    float* m;
    float* v;
    long long numel;
};

// the 64 bytes of `state`
struct State {
    double pow1, pow2;                                                    // beta1^step, beta2^step as running f64 products
    long long step, skipped;
    long long reserved[4];
};

// what the final wave leaves for the update launch (the head of the workspace, 64 bytes)
struct Scalars {
    float gn, scale, lr, lrwd, bc1, bc2, omb1, omb2;
    uint32_t skip;
    uint32_t pad[7];
};

constexpr long long kScalarBytes = (long long)sizeof(Scalars);

// blocks of one tensor: each tensor is padded to a multiple of 256 places
CCX_HD long long blocks_of(long long numel) { return ccx_tree::blocks_of(numel); }

// B of the whole table
CCX_HD long long total_blocks(const Tensor* tab, int T) {
    long long B = 0;
    for (int k = 0; k < T; ++k) B += blocks_of(tab[k].numel);
    return B;
}

// Block b of the sequence (0 <= b < B): its tensor t and its index within that tensor.  A scan of the T prefix counts; b is
// uniform over a workgroup, so on the device this is scalar work.
CCX_HD void locate(const Tensor* tab, int T, long long b, int& t, long long& block_in_tensor) {
    long long first = 0;
    t = 0;
    block_in_tensor = b;
    for (int k = 0; k < T; ++k) {
        if (b >= first) {
            t = k;
            block_in_tensor = b - first;
        }
        first += blocks_of(tab[k].numel);
    }
}

// a place's term of the sum of squares: the exact f64 product (48 significant bits at most); a padding place is +0.0
CCX_HD double square_term(bool exists, float g) {
    const double d = (double)g;
    const double dd = d * d;
    return exists ? dd : 0.0;
}

// Steps 2-4: from the sum S to the call's scalars and `stats`; `st` is advanced (or, on a skip, only st.skipped).
// lr is the rate in force (the by-value argument or lr_dev[0]).
CCX_HD void finals(double S, float lr, float beta1, float beta2, float weight_decay, float max_grad_norm, State& st, Scalars& sc,
                   float (&stats)[4]) {
    const double nd = __builtin_sqrt(S);
    const float gn = (float)nd;
    const bool skip = gn != gn || gn == __builtin_inff();
    float scale = 1.0f;
    if (max_grad_norm > 0.0f) {
        const float den = gn + kNormEps;
        const float c = max_grad_norm / den;
        scale = c < 1.0f ? c : 1.0f;
    }
    if (skip) {
        st.skipped = st.skipped + 1;
    } else {
        st.pow1 = st.pow1 * (double)beta1;
        st.pow2 = st.pow2 * (double)beta2;
        st.step = st.step + 1;
    }
    const double c1 = 1.0 - st.pow1;
    const double c2 = 1.0 - st.pow2;
    const double o1 = 1.0 - (double)beta1;
    const double o2 = 1.0 - (double)beta2;
    sc.gn = gn;
    sc.scale = scale;
    sc.lr = lr;
    sc.lrwd = lr * weight_decay;
    sc.bc1 = (float)c1;
    sc.bc2 = (float)c2;
    sc.omb1 = (float)o1;
    sc.omb2 = (float)o2;
    sc.skip = skip ? 1u : 0u;
    stats[0] = gn;
    stats[1] = scale;
    stats[2] = skip ? 1.0f : 0.0f;
    stats[3] = lr;
}

// Step 5 for one element of a step that is not skipped.
CCX_HD void update_element(float g, float& p, float& m, float& v, const Scalars& sc, bool has_clip, bool has_decay, float beta1,
                           float beta2, float eps) {
    const float gc = g * sc.scale;
    const float gs = has_clip ? gc : g;
    const float pl = p * sc.lrwd;
    const float ps = p - pl;
    const float pd = has_decay ? ps : p;
    const float m1 = beta1 * m;
    const float m2 = sc.omb1 * gs;
    const float mn = m1 + m2;
    const float gg = gs * gs;
    const float v1 = beta2 * v;
    const float v2 = sc.omb2 * gg;
    const float vn = v1 + v2;
    const float mh = mn / sc.bc1;
    const float vh = vn / sc.bc2;
    const float sq = __builtin_sqrtf(vh);
    const float dn = sq + eps;
    const float u = mh / dn;
    const float lu = sc.lr * u;
    p = pd - lu;
    m = mn;
    v = vn;
}

}  // namespace ccx_adam
