// ccx_c51.h -- CCX_C51 (include/ccx.h) as inline functions: the support, the distribution of one (row, action) over A atoms
// (the masked-softmax pattern of ccx_softmax.h over atoms instead of actions), its expected value (ONE function, shared by
// ccx_c51_q_values and the bootstrap choice inside the loss, as `greedy` is in CCX_QLEARN), the target projection in gather
// form, the cross-entropy of a row and its gradient.  exp_spec / log_spec are ccx_softmax.h's, greedy / legal_set / the
// counting rule / the final values are ccx_qlearn.h's, the f64 tree is ccx_tree.h's: called, not restated.
// The per-place functions are CCX_HD; the sums over a row's 64 places exist twice, as ccx_tree.h's do: in array form for
// the host (tests/test_c51_host_rule.py runs the host build against the NumPy spec bit for bit) and as wave butterflies for
// the device.  The discipline is ccx_softmax.h's: every line is ONE operation of the stated type, the including units are
// compiled with -ffp-contract=off, `/` is the correctly rounded division, and what a rule does not read is SELECTED away
// before any arithmetic, never multiplied by zero.
#pragma once
#include "ccx_qlearn.h"

namespace ccx_c51 {

constexpr int kMaxAtoms = 64, kMinAtoms = 2;
constexpr int kSums = ccx_qlearn::kSums;                                  // count, term, ce, qa, y, bad

// ---- the support: dz = (vmax - vmin) / (float)(A - 1);  z_j = vmin + (float)j * dz
CCX_HD float atom_gap(float vmin, float vmax, int A) {
    const float span = vmax - vmin;
    const float den = (float)(A - 1);
    return span / den;
}
CCX_HD float atom_value(float vmin, float dz, int j) {
    const float fj = (float)j;
    const float s = fj * dz;
    return vmin + s;
}

// ---- the maximum of two places: NaN-ignoring (a NaN beside a number gives the number, two NaNs a NaN) and with zeros of
// either sign made +0.0, so that it is symmetric in its arguments bit for bit and the butterfly gives every lane the same.
CCX_HD float max2(float a, float b) {
    const float m = __builtin_fmaxf(a, b);
    return m == 0.0f ? 0.0f : m;
}

// ---- step 1, one place: d = l - mx;  u = d - d (+0.0 for a finite d, NaN for an infinite one or a NaN);
// e = d >= -80 ? exp_spec(d) : u.  A logit far below the maximum weighs exactly +0.0; a NaN, a +inf and a -inf logit all put
// a NaN into S: every logit that is read must be finite, and one that is not is loud.  Places j >= A hold +0.0.
CCX_HD float atom_weight(float l, float mx, bool live, float& d) {
    d = l - mx;
    const float u = d - d;
    const bool in = d >= ccx_softmax::kDMin;
    const float x = in ? d : 0.0f;                                        // (exp_spec sees [-80, 0] only)
    const float ex = ccx_softmax::exp_spec(x);
    const float e = in ? ex : u;
    return live ? e : 0.0f;
}

// log S, S in [1, 64] or NaN (log_spec works on the bits: a NaN is selected past it)
CCX_HD float log_sum(float S) {
    const float ls = ccx_softmax::log_spec(S);
    return S != S ? S : ls;
}

// ---- step 2, one place of T = sum(e_j * z_j); the expected value is T / S
CCX_HD float expected_place(float e, float z, bool live) {
    const float ez = e * z;
    return live ? ez : 0.0f;
}
CCX_HD float expected_value(float T, float S) { return T / S; }

// ---- step 4.  cut = done || disc == 0: nothing of the next state is read; the target is the point mass at r, stated as
// p_0 = 1, p_j = +0.0 (j > 0) so that ONE projection rule serves both.
CCX_HD bool target_cut(bool done, float disc) { return done || disc == 0.0f; }
CCX_HD float target_mass(float e, float S, bool cut, int j) {
    const float q = e / S;
    const float point = j == 0 ? 1.0f : 0.0f;
    return cut ? point : q;
}
// b_j: the position of t_j on the support in units of dz, limited to [0, top] by two selects.  u = t - t is +0.0 for a finite
// t and NaN otherwise; the selects hand u (top + u) out instead of the bare limit, so that an infinite or NaN reward or
// discount is not clamped into the support: it goes through loudly.
CCX_HD float target_place(float r, float disc, bool cut, float z, float vmin, float dz, float top) {
    const float gz = disc * z;
    const float tz = r + gz;
    const float t = cut ? r : tz;
    const float u = t - t;
    const float tv = t - vmin;
    const float b0 = tv / dz;
    const float b1 = b0 < 0.0f ? u : b0;
    const float tu = top + u;
    return b1 > top ? tu : b1;
}
// w_ij = max(+0.0f, 1 - |b_j - i|) as a select that a NaN passes (the comparison is false)
CCX_HD float hat(float b, float fi) {
    const float a = b - fi;
    const float ab = __builtin_fabsf(a);
    const float om = 1.0f - ab;
    return om < 0.0f ? 0.0f : om;
}
// one step of m_i = sum over j ascending of p_j * w_ij, onto +0.0f
CCX_HD float project_add(float m, float p, float b, float fi) {
    const float w = hat(b, fi);
    const float pw = p * w;
    return m + pw;
}

// ---- step 5, one place: logp_i = d_i - log S;  c_i = m_i != 0 ? m_i * logp_i : +0.0f  (ce = 0.0f - sum c_i);  m_i * z_i
CCX_HD float ce_place(float m, float d, float lS, bool live) {
    const float logp = d - lS;
    const float prod = m * logp;
    const float c = m != 0.0f ? prod : 0.0f;
    return live ? c : 0.0f;
}
CCX_HD float ce_of(float csum) { return 0.0f - csum; }
CCX_HD float weighted(bool has_w, float w, float ce) {
    const float wc = w * ce;
    return has_w ? wc : ce;
}
CCX_HD float mean_place(float m, float z, bool live) {
    const float mz = m * z;
    return live ? mz : 0.0f;
}
CCX_HD float live_or_zero(float m, bool live) { return live ? m : 0.0f; }

// ---- step 7, one place: gw * ((e_j / S) * Msum - m_j)
CCX_HD float grad_place(float e, float S, float Msum, float m, float gw) {
    const float p = e / S;
    const float pm = p * Msum;
    const float df = pm - m;
    return gw * df;
}

// ---- the sums over a row's 64 places, host form: the halving butterfly of ccx_tree.h in f32 (offsets 32, 16, .. 1; every
// place ends with the same bits), and the same butterfly with max2
inline float halve64f(const float* v) {
    float s[64], t[64];
    for (int j = 0; j < 64; ++j) s[j] = v[j];
    for (int o = 32; o >= 1; o >>= 1) {
        for (int j = 0; j < 64; ++j) t[j] = s[j] + s[j ^ o];
        for (int j = 0; j < 64; ++j) s[j] = t[j];
    }
    return s[0];
}
inline float max64(const float* v) {
    float s[64], t[64];
    for (int j = 0; j < 64; ++j) s[j] = v[j];
    for (int o = 32; o >= 1; o >>= 1) {
        for (int j = 0; j < 64; ++j) t[j] = max2(s[j], s[j ^ o]);
        for (int j = 0; j < 64; ++j) s[j] = t[j];
    }
    return s[0];
}

struct Support {
    int A;
    float vmin, dz, top;
};
CCX_HD Support support_of(int A, float vmin, float vmax) { return Support{A, vmin, atom_gap(vmin, vmax, A), (float)(A - 1)}; }

// the distribution of one (row, action) on the host: l = its A logits
struct DistHost {
    float d[64], e[64], S;
};
inline void dist_host(const float* l, int A, DistHost& D) {
    float v[64];
    for (int j = 0; j < 64; ++j) v[j] = j < A ? l[j] : -__builtin_inff();
    const float mx = max64(v);
    for (int j = 0; j < 64; ++j) D.e[j] = atom_weight(v[j], mx, j < A, D.d[j]);
    D.S = halve64f(D.e);
}
// THE expected value on the host
inline float expected_host(const DistHost& D, const Support& Z) {
    float v[64];
    for (int j = 0; j < 64; ++j) v[j] = expected_place(D.e[j], atom_value(Z.vmin, Z.dz, j), j < Z.A);
    return expected_value(halve64f(v), D.S);
}

struct RowHost {
    float ce, term, qa, y;
    uint32_t kstar;
};
// Steps 1-5 of one row that counts.  la: logits[i][a] (A floats); nt / nsel: next_target[i] and what chooses the bootstrap
// action (next_online[i] for double-Q, else nt), [5][A] each, not read where the target is cut; m: A floats out.
inline void forward_row_host(const Support& Z, const float* la, float r, bool done, float disc, const float* nt, const float* nsel,
                             uint32_t mbyte_next, bool has_w, float w, float* m, RowHost& t) {
    const int A = Z.A;
    const bool cut = target_cut(done, disc);
    DistHost P{};
    P.S = 1.0f;                                                           // (a cut target reads neither)
    t.kstar = 4u;
    if (!cut) {
        float q[5];
        for (int k = 0; k < 5; ++k) {
            dist_host(nsel + k * A, A, P);
            q[k] = expected_host(P, Z);
        }
        t.kstar = ccx_qlearn::greedy(q, ccx_qlearn::legal_set(mbyte_next));
        dist_host(nt + t.kstar * A, A, P);
    }
    float p[64], b[64], mm[64], v[64];
    for (int j = 0; j < A; ++j) {
        p[j] = target_mass(P.e[j], P.S, cut, j);
        b[j] = target_place(r, disc, cut, atom_value(Z.vmin, Z.dz, j), Z.vmin, Z.dz, Z.top);
    }
    for (int i = 0; i < 64; ++i) {
        float acc = 0.0f;
        for (int j = 0; j < A; ++j) acc = project_add(acc, p[j], b[j], (float)i);
        mm[i] = acc;
    }
    DistHost D;
    dist_host(la, A, D);
    const float lS = log_sum(D.S);
    for (int i = 0; i < 64; ++i) v[i] = ce_place(mm[i], D.d[i], lS, i < A);
    t.ce = ce_of(halve64f(v));
    t.term = weighted(has_w, w, t.ce);
    t.qa = expected_host(D, Z);
    for (int i = 0; i < 64; ++i) v[i] = mean_place(mm[i], atom_value(Z.vmin, Z.dz, i), i < A);
    t.y = halve64f(v);
    for (int i = 0; i < A; ++i) m[i] = mm[i];
}
// Step 7 of one row that counts: g = A gradients at the stored action
inline void backward_row_host(int A, const float* la, const float* m, float gw, float* g) {
    DistHost D;
    dist_host(la, A, D);
    float v[64];
    for (int i = 0; i < 64; ++i) v[i] = live_or_zero(i < A ? m[i] : 0.0f, i < A);
    const float Msum = halve64f(v);
    for (int i = 0; i < A; ++i) g[i] = grad_place(D.e[i], D.S, Msum, m[i], gw);
}

#if defined(__HIPCC__)
// ---- the same sums on the device: a lane is a place, f32 addition and max2 commute, so all lanes agree
__device__ __forceinline__ float wave_sum(float s) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) s = s + __shfl_xor(s, o, 64);
    return s;
}
__device__ __forceinline__ float wave_max(float s) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) s = max2(s, __shfl_xor(s, o, 64));
    return s;
}
struct Dist {
    float d, e, S;
};
// l: the A contiguous logits of one (row, action); lanes >= A load nothing
__device__ __forceinline__ Dist wave_dist(const float* l, uint32_t lane, int A) {
    const bool live = lane < (uint32_t)A;
    float v = -__builtin_inff();
    if (live) v = l[lane];
    const float mx = wave_max(v);
    Dist D;
    D.e = atom_weight(v, mx, live, D.d);
    D.S = wave_sum(D.e);
    return D;
}
// THE expected value on the device (z: the lane's atom)
__device__ __forceinline__ float wave_expected(const Dist& D, float z, bool live) {
    return expected_value(wave_sum(expected_place(D.e, z, live)), D.S);
}
#endif

}  // namespace ccx_c51
