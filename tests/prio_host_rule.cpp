// The rules of csrc/ccx_prio.h compiled for the host (tests/test_prio_host_rule.py: -O2 -ffp-contract=off), behind a C
// interface for ctypes.  The tree is built here by plain loops from the header's shape (sums and minima of the children,
// level by level) at whatever fan-out the test asks for; the descent, the point, the quantisation and the weight are the
// header's functions.
#include <vector>

#include "ccx_prio.h"

extern "C" {

// {top, launches, nodes, n[0..7], off[0..7]} of shape_of(R, fan)
void host_prio_shape(long long R, int fan, long long* out) {
    const ccx_prio::Shape s = ccx_prio::shape_of(R, fan);
    out[0] = s.top;
    out[1] = s.launches;
    out[2] = s.nodes;
    for (int l = 0; l < ccx_prio::kMaxLevels; ++l) {
        out[3 + l] = s.n[l];
        out[3 + ccx_prio::kMaxLevels + l] = s.off[l];
    }
}

long long host_prio_tree_words(long long R) { return ccx_prio::tree_words(R); }
int host_prio_fan() { return ccx_prio::kFan; }

// index[k] = descend(u[k]) over a tree of fan-out `fan` built from leaf[0..R); returns T, *min_out the smallest non-zero leaf
unsigned long long host_prio_descend(const int* leaf, long long R, int fan, const unsigned long long* u, long long count,
                                     long long* index, long long* min_out) {
    const ccx_prio::Shape s = ccx_prio::shape_of(R, fan);
    std::vector<long long> tree(2 * s.nodes, -1);
    for (int l = 1; l <= s.top; ++l)
        for (long long i = 0; i < s.n[l]; ++i) {
            long long sum = 0, mn = 0;
            for (long long c = i * fan; c < (i + 1) * fan && c < s.n[l - 1]; ++c) {
                const long long v = l == 1 ? (long long)leaf[c] : tree[s.off[l - 1] + c];
                const long long m = l == 1 ? (long long)leaf[c] : tree[s.nodes + s.off[l - 1] + c];
                sum += v;
                mn = mn == 0 ? m : (m == 0 ? mn : (m < mn ? m : mn));
            }
            tree[s.off[l] + i] = sum;
            tree[s.nodes + s.off[l] + i] = mn;
        }
    unsigned long long T = 0;
    long long mn = 0;
    for (long long i = 0; i < s.n[s.top]; ++i) {
        const long long m = tree[s.nodes + s.off[s.top] + i];
        T += (unsigned long long)tree[s.off[s.top] + i];
        mn = mn == 0 ? m : (m == 0 ? mn : (m < mn ? m : mn));
    }
    *min_out = mn;
    for (long long k = 0; k < count; ++k) index[k] = ccx_prio::descend(leaf, tree.data(), s, fan, u[k], T);
    return T;
}

unsigned long long host_prio_point(uint32_t w0, uint32_t w1, unsigned long long b, unsigned long long B, int stratified) {
    return ccx_prio::point_of(w0, w1, b, B, stratified != 0);
}

// leaf[b] from count arrays td[a][b][n]
void host_prio_quantise(const float* const* td, int count, long long B, int N, float alpha, float eps, int* leaf) {
    for (long long b = 0; b < B; ++b) {
        float m = 0.0f;
        for (int a = 0; a < count; ++a)
            for (int n = 0; n < N; ++n) m = ccx_prio::td_max(m, td[a][b * N + n]);
        leaf[b] = ccx_prio::quantise(m, alpha, eps);
    }
}

void host_prio_weight(long long min_leaf, const int* leaf_drawn, long long B, float beta, float* w) {
    for (long long b = 0; b < B; ++b) w[b] = ccx_prio::weight(min_leaf, leaf_drawn[b], beta, leaf_drawn[b] > 0);
}

}  // extern "C"
