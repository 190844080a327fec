// ccx_prio.h -- CCX_PRIO (include/ccx.h) as inline functions: the shape of the integer sum tree over the leaves, the
// fixed-point priority of a record from its TD errors, the 64-bit point a draw aims at (stratified or not), the descent from
// the top of the tree to a leaf, and the importance weight.  Included by ccx_prio.hip; it also compiles with a plain host C++
// compiler (tests/test_prio_host_rule.py runs it against the spec of tests/_prio_spec.py, integers exactly and f32 bit for
// bit).  The sums are integers: there is no rounding in the tree.  The two f32 rules (quantise, weight) are one operation a
// line, as ccx_softmax.h's; the units that include this are compiled with -ffp-contract=off and correctly rounded division.
// exp_spec and log_spec are ccx_softmax.h's, unchanged.  log_spec is documented there for [1, 5], but its code takes any
// positive normal float (exponent and mantissa are split exactly); this rule uses it on [2^-31, 2^15] -- x of an update lies
// in [2^-16, 2^15], r of a weight in [1 / (2^31 - 1), 1] -- and exp_spec on [-22, 11], inside its [-80, 80].
#pragma once
#include <stdint.h>

#include "ccx_replay.h"
#include "ccx_softmax.h"

namespace ccx_prio {

constexpr uint32_t kStream = 0x7F4A7C15u;                                 // ccx_kernels.h: kPrioStream (asserted equal there)
constexpr int kStateWords = 4;                                            // pstate = {max_leaf, draws, T, min_leaf}, int64
constexpr long long kOne = 65536;                                         // 1.0 in fixed point: 16 fractional bits
constexpr int kMaxTd = 8;                                                 // td_error arrays of one update

// ---------------------------------------------------------------- the tree (private: nothing observable depends on it)
// Level 0 is the leaves, n[0] = R; level l + 1 has n[l + 1] = ceil(n[l] / kFan) nodes, node i the sum of nodes kFan i ..
// kFan i + kFan - 1 of level l.  A workgroup of the block kernel takes kFan^2 nodes of an even level and writes the kFan
// nodes above them and the one above those, so the levels come in pairs: `launches` block launches build levels 1 .. 2
// launches, until at most kFan^2 nodes are left; the final workgroup sums those into level `top` = 2 launches + 1 (at most
// kFan nodes) and into T.  Levels 1 .. top live in ONE int64 array of 2 * nodes words: the sums of level l at off[l], the
// minima of the non-zero leaves below each node at nodes + off[l].
constexpr int kFan = 16;
constexpr int kMaxLevels = 8;                                             // R < 2^31, kFan = 16: top <= 7 (kFan = 4 in the host test: R small)

struct Shape {
    int top, launches;
    long long nodes;                                                      // all nodes of levels 1 .. top
    long long n[kMaxLevels], off[kMaxLevels];                             // off[0] is not used: the leaves are the caller's array
};

CCX_HD Shape shape_of(long long R, int fan) {
    Shape s{};
    s.n[0] = R;
    s.launches = 0;
    const long long block = (long long)fan * fan;
    int l = 0;
    long long at = 0;
    do {                                                                  // one block launch: two levels
        for (int k = 0; k < 2; ++k) {
            s.n[l + 1] = (s.n[l] + fan - 1) / fan;
            s.off[l + 1] = at;
            at += s.n[l + 1];
            ++l;
        }
        ++s.launches;
    } while (s.n[l] > block && l + 3 < kMaxLevels);
    s.n[l + 1] = (s.n[l] + fan - 1) / fan;                                // the final workgroup's level
    s.off[l + 1] = at;
    at += s.n[l + 1];
    s.top = l + 1;
    s.nodes = at;
    return s;
}

// int64 words of the tree array of R records
CCX_HD long long tree_words(long long R) { return R < 1 ? 0 : 2 * shape_of(R, kFan).nodes; }

// ---------------------------------------------------------------- the priority of a record (update)
// m: the maximum of |td| over the record's agents and arrays, from +0.0; a NaN never wins, +inf does
CCX_HD float td_max(float m, float td) {
    const float a = __builtin_fabsf(td);
    return a > m ? a : m;
}

// leaf value of a record whose largest |td| is m: p = x^alpha in fixed point, 1 <= leaf < 2^31
CCX_HD int quantise(float m, float alpha, float eps) {
    const float s = m + eps;
    const float lo = 0x1p-16f, hi = 0x1p+15f;
    const float x = s < lo ? lo : (s > hi ? hi : s);                      // (+inf: hi)
    const float lx = ccx_softmax::log_spec(x);
    const float e = alpha * lx;
    const float pw = ccx_softmax::exp_spec(e);
    const float p = alpha == 0.0f ? 1.0f : pw;
    const float f = __builtin_floorf(p * 65536.0f);
    const float top = 0x1.fffffep+30f;                                    // the largest f32 below 2^31
    const float c = f > top ? top : f;                                    // clamped in f32 BEFORE the cast
    const int q = (int)c;
    return q < 1 ? 1 : q;
}

// ---------------------------------------------------------------- the point of a draw
// stratified: floor((b 2^64 + x) / B), 0 <= b < B < 2^31, as two 64-by-32-bit divisions; else x = w0 2^32 + w1
CCX_HD unsigned long long point_of(uint32_t w0, uint32_t w1, unsigned long long b, unsigned long long B, bool stratified) {
    if (!stratified) return ((unsigned long long)w0 << 32) | (unsigned long long)w1;
    const unsigned long long t1 = (b << 32) | (unsigned long long)w0;
    const unsigned long long q1 = t1 / B, r1 = t1 % B;
    const unsigned long long t2 = (r1 << 32) | (unsigned long long)w1;
    const unsigned long long q2 = t2 / B;
    return (q1 << 32) | q2;
}

// ---------------------------------------------------------------- the descent
// the smallest i with leaf[0] + .. + leaf[i] > u, for 0 <= u < T (T == 0: -1).  At every level the walk stays inside the
// children of the node it came from, and inside the level: parent == sum of children exactly, so it ends before either.
CCX_HD long long descend(const int* leaf, const long long* tree, const Shape& s, int fan, unsigned long long u, unsigned long long T) {
    if (T == 0ull) return -1;
    long long node = 0;
    unsigned long long rem = u;
    for (int l = s.top; l >= 0; --l) {
        const long long first = l == s.top ? 0 : node * fan;
        long long last = l == s.top ? s.n[l] - 1 : first + fan - 1;          // (the top level is one group, whatever its size)
        last = last < s.n[l] - 1 ? last : s.n[l] - 1;
        long long c = first;
        for (; c < last; ++c) {
            const unsigned long long v = l ? (unsigned long long)tree[s.off[l] + c] : (unsigned long long)(long long)leaf[c];
            if (rem < v) break;
            rem -= v;
        }
        node = c;
    }
    return node;
}

// ---------------------------------------------------------------- the importance weight
// (p_min / p_i)^beta: 1.0 exactly where the drawn leaf is the smallest; +0.0 where nothing was drawn
CCX_HD float weight(long long min_leaf, int leaf_drawn, float beta, bool drawn) {
    const float bt = beta < 0.0f ? 0.0f : (beta > 1.0f ? 1.0f : beta);
    const float r = (float)((double)min_leaf / (double)(drawn ? leaf_drawn : 1));
    const float lr = ccx_softmax::log_spec(drawn ? r : 1.0f);
    const float e = bt * lr;
    const float w = ccx_softmax::exp_spec(e);
    return drawn ? w : 0.0f;
}

}  // namespace ccx_prio
