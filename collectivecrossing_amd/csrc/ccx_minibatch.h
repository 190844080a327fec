// ccx_minibatch.h -- CCX_MINIBATCH (include/ccx.h) as inline functions: the keyed permutation of a rollout's M = K E records
// (an unbalanced Feistel network of six rounds with cycle walking: any lane computes pi_c(p) from p alone, nothing is
// materialised), which positions a draw covers, how the state {epoch, cursor} advances, where the observation row of a record
// lies, and the fields of the EMPTY row.  Included by ccx_minibatch.hip; it also compiles with a plain host C++ compiler
// (tests/test_minibatch_host_rule.py runs it against the spec of tests/_minibatch_spec.py as exact integers).  Everything here
// is integer work: there is no rounding to define.
// The round word is ccx_kernels.h's random_word (that header needs the HIP runtime): the network takes it as a callable
// `word(right, epoch_lo, epoch_hi, round)`, so the kernels pass the library's own and the host test its four restated lines.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define CCX_MB_HD __host__ __device__ __forceinline__
#else
#define CCX_MB_HD inline
#endif

namespace ccx_minibatch {

constexpr uint32_t kStream = 0x1B873593u;                                 // ccx_kernels.h: kMinibatchStream (asserted equal there)
constexpr int kRounds = 6;                                                // four left pi(p + 1) = pi(p) + 1 at 1.12-1.27 times chance
constexpr int kStateWords = 4;                                            // state = {epoch, cursor, 0, 0}, int64
constexpr long long kMaxRecords = (1ll << 31) - 1;                        // 1 <= M = K E < 2^31

// the EMPTY row: what an index outside [0, M) gathers (CCX_REPLAY's empty record where the two share a field)
constexpr uint8_t kEmptyAction = 255u, kEmptyValid = 0u, kEmptyMasks = 0x10u;
constexpr uint8_t kMasksAll = 0x1Fu, kValidLive = 4u;                     // what a record gets without a masks / valid source

// x = L 2^b + R: w = the smallest integer >= 2 with 2^w >= M, a = floor(w / 2) bits of L, b = w - a bits of R
struct Split { uint32_t w, a, b; };
CCX_MB_HD Split split_of(uint32_t M) {
    uint32_t w = 2u;
    while (w < 31u && (1u << w) < M) ++w;                                 // M < 2^31
    return Split{w, w >> 1, w - (w >> 1)};
}

// the six rounds: (L, R) <- (R, L ^ (word(R, c_lo, c_hi, r) & (2^wl - 1))), wl <- w - wl, with wl the width of L (a at the
// start, so (a, b) again at the end).  Each round is invertible: a bijection of [0, 2^w).
template <class Word>
CCX_MB_HD uint32_t rounds(uint32_t x, Split sp, uint32_t c_lo, uint32_t c_hi, Word word) {
    uint32_t L = x >> sp.b, R = x & ((1u << sp.b) - 1u), wl = sp.a;
    for (int r = 0; r < kRounds; ++r) {
        const uint32_t f = word(R, c_lo, c_hi, (uint32_t)r) & ((1u << wl) - 1u);
        const uint32_t l = R;
        R = L ^ f;
        L = l;
        wl = sp.w - wl;
    }
    return (L << sp.b) | R;
}

// pi_c(p), 0 <= p < M: the six rounds again while the image is >= M (cycle walking: p's cycle under the bijection of [0, 2^w)
// returns to [0, M), so the loop ends for every key; 2^w < 2 M, so a step succeeds with probability above 1 / 2)
struct Walked { uint32_t x, steps; };
template <class Word>
CCX_MB_HD Walked permute(uint32_t p, uint32_t M, Split sp, unsigned long long epoch, Word word) {
    const uint32_t c_lo = (uint32_t)epoch, c_hi = (uint32_t)(epoch >> 32);
    Walked v{p, 0u};
    do {
        v.x = rounds(v.x, sp, c_lo, c_hi, word);
        ++v.steps;
    } while (v.x >= M);
    return v;
}

// rounds 5 .. 0 undone (the tests' independent statement of invertibility; no kernel calls it)
template <class Word>
CCX_MB_HD uint32_t rounds_inverse(uint32_t y, Split sp, uint32_t c_lo, uint32_t c_hi, Word word) {
    uint32_t L = y >> sp.b, R = y & ((1u << sp.b) - 1u), wl = sp.a;        // (an even number of rounds: the widths are (a, b) here too)
    for (int r = kRounds - 1; r >= 0; --r) {
        wl = sp.w - wl;                                                   // the width L had BEFORE round r
        const uint32_t f = word(L, c_lo, c_hi, (uint32_t)r) & ((1u << wl) - 1u);
        const uint32_t right = L;
        L = R ^ f;
        R = right;
    }
    return (L << sp.b) | R;
}

// does row b of a draw of B rows at `cursor` take a position of the epoch?  p = cursor + b < M, without forming the sum:
// whatever the state holds (a junk cursor included) the answer names a position in [0, M) or none
CCX_MB_HD bool drawn(long long cursor, long long b, long long M) { return cursor >= 0 && cursor < M - b; }

// the state behind a draw of B rows: the next epoch once the cursor has covered [0, M)
struct State { long long epoch, cursor; };
CCX_MB_HD State advance(State s, long long B, long long M) {
    if (s.cursor < 0 || s.cursor >= M - B) {                              // cursor + B >= M, without forming the sum
        s.epoch = (long long)((unsigned long long)s.epoch + 1ull);
        s.cursor = 0;
    } else {
        s.cursor += B;
    }
    return s;
}

// does record index i name a record of a rollout of M?  (anything else gathers the EMPTY row and reads nothing)
CCX_MB_HD bool in_rollout(long long i, long long M) { return i >= 0 && i < M; }

// the observation the step of record j = s E + e ACTED ON: with obs0 given it is obs0[e] for s == 0 and obs_steps[s - 1][e]
// = record j - E of obs_steps otherwise (CCX_REPLAY's obs_c rule); without obs0 the caller's array holds it at j
struct RowAt { bool first; long long at; };
CCX_MB_HD RowAt row_of(long long j, long long E, bool has_obs0) {
    if (!has_obs0) return RowAt{false, j};
    return j < E ? RowAt{true, j} : RowAt{false, j - E};
}

// 8-byte unit t (0 <= t < N (3 + 2 N)) of the N DefaultObservation rows of a record whose compact records are +0.0
// (ccx_kernels.h: obs_unit_addr): 0 = (+0, +0), 1 = (door_centre, division_y), 2 = (door_left, door_right), 3 = (-1, -1)
CCX_MB_HD int empty_unit_kind(uint32_t t, uint32_t N) {
    const uint32_t U = 3u + 2u * N, row = t / U, u = t - row * U;
    if (u < 3u) return (int)u;
    return ((u - 3u) >> 1) == row ? 3 : 0;
}

}  // namespace ccx_minibatch
