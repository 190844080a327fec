// ccx_replay.h -- CCX_REPLAY (include/ccx.h) as inline functions: the slot a pushed (step, env) record lands in, the number of
// filled records, the record a draw picks from its two counter-based words, and the fields of the EMPTY record.  Included by
// ccx_replay.hip; it also compiles with a plain host C++ compiler (tests/test_replay_host_rule.py runs it against the spec of
// tests/_replay_spec.py as exact integers).  Everything here is integer work: there is no rounding to define.
// The words themselves are ccx_kernels.h's random_word (that header needs the HIP runtime; the host test restates its four
// lines): this header says which keys they are drawn at and what is made of them.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define CCX_RP_HD __host__ __device__ __forceinline__
#else
#define CCX_RP_HD inline
#endif

namespace ccx_replay {

constexpr uint32_t kStream = 0x3C6EF372u;                                 // ccx_kernels.h: kReplayStream (asserted equal there)

// the EMPTY record: what the ring holds before a slot is pushed, and what an index outside [0, R) fetches
constexpr uint8_t kEmptyAction = 255u, kEmptyDone = 0u, kEmptyValid = 0u, kEmptyMasks = 0x10u;
constexpr uint8_t kMasksAll = 0x1Fu;                                      // masks_next of a step that ended its episode
constexpr double kEmptyReward = 0.0;                                      // +0.0, as both compact arrays
constexpr int kStateWords = 4;                                            // state = {head, draws, 0, 0}, int64

// record slot of step s (0 <= s < K <= S) of a block pushed at `head`, env e: ((head + s) mod S) * E + e
CCX_RP_HD long long slot_of(long long head, long long s, long long S, long long E, long long e) {
    const long long at = (head + s) % S;                                  // head >= 0, s >= 0
    return at * E + e;
}

// F: records that have been pushed (the draw's range), min(head, S) * E
CCX_RP_HD unsigned long long filled(long long head, long long S, long long E) {
    const long long steps = head < S ? head : S;
    return (unsigned long long)steps * (unsigned long long)E;
}

// the six keys of draw b of launch d: word(seed_lo, seed_hi ^ kStream; b, d_lo, d_hi, which), which = 0 (high half), 1 (low)
struct Key { uint32_t genv, episode, step; };
CCX_RP_HD Key key_of(unsigned long long b, unsigned long long d) {
    return Key{(uint32_t)b, (uint32_t)d, (uint32_t)(d >> 32)};
}

// high 64 bits of a * b
CCX_RP_HD unsigned long long mulhi64(unsigned long long a, unsigned long long b) {
    const unsigned long long m = 0xFFFFFFFFull;
    const unsigned long long a0 = a & m, a1 = a >> 32, b0 = b & m, b1 = b >> 32;
    const unsigned long long p00 = a0 * b0, p01 = a0 * b1, p10 = a1 * b0, p11 = a1 * b1;
    const unsigned long long mid = (p00 >> 32) + (p01 & m) + (p10 & m);
    return p11 + (p01 >> 32) + (p10 >> 32) + (mid >> 32);
}

// index = F == 0 ? -1 : floor((w0 * 2^32 + w1) * F / 2^64): uniform over [0, F) up to F / 2^64
CCX_RP_HD long long index_of(uint32_t w0, uint32_t w1, unsigned long long F) {
    const unsigned long long x = ((unsigned long long)w0 << 32) | (unsigned long long)w1;
    const unsigned long long hi = mulhi64(x, F);
    return F == 0ull ? -1ll : (long long)hi;
}

// does record index i name a slot of a ring of R records?  (anything else fetches the empty record and reads nothing)
CCX_RP_HD bool in_ring(long long i, long long R) { return i >= 0 && i < R; }

}  // namespace ccx_replay
