// The rules of csrc/ccx_minibatch.h compiled for the host as a program of its own (tests/test_minibatch_host_rule.py builds it
// with -fsanitize=address,undefined and runs it; it is never loaded into Python).  It prints, as integers, what the test
// compares with tests/_minibatch_spec.py: permutations with their walk lengths, the inverse network's check, and sequences of
// draws with the state behind each.  The word is ccx_kernels.h's random_word, whose four lines are restated here (that header
// needs the HIP runtime); everything else is the header's own functions.
//   perm <seed> <M> <epoch>: pi(0) .. pi(M - 1)          walk <seed> <M> <epoch>: the walk lengths
//   draw <seed> <M> <B> <epoch> <cursor>: index[0 .. B)   then   state <epoch> <cursor>
#include <cinttypes>
#include <cstdio>
#include <vector>

#include "ccx_minibatch.h"

namespace {

uint32_t mix32(uint32_t k) {
    k ^= k >> 16; k *= 0x7FEB352Du; k ^= k >> 15; k *= 0x846CA68Bu; k ^= k >> 16;
    return k;
}
uint32_t random_word(uint32_t seed_lo, uint32_t seed_hi, uint32_t genv, uint32_t episode, uint32_t step, uint32_t agent) {
    const uint32_t k = genv * 0x9E3779B1u + episode * 0x85EBCA77u + step * 0xC2B2AE3Du + agent * 0x27D4EB2Fu + seed_lo;
    return mix32(mix32(k) ^ seed_hi);
}

struct Word {
    uint32_t lo, hi;
    uint32_t operator()(uint32_t right, uint32_t c_lo, uint32_t c_hi, uint32_t r) const {
        return random_word(lo, hi ^ ccx_minibatch::kStream, right, c_lo, c_hi, r);
    }
};

const uint64_t kSeeds[] = {2024ull, 0x0123456789ABCDEFull};
const uint32_t kM[] = {1, 2, 3, 4, 5, 6, 7, 8, 9, 15, 16, 17, 33, 63, 64, 65, 129, 255, 256, 257, 513, 1000, 1023, 1025, 2049, 4097,
                       65537, 131073, 262145};
const uint64_t kEpochs[] = {0ull, 1ull, 1ull << 32, (1ull << 40) + 7ull};

}  // namespace

int main() {
    uint32_t longest = 0;
    for (const uint64_t seed : kSeeds) {
        const Word word{(uint32_t)seed, (uint32_t)(seed >> 32)};
        for (const uint32_t M : kM) {
            const ccx_minibatch::Split sp = ccx_minibatch::split_of(M);
            if (sp.a + sp.b != sp.w || (1ull << sp.w) < M || (M > 2 && (1ull << (sp.w - 1)) >= M)) {
                std::printf("bad split at M %u\n", M);
                return 1;
            }
            for (const uint64_t epoch : kEpochs) {
                if (M > 4097 && (epoch == 1ull || seed != kSeeds[0])) continue;      // (the long ones once per epoch width)
                std::vector<uint32_t> pi(M), steps(M);                   // exactly M entries: the sanitizer sees a stray index
                std::vector<uint8_t> hit(M, 0);
                for (uint32_t p = 0; p < M; ++p) {
                    const ccx_minibatch::Walked v = ccx_minibatch::permute(p, M, sp, epoch, word);
                    pi[p] = v.x;
                    steps[p] = v.steps;
                    hit[v.x] += 1;
                    longest = v.steps > longest ? v.steps : longest;
                }
                for (uint32_t x = 0; x < M; ++x)
                    if (hit[x] != 1) {
                        std::printf("not a bijection at M %u: %u hit %u times\n", M, x, (unsigned)hit[x]);
                        return 1;
                    }
                const uint32_t top = sp.w < 12 ? (1u << sp.w) : 4096u;     // the inverse network over (a prefix of) [0, 2^w)
                for (uint32_t x = 0; x < top; ++x) {
                    const uint32_t y = ccx_minibatch::rounds(x, sp, (uint32_t)epoch, (uint32_t)(epoch >> 32), word);
                    if (y >> sp.w || ccx_minibatch::rounds_inverse(y, sp, (uint32_t)epoch, (uint32_t)(epoch >> 32), word) != x) {
                        std::printf("the inverse network fails at M %u x %u\n", M, x);
                        return 1;
                    }
                }
                std::printf("perm %" PRIu64 " %u %" PRIu64 ":", seed, M, epoch);
                for (uint32_t p = 0; p < M; ++p) std::printf(" %u", pi[p]);
                std::printf("\nwalk %" PRIu64 " %u %" PRIu64 ":", seed, M, epoch);
                for (uint32_t p = 0; p < M; ++p) std::printf(" %u", steps[p]);
                std::printf("\n");
            }
        }
        // draws: two and a half epochs from the start, then states outside their range
        const long long cases[][2] = {{15, 4}, {15, 15}, {15, 16}, {16, 4}, {1, 1}, {1, 3}, {1000, 64}};
        for (const auto& c : cases) {
            const long long M = c[0], B = c[1];
            const ccx_minibatch::Split sp = ccx_minibatch::split_of((uint32_t)M);
            const long long per_epoch = (M + B - 1) / B;
            const long long junk[][2] = {{7, -1}, {7, INT64_MIN}, {7, M}, {7, M + 1}, {7, INT64_MAX}, {-1, 0}, {INT64_MAX, M - 1}};
            ccx_minibatch::State s{0, 0};
            for (long long d = 0; d < (5 * per_epoch + 1) / 2 + 7; ++d) {
                if (d >= (5 * per_epoch + 1) / 2) {
                    const long long* j = junk[d - (5 * per_epoch + 1) / 2];
                    s = ccx_minibatch::State{j[0], j[1]};
                }
                std::vector<long long> index(B);
                for (long long b = 0; b < B; ++b)
                    index[b] = ccx_minibatch::drawn(s.cursor, b, M)
                                   ? (long long)ccx_minibatch::permute((uint32_t)(s.cursor + b), (uint32_t)M, sp, (unsigned long long)s.epoch, word).x
                                   : -1ll;
                std::printf("draw %" PRIu64 " %lld %lld %lld %lld:", seed, M, B, s.epoch, s.cursor);
                for (long long b = 0; b < B; ++b) {
                    if (index[b] != -1 && !ccx_minibatch::in_rollout(index[b], M)) return 1;
                    std::printf(" %lld", index[b]);
                }
                s = ccx_minibatch::advance(s, B, M);
                std::printf("\nstate %lld %lld\n", s.epoch, s.cursor);
            }
        }
    }
    // where a record's row lies, and the kinds of the EMPTY row's units
    for (long long E = 1; E <= 5; E += 2)
        for (long long j = 0; j < 3 * E; ++j) {
            const ccx_minibatch::RowAt with = ccx_minibatch::row_of(j, E, true), without = ccx_minibatch::row_of(j, E, false);
            std::printf("row %lld %lld: %d %lld %d %lld\n", E, j, (int)with.first, with.at, (int)without.first, without.at);
        }
    for (uint32_t N = 1; N <= 4; ++N) {
        std::printf("empty %u:", N);
        for (uint32_t t = 0; t < N * (3u + 2u * N); ++t) std::printf(" %d", ccx_minibatch::empty_unit_kind(t, N));
        std::printf("\n");
    }
    std::printf("longest walk %u\n", longest);
    return 0;
}
