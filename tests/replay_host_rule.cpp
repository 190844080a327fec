// The rules of csrc/ccx_replay.h compiled for the host (tests/test_replay_host_rule.py: -O2 -ffp-contract=off), behind a C
// interface for ctypes.  The loops here only walk steps, envs and draws; every slot, every range and every index is one of
// ccx_replay.h's functions, and the word is ccx_kernels.h's formula restated in four lines (that header needs the HIP runtime).
#include "ccx_replay.h"

namespace {

uint32_t mix32(uint32_t k) {
    k ^= k >> 16; k *= 0x7FEB352Du; k ^= k >> 15; k *= 0x846CA68Bu; k ^= k >> 16;
    return k;
}
uint32_t random_word(uint32_t seed_lo, uint32_t seed_hi, uint32_t genv, uint32_t episode, uint32_t step, uint32_t agent) {
    const uint32_t k = genv * 0x9E3779B1u + episode * 0x85EBCA77u + step * 0xC2B2AE3Du + agent * 0x27D4EB2Fu + seed_lo;
    return mix32(mix32(k) ^ seed_hi);
}

}  // namespace

extern "C" {

// slots[s][e] of a block of K steps pushed at `head`
void host_replay_slots(long long head, long long K, long long S, long long E, long long* slots) {
    for (long long s = 0; s < K; ++s)
        for (long long e = 0; e < E; ++e) slots[s * E + e] = ccx_replay::slot_of(head, s, S, E, e);
}

unsigned long long host_replay_filled(long long head, long long S, long long E) { return ccx_replay::filled(head, S, E); }

// index[b], b = 0 .. B - 1, of launch d over F records
void host_replay_draw(unsigned long long seed, unsigned long long F, unsigned long long d, long long B, long long* index) {
    const uint32_t lo = (uint32_t)seed, hi = (uint32_t)(seed >> 32);
    for (long long b = 0; b < B; ++b) {
        const ccx_replay::Key k = ccx_replay::key_of((unsigned long long)b, d);
        const uint32_t w0 = random_word(lo, hi ^ ccx_replay::kStream, k.genv, k.episode, k.step, 0u);
        const uint32_t w1 = random_word(lo, hi ^ ccx_replay::kStream, k.genv, k.episode, k.step, 1u);
        index[b] = ccx_replay::index_of(w0, w1, F);
    }
}

unsigned long long host_replay_mulhi64(unsigned long long a, unsigned long long b) { return ccx_replay::mulhi64(a, b); }

int host_replay_in_ring(long long i, long long R) { return ccx_replay::in_ring(i, R) ? 1 : 0; }

// {action, done, valid, masks_next, masks_all, state words} of the empty record, and the bits of its reward
void host_replay_empty(long long* out) {
    out[0] = ccx_replay::kEmptyAction;
    out[1] = ccx_replay::kEmptyDone;
    out[2] = ccx_replay::kEmptyValid;
    out[3] = ccx_replay::kEmptyMasks;
    out[4] = ccx_replay::kMasksAll;
    out[5] = ccx_replay::kStateWords;
    const double r = ccx_replay::kEmptyReward;
    out[6] = __builtin_bit_cast(long long, r);
}

}  // extern "C"
