// ccx_tree.h -- the fixed f64 reduction tree of every bit-defined learner op (CCX_PPO_LOSS and the masked moments, CCX_MLP's
// backward, CCX_ADAM's global norm, CCX_QLEARN's TD loss, CCX_C51's categorical loss; the three losses through ccx_loss.h,
// which states what stands around their per-row rules), stated ONCE for the host and the device.  A group of 64 consecutive
// terms is halved by a butterfly; the four groups of a block of 256 are added into the block's partial; a final wave adds the
// B partials lane-strided in ascending order onto 64 places, and a last butterfly gives the sum.  The tree is fixed by the
// number of terms alone.  This header includes no rule: a unit that only sums takes it without ccx_softmax.h or ccx_ppo.h.
// It compiles with a plain host C++ compiler (tests/test_tree_host.py compiles it by itself and runs sum_host against the
// NumPy spec bit for bit).  The discipline is ccx_softmax.h's: every line is ONE operation of the stated type, and the
// including units are compiled with -ffp-contract=off.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#endif

#ifndef CCX_HD
#if defined(__HIPCC__)
#define CCX_HD __host__ __device__ __forceinline__
#else
#define CCX_HD inline
#endif
#endif

namespace ccx_tree {

constexpr int kGroupRows = 64, kBlockGroups = 4, kBlockRows = kGroupRows * kBlockGroups;

// number of block partials per quantity, B = ceil(M / 256)
CCX_HD long long blocks_of(long long M) { return (M + (kBlockRows - 1)) / kBlockRows; }

// A group of 64 consecutive rows is reduced by halving: for o = 32, 16, 8, 4, 2, 1 every place j takes s[j] + s[j ^ o] (on the
// device a wave butterfly, halve_wave below; here the array form for the host).  Every place ends with the same bits.
inline double halve64(const double* v) {
    double s[64], t[64];
    for (int j = 0; j < 64; ++j) s[j] = v[j];
    for (int o = 32; o >= 1; o >>= 1) {
        for (int j = 0; j < 64; ++j) t[j] = s[j] + s[j ^ o];
        for (int j = 0; j < 64; ++j) s[j] = t[j];
    }
    return s[0];
}

// a block of 256 consecutive rows from its four groups
CCX_HD double block_partial(double g0, double g1, double g2, double g3) { return ((g0 + g1) + g2) + g3; }

// place j of the final wave, NQ quantities at once (P = [NQ][B]): per quantity P[j], P[j + 64], ... in ascending order onto
// +0.0.  (One loop for all quantities, unrolled: the loads of several rounds are in flight together; the additions of a
// quantity keep their order.)
template <int NQ>
CCX_HD void strided_partials(const double* P, long long B, int j, double (&acc)[NQ]) {
#pragma unroll
    for (int q = 0; q < NQ; ++q) acc[q] = 0.0;
#pragma unroll 4
    for (long long i = j; i < B; i += 64) {
#pragma unroll
        for (int q = 0; q < NQ; ++q) acc[q] = acc[q] + P[(long long)q * B + i];
    }
}

// ---- the composition on the host.  One block: n <= 256 terms, the missing ones count as +0.0.
inline double block_host(const double* terms, int n) {
    double G[kBlockGroups];
    for (int g = 0; g < kBlockGroups; ++g) {
        double v[kGroupRows];
        for (int j = 0; j < kGroupRows; ++j) v[j] = g * kGroupRows + j < n ? terms[g * kGroupRows + j] : 0.0;
        G[g] = halve64(v);
    }
    return block_partial(G[0], G[1], G[2], G[3]);
}

// the final wave over one quantity's B partials
inline double final_host(const double* P, long long B) {
    double places[64];
    for (int j = 0; j < 64; ++j) {
        double one[1];
        strided_partials<1>(P, B, j, one);
        places[j] = one[0];
    }
    return halve64(places);
}

// the tree over M >= 1 consecutive terms
inline double sum_host(const double* terms, long long M) {
    const long long B = blocks_of(M);
    double* P = new double[B];
    for (long long b = 0; b < B; ++b) {
        const long long left = M - b * kBlockRows;
        P[b] = block_host(terms + b * kBlockRows, left < kBlockRows ? (int)left : kBlockRows);
    }
    const double sum = final_host(P, B);
    delete[] P;
    return sum;
}

#if defined(__HIPCC__)
// ---- the device pieces.  A group: for o = 32 .. 1 every lane takes s + (lane ^ o)'s s; f64 addition commutes, so all lanes
// agree.
__device__ __forceinline__ double halve_wave(double s) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) s = s + __shfl_xor(s, o, 64);
    return s;
}

// The epilogue of a partial kernel (a workgroup of four waves, thread t holds the NQ terms of row t of block blockIdx.x):
// each wave halves its group, lane 0 leaves it in LDS, and behind a barrier the first NQ threads add the four groups and
// write partials[q][blockIdx.x] (partials = [NQ][B]).  Every thread of the workgroup must arrive.
template <int NQ>
__device__ __forceinline__ void block_sums(double (&s)[NQ], double (&groups)[NQ][kBlockGroups], double* partials, long long B) {
    const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
        s[q] = halve_wave(s[q]);
        if (lane == 0u) groups[q][w] = s[q];
    }
    __syncthreads();
    if (threadIdx.x < (uint32_t)NQ) {
        const uint32_t q = threadIdx.x;
        partials[(long long)q * B + blockIdx.x] = block_partial(groups[q][0], groups[q][1], groups[q][2], groups[q][3]);
    }
}

// The same epilogue for a workgroup of MORE than four waves (CCX_C51: the rows of a block are worked on by sixteen waves and
// handed over in LDS): thread t < 256 holds the terms of row t, the waves behind the fourth hold nothing and only arrive at
// the barrier.  The tree is the one above: the same butterfly per group, the same block_partial.
template <int NQ>
__device__ __forceinline__ void block_sums_wide(double (&s)[NQ], double (&groups)[NQ][kBlockGroups], double* partials, long long B) {
    const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
    if (w < (uint32_t)kBlockGroups) {
#pragma unroll
        for (int q = 0; q < NQ; ++q) {
            s[q] = halve_wave(s[q]);
            if (lane == 0u) groups[q][w] = s[q];
        }
    }
    __syncthreads();
    if (threadIdx.x < (uint32_t)NQ) {
        const uint32_t q = threadIdx.x;
        partials[(long long)q * B + blockIdx.x] = block_partial(groups[q][0], groups[q][1], groups[q][2], groups[q][3]);
    }
}

// the one-quantity form: partials = [B]
__device__ __forceinline__ void block_sums(double s, double (&groups)[kBlockGroups], double* partials) {
    const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
    s = halve_wave(s);
    if (lane == 0u) groups[w] = s;
    __syncthreads();
    if (threadIdx.x == 0u) partials[blockIdx.x] = block_partial(groups[0], groups[1], groups[2], groups[3]);
}

// The opening of a final kernel (ONE wave): lane j is place j, then the butterfly per quantity.  Every lane holds the sums.
template <int NQ>
__device__ __forceinline__ void final_sums(const double* partials, long long B, double (&s)[NQ]) {
    strided_partials(partials, B, (int)threadIdx.x, s);
#pragma unroll
    for (int q = 0; q < NQ; ++q) s[q] = halve_wave(s[q]);
}

// the one-quantity form
__device__ __forceinline__ double final_sums(const double* partials, long long B) {
    double s[1];
    strided_partials<1>(partials, B, (int)threadIdx.x, s);
    return halve_wave(s[0]);
}
#endif

}  // namespace ccx_tree
