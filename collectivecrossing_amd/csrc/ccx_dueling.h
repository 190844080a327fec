// ccx_dueling.h -- CCX_DUELING (include/ccx.h) as inline functions: the dueling combine of one row, forward and backward.
// A row of a dueling head's output is va[6]: va[k], k = 0..4, the advantage of action k (index = action id), va[5] the state
// value.  Included by ccx_dueling.hip (rows from memory, and the fused actor kernel of one head) and by the fused actor
// kernel of ccx_sides.hip (rows from the tile); it also compiles with a plain host C++ compiler (tests/test_dueling_host_rule.py runs it against the
// NumPy spec bit for bit).
// The discipline is ccx_qlearn.h's: every line is ONE correctly rounded f32 operation, the including units are compiled with
// -ffp-contract=off, `/` is the correctly rounded division.
// The mean runs over ALL five actions whatever the state's mask says: the combine is a property of the network, the mask a
// property of the state (the legal set enters where an action is chosen, ccx_qlearn.h's greedy / choice, not here).
#pragma once
#include <stdint.h>

#ifndef CCX_HD
#if defined(__HIPCC__)
#define CCX_HD __host__ __device__ __forceinline__
#else
#define CCX_HD inline
#endif
#endif

namespace ccx_dueling {

constexpr int kActions = 5, kRow = 6;                                     // q has five values to a row, va six

// q_k = va5 + (va_k - mean(va_0..4)).  A NaN in one advantage reaches all five q of the row (through the mean).
CCX_HD void forward(const float (&va)[kRow], float (&q)[kActions]) {
    const float s01 = va[0] + va[1];
    const float s012 = s01 + va[2];
    const float s0123 = s012 + va[3];
    const float s = s0123 + va[4];
    const float mean = s / 5.0f;
#pragma unroll
    for (int k = 0; k < kActions; ++k) {
        const float c = va[k] - mean;
        q[k] = va[5] + c;
    }
}

// A pure function of grad_q: it reads neither va nor q.  Five +0.0 give six +0.0 (t = +0, gm = +0 / 5 = +0, +0 - +0 = +0):
// a row that does not count in ccx_td_loss_backward stays exactly +0.0 through the combine.
CCX_HD void backward(const float (&g)[kActions], float (&gva)[kRow]) {
    const float t01 = g[0] + g[1];
    const float t012 = t01 + g[2];
    const float t0123 = t012 + g[3];
    const float t = t0123 + g[4];
    const float gm = t / 5.0f;
#pragma unroll
    for (int k = 0; k < kActions; ++k) gva[k] = g[k] - gm;
    gva[5] = t;
}

}  // namespace ccx_dueling
