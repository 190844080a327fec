// ccx_loss.h -- the frame of a loss over the rows that count (CCX_PPO_LOSS with the masked moments, CCX_QLEARN's TD loss and
// its discounted form, CCX_C51's categorical loss), stated ONCE: what stands around a unit's per-row rule on the device and
// around its launches in the entry.  This header includes no rule: which rows count (ccx_ppo::row_counts, or
// ccx_qlearn::row_counts and row_bad), a row's terms and the final values stay in ccx_ppo.h, ccx_qlearn.h and ccx_c51.h; the
// tree the sums go through is ccx_tree.h's.  The discipline is ccx_tree.h's: every line is ONE operation of the stated type,
// and the including units are compiled with -ffp-contract=off.
//
// Forward: a partial kernel (a block of 256 consecutive rows to a workgroup) and a final kernel (ONE wave), two plain
// launches: no atomic, no last-block-done counter.  Rows that do not count and rows >= M enter the sums as +0.0, selected.
// Backward: one launch that recomputes the forward terms and reads nothing of the forward but `stats`; with n = stats[6] == 0
// every gradient is +0.0f, selected, never the product of a scale that is not finite.
#pragma once
#include "ccx_internal.h"
#include "ccx_tree.h"

namespace ccx_loss {

// ---- device pieces

// What decides whether a row counts, as the unit's own row_counts / row_bad take it: the action byte and the `valid` byte
// (1 where there is no `valid`) at rl, the row's index clamped to M - 1 (surplus lanes load what the last row loads).
struct Gate {
    uint32_t a, vbyte;
    bool has_valid;
};

__device__ __forceinline__ Gate gate_of(const uint8_t* actions, const uint8_t* valid, long long rl) {
    Gate g;
    g.a = actions[rl];
    g.has_valid = valid != nullptr;
    g.vbyte = g.has_valid ? (uint32_t)valid[rl] : 1u;
    return g;
}

// A row's NT f32 terms into the sums ccx_tree::block_sums / block_sums_wide take: s[0] is the count, s[1 + k] term k, exact
// as f64.  Sums behind them (a tally of bad rows) are the unit's.
template <int NT, int NQ>
__device__ __forceinline__ void select_sums(bool counts, const float (&t)[NT], double (&s)[NQ]) {
    static_assert(NT < NQ, "the count stands in front of the terms");
    s[0] = counts ? 1.0 : 0.0;
#pragma unroll
    for (int k = 0; k < NT; ++k) s[1 + k] = counts ? (double)t[k] : 0.0;
}

// The body of a final kernel (ONE wave): the tree's last level over partials = [NQ][B], then lane 0 takes the NO final
// values from finals(sums, values) and stores them.
template <int NQ, int NO, class Finals>
__device__ __forceinline__ void final_body(const double* partials, long long B, float* out, Finals finals) {
    double s[NQ];
    ccx_tree::final_sums(partials, B, s);
    if (threadIdx.x == 0u) {
        float o[NO];
        finals(s, o);
#pragma unroll
        for (int k = 0; k < NO; ++k) out[k] = o[k];
    }
}

// The opening of a backward kernel: whether any row counted at all (n = stats[6]), and sc = grad_loss / n, the correctly
// rounded f32 division made once per call (grad_loss absent = 1.0f).  A row's `counts` is `any && row_counts(...)`.  A kernel
// whose waves leave early where their row does not count (CCX_C51) takes any_counted in front of the branch and the scale
// inside it.
struct Scale {
    float sc;
    bool any;
};

__device__ __forceinline__ bool any_counted(const float* stats_in) { return stats_in[6] != 0.0f; }

__device__ __forceinline__ Scale scale_of(const float* stats_in, const float* grad_loss) {
    const float n = stats_in[6];
    const float g = grad_loss ? grad_loss[0] : 1.0f;
    return Scale{g / n, any_counted(stats_in)};
}

// ---- host pieces

// bytes of a forward's workspace, partials = [nq][B] f64; 0 for rows < 1
inline int64_t workspace_bytes(int64_t rows, int nq) {
    return rows < 1 ? 0 : (int64_t)ccx_tree::blocks_of(rows) * nq * (int64_t)sizeof(double);
}

inline int check_gamma(const char* who, float gamma) {
    if (!(gamma >= 0.0f && gamma <= 1.0f)) return ccxi::fail(CCX_EINVAL, "%s: gamma must be finite and lie in [0, 1], got %g", who, (double)gamma);
    return CCX_OK;
}

inline int no_check() { return CCX_OK; }

// The forward entry of a loss over the tree.  `required`: every pointer of the entry's NULL list is there; `optional` names
// the ones that need not be.  early() and late() are the entry's own refusals in front of and behind the workspace's (its
// alignments, its hyper-parameters), each returning a code.  partial(partials, blocks) fills the entry's argument struct,
// launches its instantiation of the partial kernel over `blocks` workgroups and returns the struct for final_kernel.
template <class Early, class Late, class Partial, class Args>
int forward(const char* who, ccx_handle* h, bool required, const char* optional, int64_t rows, void* workspace, Early early,
            Late late, Partial partial, void (*final_kernel)(Args)) {
    if (!h) return ccxi::fail(CCX_EINVAL, "NULL handle");
    if (!required) return ccxi::fail(CCX_EINVAL, "%s: NULL argument (%s)", who, optional);
    unsigned blocks = 0;
    if (int rc = ccxi::row_blocks(who, rows, ccx_tree::kBlockRows, blocks)) return rc;
    if (int rc = early()) return rc;
    if (ccxi::misaligned(8, workspace)) return ccxi::fail(CCX_EINVAL, "%s: workspace must be 8-byte aligned", who);
    if (int rc = late()) return rc;
    CCX_HIP(hipSetDevice(h->device));
    const Args A = partial(static_cast<double*>(workspace), blocks);
    hipLaunchKernelGGL(final_kernel, dim3(1), dim3(64), 0, h->stream, A);
    CCX_HIP(hipGetLastError());
    return CCX_OK;
}

}  // namespace ccx_loss
