// ccx_nstep.h -- CCX_NSTEP (include/ccx.h) as inline functions: the slot of the k-th successor of a record, the number of
// successors that exist, the env-level and the per-agent length of the window, the f64 chain of the discounted return, the
// dropped row and the byte ccx_nstep_push makes of a step's env flags.  Included by ccx_nstep.hip; it also compiles with a
// plain host C++ compiler (tests/test_nstep_host_rule.py runs it against the spec of tests/_nstep_spec.py bit for bit).
// The window's bytes and rewards arrive as arrays of kMax elements, element k being record slot_k's; only the elements k < n
// are read.  Every loop runs its full static length with the condition carried along, so that on the device the arrays stay
// in registers; every f64 line is ONE operation, and what lies beyond the window is SELECTED away, never multiplied by zero.
// The byte arrays are templates on their element: the host walks uint8_t, the kernel holds each byte in a 32-bit register of
// its own (bytes packed four to a register would make every load wait for the one before it).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define CCX_NS_HD __host__ __device__ __forceinline__
#else
#define CCX_NS_HD inline
#endif

namespace ccx_nstep {

constexpr int kMax = 16;                                                  // CCX_NSTEP_MAX (asserted equal in ccx_nstep.hip)
constexpr uint32_t kCutFlags = 0x01u | 0x02u | 0x04u;                     // CCX_EF_ALL_TERMINATED | _ALL_TRUNCATED | _RESET (asserted there)

// cut byte of a pushed step: the episode of the env ended with it
CCX_NS_HD uint8_t cut_of(uint32_t env_flags) { return (env_flags & kCutFlags) != 0u ? (uint8_t)1 : (uint8_t)0; }

// the head the ring's push read, from the head it left behind: head' - K, and 0 for a caller that pushed nothing
CCX_NS_HD long long pushed_at(long long head_after, long long K) {
    const long long head = head_after - K;
    return head < 0 ? 0 : head;
}

// a mod S in [0, S), for any a
CCX_NS_HD long long mod_steps(long long a, long long S) {
    const long long r = a % S;
    return r < 0 ? r + S : r;
}

// record slot of the k-th successor of the record at ring step p, env e: ((p + k) mod S) * E + e.  0 <= p < S and 0 <= k <= S
// (a window is never longer than the ring), so the reduction is one conditional subtraction: the slot lies in [0, S E).
// (A template on the integer: the host walks long long, the kernel 32 bits -- S E < 2^31.)
template <class Int>
CCX_NS_HD Int slot_k(Int p, Int k, Int S, Int E, Int e) {
    const Int q = p + k;
    return (q >= S ? q - S : q) * E + e;
}

// the newest ring step, (head - 1) mod S: only meaningful while head != 0
CCX_NS_HD long long newest_step(long long head, long long S) { return mod_steps(head - 1, S); }

// successors of ring step p that exist: none in an empty ring or for a step not yet pushed, else (head - 1 - p) mod S
CCX_NS_HD long long avail(long long head, long long p, long long S) {
    if (head == 0) return 0;
    if (head < S && p >= head) return 0;
    return mod_steps(head - 1 - p, S);
}

// m_env = 1; while (m_env < n && m_env <= avail && cut[m_env - 1] == 0) ++m_env
template <class Byte>
CCX_NS_HD int env_span(int n, long long av, const Byte (&cut)[kMax]) {
    int m = 1;
    bool go = true;
#pragma unroll
    for (int k = 1; k < kMax; ++k) {
        go = go && k < n && (long long)k <= av && cut[k - 1] == 0;
        m += go ? 1 : 0;
    }
    return m;
}

// m_a = 1; while (m_a < m_env && done[m_a - 1] == 0 && valid[m_a] != 0) ++m_a;  done_out = done[m_a - 1], carried along with
// the walk (selected by the walk's own condition, not looked up by index afterwards)
template <class Byte>
struct Span { int m; Byte done_out; };
template <class Byte>
CCX_NS_HD Span<Byte> agent_span(int m_env, const Byte (&done)[kMax], const Byte (&valid)[kMax]) {
    int m = 1;
    Byte last = done[0];
    bool go = true;
#pragma unroll
    for (int k = 1; k < kMax; ++k) {
        go = go && k < m_env && done[k - 1] == 0 && valid[k] != 0;
        m += go ? 1 : 0;
        last = go ? done[k] : last;
    }
    return Span<Byte>{m, last};
}

// G = reward[0] + gamma reward[1] + ... + gamma^(m - 1) reward[m - 1], k ascending, and discount = (float)gamma^m
struct Return { double G; float discount; };
CCX_NS_HD Return returns(int m, const double (&reward)[kMax], float gamma) {
    const double gd = (double)gamma;
    double g = 1.0, G = reward[0];
#pragma unroll
    for (int k = 1; k < kMax; ++k) {
        const double gn = g * gd;
        const double t = gn * reward[k];
        const double Gn = G + t;
        g = (k < m) ? gn : g;
        G = (k < m) ? Gn : G;
    }
    g = g * gd;
    return Return{G, (float)g};
}

// the agent stopped being live inside the env's window without terminating: the row is left out
CCX_NS_HD bool dropped(int m_a, int m_env, uint32_t done_out) { return m_a < m_env && done_out == 0; }

}  // namespace ccx_nstep
