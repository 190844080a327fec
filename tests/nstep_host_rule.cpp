// The rules of csrc/ccx_nstep.h compiled for the host (tests/test_nstep_host_rule.py: -O2 -ffp-contract=off), behind a C
// interface for ctypes.  The loops here only walk records, successors and agents and copy the window's bytes and rewards into
// the arrays the header takes, as the kernel's lanes do; every slot, span, return and flag is one of ccx_nstep.h's functions.
// With -DNSTEP_HOST_MAIN the file is a program of its own: it runs the walk over a few hundred random small rings whose
// arrays have exactly the ring's size (built with -fsanitize=address,undefined: an access outside them ends the program).
#include "ccx_nstep.h"
#include "ccx_replay.h"

extern "C" {

// the cut bytes behind a push of K steps that left head_after
void host_nstep_push(unsigned char* cut, long long head_after, long long K, long long S, long long E, const unsigned char* env_flags) {
    const long long head = ccx_nstep::pushed_at(head_after, K);
    for (long long s = 0; s < K; ++s)
        for (long long e = 0; e < E; ++e) cut[ccx_replay::slot_of(head, s, S, E, e)] = ccx_nstep::cut_of(env_flags[s * E + e]);
}

void host_nstep_mark(unsigned char* cut, long long head, long long S, long long E, const unsigned char* env_mask) {
    if (head == 0) return;
    for (long long e = 0; e < E; ++e)
        if (env_mask == nullptr || env_mask[e] != 0) cut[ccx_nstep::newest_step(head, S) * E + e] = 1;
}

long long host_nstep_avail(long long head, long long p, long long S) { return ccx_nstep::avail(head, p, S); }

// the windows of index[0 .. B): per row reward f64, discount f32, span, done, valid [B][N]; per record last (the slot the
// window ends on, -1 outside the ring) and m_env [B]
void host_nstep_fetch(const double* ring_reward, const unsigned char* ring_done, const unsigned char* ring_valid,
                      const unsigned char* cut, long long head, long long S, long long E, long long N, int n, float gamma,
                      long long B, const long long* index, double* reward, float* discount, unsigned char* span,
                      unsigned char* done, unsigned char* valid, long long* last, int* m_env_out) {
    constexpr int kMax = ccx_nstep::kMax;
    const long long R = S * E;
    for (long long b = 0; b < B; ++b) {
        const long long idx = index[b];
        const bool read = ccx_replay::in_ring(idx, R);
        const long long at0 = read ? idx : 0;
        const long long p = at0 / E, e = at0 - p * E;
        unsigned char ct[kMax];
        for (int k = 0; k < kMax; ++k) ct[k] = 0;
        if (read)
            for (int k = 0; k < n; ++k) ct[k] = cut[ccx_nstep::slot_k<long long>(p, k, S, E, e)];
        const long long av = read ? ccx_nstep::avail(head, p, S) : 0;
        const int m_env = ccx_nstep::env_span(n, av, ct);
        last[b] = read ? ccx_nstep::slot_k<long long>(p, m_env - 1, S, E, e) : -1;
        m_env_out[b] = m_env;
        for (long long a = 0; a < N; ++a) {
            unsigned char dn[kMax], vl[kMax];
            double rw[kMax];
            for (int k = 0; k < kMax; ++k) {
                dn[k] = ccx_replay::kEmptyDone;
                vl[k] = ccx_replay::kEmptyValid;
                rw[k] = ccx_replay::kEmptyReward;
            }
            if (read)
                for (int k = 0; k < n; ++k) {
                    const long long sk = ccx_nstep::slot_k<long long>(p, k, S, E, e) * N + a;
                    dn[k] = ring_done[sk];
                    vl[k] = ring_valid[sk];
                    rw[k] = ring_reward[sk];
                }
            const ccx_nstep::Span<unsigned char> sp = ccx_nstep::agent_span(m_env, dn, vl);
            const int m_a = sp.m;
            const ccx_nstep::Return ret = ccx_nstep::returns(m_a, rw, gamma);
            const unsigned char done_out = sp.done_out;
            reward[b * N + a] = ret.G;
            discount[b * N + a] = ret.discount;
            span[b * N + a] = (unsigned char)m_a;
            done[b * N + a] = done_out;
            valid[b * N + a] = ccx_nstep::dropped(m_a, m_env, done_out) ? (unsigned char)0 : vl[0];
        }
    }
}

}  // extern "C"

#if defined(NSTEP_HOST_MAIN)
#include <cstdio>
#include <vector>

namespace {

unsigned long long state = 0x9E3779B97F4A7C15ull;
unsigned next(unsigned below) {                                          // xorshift64*: small, seeded, the same everywhere
    state ^= state >> 12; state ^= state << 25; state ^= state >> 27;
    return (unsigned)(((state * 0x2545F4914F6CDD1Dull) >> 33) % below);
}

}  // namespace

int main() {
    long long windows = 0, longest = 0;
    for (int round = 0; round < 400; ++round) {
        const long long S = 1 + next(9), E = 1 + next(4), N = 1 + next(4), R = S * E;
        const int n = 1 + (int)next((unsigned)(S < ccx_nstep::kMax ? S : ccx_nstep::kMax));
        std::vector<double> ring_reward(R * N);
        std::vector<unsigned char> ring_done(R * N), ring_valid(R * N), cut(R, 0);
        for (long long i = 0; i < R * N; ++i) {
            ring_reward[i] = (double)next(2000) / 1000.0 - 1.0;
            ring_done[i] = next(8) == 0 ? 1 : 0;
            ring_valid[i] = next(8) == 0 ? 0 : 4;
        }
        // heads at the edges: empty, partly filled, exactly full, rewritten, far out, and a junk value below zero
        const long long heads[] = {0, 1, S - 1 > 0 ? S - 1 : 0, S, S + 1, 2 * S, 3 * S + 2, (1ll << 40) + 3, -5};
        for (const long long head : heads) {
            if (head > 0) {                                              // the latest block of K steps, and a manual cut
                const long long K = 1 + next((unsigned)S);
                std::vector<unsigned char> env_flags(K * E);
                for (auto& f : env_flags) f = (unsigned char)(next(4) == 0 ? (1u << next(8)) : 0u);
                host_nstep_push(cut.data(), head, K, S, E, env_flags.data());
                if (next(3) == 0) host_nstep_mark(cut.data(), head, S, E, nullptr);
            }
            std::vector<long long> index;
            for (long long i = -2; i < R + 2; ++i) index.push_back(i);
            index.push_back(1ll << 40);
            index.push_back(-(1ll << 62));
            const long long B = (long long)index.size();
            std::vector<double> reward(B * N);
            std::vector<float> discount(B * N);
            std::vector<unsigned char> span(B * N), done(B * N), valid(B * N);
            std::vector<long long> last(B);
            std::vector<int> m_env(B);
            const float gamma = next(3) == 0 ? 1.0f : (next(2) ? 0.0f : 0.99f);
            host_nstep_fetch(ring_reward.data(), ring_done.data(), ring_valid.data(), cut.data(), head, S, E, N, n, gamma, B,
                             index.data(), reward.data(), discount.data(), span.data(), done.data(), valid.data(), last.data(),
                             m_env.data());
            for (long long b = 0; b < B; ++b) {
                const bool inside = index[b] >= 0 && index[b] < R;
                if (m_env[b] < 1 || m_env[b] > n || (inside ? (last[b] < 0 || last[b] >= R) : (last[b] != -1 || m_env[b] != 1))) {
                    std::printf("round %d head %lld b %lld: m_env %d last %lld\n", round, head, b, m_env[b], last[b]);
                    return 1;
                }
                for (long long a = 0; a < N; ++a)
                    if (span[b * N + a] < 1 || span[b * N + a] > m_env[b]) {
                        std::printf("round %d head %lld b %lld a %lld: span %d of %d\n", round, head, b, a, (int)span[b * N + a], m_env[b]);
                        return 1;
                    }
                ++windows;
                longest = m_env[b] > longest ? m_env[b] : longest;
            }
        }
    }
    std::printf("%lld windows walked, the longest of %lld steps\n", windows, longest);
    return longest > 1 ? 0 : 1;
}
#endif
