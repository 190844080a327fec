// The step rule of csrc/ccx_step_rule.h compiled for the host (tests/test_step_rule_host.py: -O2 -ffp-contract=off), behind
// a C interface for ctypes.  With -DSTEP_RULE_MAIN it is a stand-alone program that walks the same cases against
// statements written out here (for a sanitiser build; exit status 0 = all equal).
#include "ccx_step_rule.h"

#include <stdint.h>

extern "C" {

// geom: W, H, div, tl, tr, dl, dr, bdy, edy.  term_b / term_e: u8 [(H + 1)(W + 1)] or null (the built-in rule).
// out: u64 [(H + 3)(W + 3)], every cell of the padded grid.
void host_cell_table(const int* geom, int reward_mode, const uint8_t* term_b, const uint8_t* term_e, unsigned long long* out) {
    const ccx::CellGeometry g{geom[0], geom[1], geom[2], geom[3], geom[4], geom[5], geom[6], geom[7], geom[8]};
    const int Wp = g.W + 3;
    for (int y = -1; y <= g.H + 1; ++y)
        for (int x = -1; x <= g.W + 1; ++x) {
            const bool in = x >= 0 && x <= g.W && y >= 0 && y <= g.H;
            const int tb = (term_b && in) ? term_b[y * (g.W + 1) + x] : -1, te = (term_e && in) ? term_e[y * (g.W + 1) + x] : -1;
            out[ccx::cell_index(x, y, Wp)] = ccx::cell_word(g, reward_mode, x, y, tb, te);
        }
}
int host_cell_ok(const int* geom, int x, int y) {
    const ccx::CellGeometry g{geom[0], geom[1], geom[2], geom[3], geom[4], geom[5], geom[6], geom[7], geom[8]};
    return ccx::cell_ok(g, x, y) ? 1 : 0;
}
int host_cell_index(int x, int y, int Wp) { return ccx::cell_index(x, y, Wp); }
int host_cell_origin(int Wp) { return ccx::cell_origin(Wp); }
int host_cell_of_placement(uint32_t pn, int Wp) { return ccx::cell_of_placement(pn, Wp); }
// out: legality bits of actions 0..4 (bit a), legal4, info flags, x, y, at-destination, terminated, class, distance
void host_cell_fields(unsigned long long word, int boarding, int32_t* out) {
    const uint32_t lo = (uint32_t)word, hi = (uint32_t)(word >> 32);
    const uint32_t tsh = ccx::cell_tsh(boarding != 0), tsh2 = ccx::cell_tsh2(boarding != 0);
    uint32_t legal = 0;
    for (uint32_t a = 0; a < 5; ++a) legal |= ccx::cell_legal(lo, a) << a;
    out[0] = (int32_t)legal;
    out[1] = (int32_t)ccx::cell_legal4(lo);
    out[2] = (int32_t)ccx::cell_info_flags(lo);
    out[3] = (int32_t)ccx::cell_x(lo);
    out[4] = (int32_t)ccx::cell_y(lo);
    out[5] = (int32_t)ccx::cell_at_dest(lo, tsh);
    out[6] = (int32_t)ccx::cell_terminated(lo, tsh);
    out[7] = (int32_t)ccx::cell_class(lo, tsh);
    out[8] = ccx::cell_distance(hi, tsh2);
    out[9] = (int32_t)(ccx::cell_xy_bytes(ccx::cell_x(lo), ccx::cell_y(lo)) == (lo & 0xFFFF0000u));
}

struct HostRewards { int reward_mode; double r_dest, r_nogoal, r_pen; };
// the reward of a LIVE (live != 0) or done agent of the given type on the cell `word`
double host_cell_reward(unsigned long long word, int boarding, int live, int reward_mode, double r_dest, double r_door, double r_area,
                        double r_f, double r_nogoal, double r_pen) {
    const HostRewards p{reward_mode, r_dest, r_nogoal, r_pen};
    const double r = ccx::cell_reward((uint32_t)word, (uint32_t)(word >> 32), ccx::cell_tsh(boarding != 0), ccx::cell_tsh2(boarding != 0),
                                      ccx::reward_class_a(p), r_door, r_area, r_f);
    return ccx::reward_if_live(r, (uint32_t)live);
}

uint32_t host_agent_flag_byte(uint32_t out2, uint32_t flags_before, uint32_t lo, int boarding, uint32_t act) {
    return ccx::agent_flag_byte(out2, flags_before, lo, ccx::cell_tsh(boarding != 0), act);
}
uint32_t host_env_flag_byte(uint32_t ef, int resets) { return ccx::env_flag_byte(ef, resets ? (uint32_t)ccx::CCX_K_EF_RESET : 0u); }

unsigned long long host_pool_stride(unsigned long long total_envs, unsigned long long P) { return ccx::pool_stride_of(total_envs, P); }
unsigned long long host_pool_entry(unsigned long long global_env, unsigned long long episode, unsigned long long stride,
                                   unsigned long long P) {
    return ccx::pool_entry(global_env, episode, stride, P);
}

}  // extern "C"

#ifdef STEP_RULE_MAIN
#include <cstdio>
#include <vector>

namespace {

int g_bad = 0;
void expect(bool ok, const char* what, long long a = 0, long long b = 0, long long c = 0) {
    if (!ok && g_bad++ < 20) std::printf("MISMATCH %s (%lld, %lld, %lld)\n", what, a, b, c);
}

// collectivecrossing.py:509-534, written out
bool ok_here(const int* g, int x, int y) {
    if (x < 0 || x > g[0] || y < 0 || y > g[1]) return false;
    if (y == g[2] && !(g[5] < x && x < g[6])) return false;
    if (y >= g[2] && !(g[3] < x && x < g[4])) return false;
    return true;
}

void walk_geometry(const int* g, bool user_term) {
    const int W = g[0], H = g[1], Wp = W + 3, Hp = H + 3;
    std::vector<uint8_t> tb((size_t)(W + 1) * (H + 1)), te(tb.size());
    for (size_t k = 0; k < tb.size(); ++k) { tb[k] = (uint8_t)(k % 3 == 0); te[k] = (uint8_t)(k % 5 == 1 ? 7 : 0); }
    std::vector<unsigned long long> tab((size_t)Wp * Hp, ~0ull);
    for (int mode = 0; mode < 4; ++mode) {
        host_cell_table(g, mode, user_term ? tb.data() : nullptr, user_term ? te.data() : nullptr, tab.data());
        for (int y = -1; y <= H + 1; ++y)
            for (int x = -1; x <= W + 1; ++x) {
                const unsigned long long w = tab[(size_t)host_cell_index(x, y, Wp)];
                const bool in = x >= 0 && x <= W && y >= 0 && y <= H;
                if (!in) { expect(w == 0ull, "border cell", x, y); continue; }
                expect(host_cell_ok(g, x, y) == (ok_here(g, x, y) ? 1 : 0), "cell_ok", x, y);
                for (int b = 0; b < 2; ++b) {
                    int32_t f[10];
                    host_cell_fields(w, b, f);
                    const int want = (ok_here(g, x + 1, y) ? 1 : 0) | (ok_here(g, x, y + 1) ? 2 : 0) | (ok_here(g, x - 1, y) ? 4 : 0) |
                                     (ok_here(g, x, y - 1) ? 8 : 0);
                    expect(f[0] == want && f[1] == want, "legality", x, y, f[0]);
                    const bool in_tram = y >= g[2] && g[3] <= x && x <= g[4], at_door = y == g[2] && (x == g[5] - 1 || x == g[6] + 1);
                    expect(f[2] == ((in_tram ? 0x10 : 0) | (at_door ? 0x20 : 0)), "info bits", x, y, f[2]);
                    expect(f[3] == x && f[4] == y && f[9] == 1, "x / y bytes", x, y);
                    const bool dest = y == (b ? g[7] : g[8]);
                    expect(f[5] == (dest ? 1 : 0), "destination bit", x, y, b);
                    const int term = user_term ? ((b ? tb : te)[(size_t)y * (W + 1) + x] != 0 ? 1 : 0) : (dest ? 1 : 0);
                    expect(f[6] == term, "terminated bit", x, y, b);
                    for (int live = 0; live < 2; ++live) {
                        const double r = host_cell_reward(w, b, live, mode, 15.0, 10.0, 5.0, 0.1, 0.0, -1.0);
                        expect(live || (r == 0.0 && !__builtin_signbit(r)), "reward of a done agent", x, y, b);
                        if (live && f[7] == 0 && f[8] == 0) expect(r == 0.0 && !__builtin_signbit(r), "+0.0 at distance 0", x, y, b);
                    }
                }
            }
    }
    expect(host_cell_origin(Wp) == host_cell_index(0, 0, Wp), "cell_origin");
    for (int y = 0; y <= H; ++y)
        for (int x = 0; x <= W; ++x)
            expect(host_cell_of_placement((uint32_t)x | ((uint32_t)y << 8), Wp) == host_cell_index(x, y, Wp), "cell_of_placement", x, y);
}

}  // namespace

int main() {
    const int bench[9] = {12, 8, 4, 2, 10, 7, 9, 8, 0};       // the 12 x 8 benchmark geometry (tram 2..10, door 7..9)
    const int small[9] = {12, 8, 4, 1, 11, 4, 8, 8, 0};       // the smallest grid of the split-step cases
    const int offc[9] = {13, 9, 5, 1, 12, 3, 8, 9, 0};        // door 3..8: (3 + 8) / 2 rounds
    walk_geometry(bench, false);
    walk_geometry(small, false);
    walk_geometry(small, true);
    walk_geometry(offc, false);
    // the flag byte, include/ccx.h:81-89 written out
    for (uint32_t out2 = 0; out2 < 4; ++out2)
        for (uint32_t before = 0; before < 4; ++before)
            for (uint32_t act = 0; act < 2; ++act)
                for (uint32_t dest = 0; dest < 2; ++dest)
                    for (uint32_t info = 0; info < 4; ++info)
                        for (int b = 0; b < 2; ++b) {
                            const uint32_t lo = (info << 5) | (dest << (b ? 8 : 12)) | ((dest ^ 1u) << (b ? 12 : 8)) | 0xABCD000Fu;
                            const bool live = before == 0, emit = live || (out2 & ~before) != 0;
                            const uint32_t want = (out2 & 1u ? 0x01u : 0u) | (out2 & 2u ? 0x02u : 0u) | (live ? 0x04u : 0u) | (emit ? 0x08u : 0u) |
                                                  (info & 1u ? 0x10u : 0u) | (info & 2u ? 0x20u : 0u) | (act ? 0x40u : 0u) | (dest ? 0x80u : 0u);
                            expect(host_agent_flag_byte(out2, before, lo, b, act) == want, "flag byte", out2, before, lo);
                        }
    for (uint32_t ef = 0; ef < 4; ++ef)
        for (int resets = 0; resets < 2; ++resets)
            expect(host_env_flag_byte(ef, resets) == (ef | ((ef != 0 && resets) ? 4u : 0u)), "env byte", ef, resets);
    // the pool cursor against 128-bit arithmetic
    const unsigned long long Ps[] = {1, 2, 3, 7, 1024, 100003}, eps[] = {0, 1, 7, (1ull << 31) - 2};
    const unsigned long long gs[] = {0, 5, (1ull << 31) - 30, (1ull << 31), (1ull << 32) - 29, (1ull << 32), (1ull << 40) + 12345};
    for (unsigned long long P : Ps)
        for (unsigned long long total : {P, P + 1, 2 * P - 1, (1ull << 33) + 93100ull, P * 50000ull})
            for (unsigned long long ep : eps)
                for (unsigned long long ep2 : {ep, ep + P})
                    for (unsigned long long g : gs) {
                        const unsigned long long stride = host_pool_stride(total, P);
                        expect(stride == (total % P ? total % P : 1 % P), "pool stride", (long long)total, (long long)P);
                        const unsigned __int128 want = ((unsigned __int128)g + (unsigned __int128)ep2 * stride) % P;
                        expect(host_pool_entry(g, ep2, stride, P) == (unsigned long long)want, "pool cursor", (long long)g, (long long)ep2, (long long)P);
                    }
    std::printf(g_bad ? "step rule: %d mismatches\n" : "step rule: all cases equal\n", g_bad);
    return g_bad ? 1 : 0;
}
#endif
