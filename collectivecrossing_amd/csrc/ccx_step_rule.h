// ccx_step_rule.h -- the per-agent rule of ONE env-step, stated once: what a cell word means, what reward a cell pays, how
// the flag bytes are built, which pool entry a restarted env takes.  Included by every kernel that steps envs (the rollout
// kernel, the short-launch kernel, the split step, the policy / mask / reset kernels), which inline exactly these functions,
// and by build_cell_table (ccx_api.hip); it also compiles with a plain host C++ compiler (tests/test_step_rule_host.py runs
// it against independent statements of the reference's lines and against the CPU oracle, bit for bit).
// Plain C++17: no HIP type, no global state.
#pragma once
#include <stdint.h>

#ifndef CCX_HD
#if defined(__HIPCC__)
#define CCX_HD __host__ __device__ __forceinline__
#else
#define CCX_HD inline
#endif
#endif

namespace ccx {

enum : int { CCX_K_REWARD_DEFAULT = 0, CCX_K_REWARD_SIMPLE_DISTANCE = 1, CCX_K_REWARD_BINARY = 2,
             CCX_K_REWARD_CONSTANT_NEGATIVE = 3 };
enum : uint32_t { CCX_K_EF_ALL_TERM = 1u, CCX_K_EF_ALL_TRUNC = 2u, CCX_K_EF_RESET = 4u };   // include/ccx.h: CCX_EF_*

// ---- 1. the cell word -------------------------------------------------------------------------------------------------
// Everything the step needs to know about a grid cell is precomputed once per handle on the host (ccx_api.hip:
// build_cell_table, a loop over cell_word) for the padded grid x in [-1, W+1], y in [-1, H+1] (cell_index) and copied to LDS
// at kernel start, one 64-bit word per cell:
//   lo: bits 0-3  move a (right, up, left, down) from this cell lands on a cell that is in the
//                 grid and not a wall                       (collectivecrossing.py:509-534)
//       bit4 = 0 always (the "legality bit" of action 4 = wait: `(lo >> a) & 1` needs no clamp)
//       bit5 IN_TRAM_AREA (:551-554)  bit6 AT_DOOR (:556-563)       -- CCX_AF_* bits 4/5, shifted up by one
//       bit8  boarding: on destination row (:663-683)   bits 9-10  boarding reward class
//       bit11 boarding: terminateds[id] on this cell (terminateds.py:66-82: = bit 8 for the built-in strategies;
//             ccx_set_terminated_table overrides it)
//       bit12 exiting:  on destination row              bits 13-14 exiting reward class
//       bit15 exiting:  terminateds[id] on this cell (= bit 12, or the user's table)
//       byte2 = x, byte3 = y  (0 for border cells)
//   hi: int16 signed distance term of the boarding reward | int16 of the exiting reward << 16
// reward class (rewards.py:44-182): 0 = (double)sd * distance_penalty_factor, 1/2/3 = constants
// rA/rB/rC chosen per reward mode (reward_class_a).  Border cells are 0: never occupied, no move lands there.
// The word of the agent's CURRENT cell is carried in registers, so the legality of a move is a bit test; the word of the
// proposed cell is fetched off the critical path and only consumed once the move is known to happen.  The sim wave hands a
// writer wave ONE word per lane and step (ccx_kernels.h: kHw*) that holds the LDS address of the agent's cell word; the
// writer looks the word up itself.
constexpr uint32_t kCellLegalMask = 0xFu;                          // bits 0-3
constexpr uint32_t kCellInTram = 0x20u, kCellAtDoor = 0x40u;
constexpr uint32_t kCellInfoShift = 1u, kCellInfoMask = 0x30u;     // (lo >> 1) & 0x30 = CCX_AF_IN_TRAM_AREA | CCX_AF_AT_DOOR
constexpr uint32_t kCellBoardingShift = 8u, kCellExitingShift = 12u;   // the type's nibble: destination bit, class, terminated
constexpr uint32_t kCellClassShift = 1u, kCellClassMask = 3u;      // (relative to the type's destination bit)
constexpr uint32_t kCellTermShift = 3u;                            // (relative to the type's destination bit)
constexpr uint32_t kCellXShift = 16u, kCellYShift = 24u, kCellByteMask = 0xFFu;
constexpr uint32_t kCellDistBoardingShift = 0u, kCellDistExitingShift = 16u;   // halves of the high word

// what the cell rules read of the geometry: any type with these fields (KParams has them)
struct CellGeometry { int W, H, div, tl, tr, dl, dr, bdy, edy; };

CCX_HD int cell_index(int x, int y, int Wp) { return (y + 1) * Wp + x + 1; }              // Wp = W + 3
CCX_HD int cell_origin(int Wp) { return Wp + 1; }                                         // = cell_index(0, 0, Wp)
// a reset-pool placement (u16: x | y << 8, include/ccx.h: ccx_set_reset_pool) -> its cell
CCX_HD int cell_of_placement(uint32_t pn, int Wp) { return (int)(pn >> 8) * Wp + (int)(pn & kCellByteMask) + Wp + 1; }

// collectivecrossing.py:509-534 _is_valid_position (+ :565-588 _would_hit_tram_wall, which it implies)
template <typename G>
CCX_HD bool cell_ok(const G& g, int x, int y) {
    bool ok = x >= 0 && x <= g.W && y >= 0 && y <= g.H;
    if (y == g.div) ok = ok && (g.dl < x && x < g.dr);
    if (y >= g.div) ok = ok && (g.tl < x && x < g.tr);
    return ok;
}

CCX_HD uint32_t cell_xy_bytes(uint32_t x, uint32_t y) { return (x << kCellXShift) | (y << kCellYShift); }   // bytes 2 and 3

// The word of cell (x, y); 0 outside the grid.  term_b / term_e: terminateds[id] of a boarding / exiting agent on this cell
// as a position-only user strategy says (0 / 1), or negative for the built-in rule (the destination row).
template <typename G>
CCX_HD unsigned long long cell_word(const G& g, int reward_mode, int x, int y, int term_b, int term_e) {
    if (!(x >= 0 && x <= g.W && y >= 0 && y <= g.H)) return 0ull;
    const int DX[4] = {1, 0, -1, 0}, DY[4] = {0, 1, 0, -1};   // actions.py:18-24
    uint32_t lo = 0;
    for (int a = 0; a < 4; ++a) lo |= (cell_ok(g, x + DX[a], y + DY[a]) ? 1u : 0u) << a;
    const bool in_area = y >= g.div && g.tl <= x && x <= g.tr;
    const bool at_door = y == g.div && (x == g.dl - 1 || x == g.dr + 1);
    const bool dest_b = y == g.bdy, dest_e = y == g.edy;
    const int dc = (g.dl + g.dr) / 2;                          // observations.py:70-71, rewards.py:81
    const int adx = x > dc ? x - dc : dc - x;
    uint32_t cls_b = 1, cls_e = 1;                             // binary / constant_negative: always the constant rA
    int sd_b = 0, sd_e = 0;
    if (reward_mode == CCX_K_REWARD_DEFAULT) {
        cls_b = dest_b ? 1 : at_door ? 2 : in_area ? 3 : 0;
        cls_e = dest_e ? 1 : !in_area ? 3 : 0;
        sd_b = -(adx + (g.div - y));
        sd_e = adx + (y - g.div);
    } else if (reward_mode == CCX_K_REWARD_SIMPLE_DISTANCE) {
        cls_b = cls_e = 0;
        sd_b = -(y > g.bdy ? y - g.bdy : g.bdy - y);
        sd_e = -(y > g.edy ? y - g.edy : g.edy - y);
    }
    const uint32_t tb = term_b < 0 ? (dest_b ? 1u : 0u) : (term_b != 0 ? 1u : 0u);
    const uint32_t te = term_e < 0 ? (dest_e ? 1u : 0u) : (term_e != 0 ? 1u : 0u);
    const uint32_t nib_b = (dest_b ? 1u : 0u) | (cls_b << kCellClassShift) | (tb << kCellTermShift);
    const uint32_t nib_e = (dest_e ? 1u : 0u) | (cls_e << kCellClassShift) | (te << kCellTermShift);
    lo |= (in_area ? kCellInTram : 0u) | (at_door ? kCellAtDoor : 0u) | (nib_b << kCellBoardingShift) |
          (nib_e << kCellExitingShift) | cell_xy_bytes((uint32_t)x, (uint32_t)y);
    const uint32_t hi = (((uint32_t)sd_b & 0xFFFFu) << kCellDistBoardingShift) | (((uint32_t)sd_e & 0xFFFFu) << kCellDistExitingShift);
    return (unsigned long long)lo | ((unsigned long long)hi << 32);
}

// accessors.  `tsh` / `tsh2`: where an agent's type finds its nibble in the low word / its distance in the high word
CCX_HD uint32_t cell_tsh(bool boarding) { return boarding ? kCellBoardingShift : kCellExitingShift; }
CCX_HD uint32_t cell_tsh2(bool boarding) { return boarding ? kCellDistBoardingShift : kCellDistExitingShift; }
CCX_HD uint32_t cell_legal(uint32_t lo, uint32_t a) { return (lo >> a) & 1u; }                 // a = 0..4 (4 = wait: never)
CCX_HD uint32_t cell_legal4(uint32_t lo) { return lo & kCellLegalMask; }                       // bit a = move a is legal
CCX_HD uint32_t cell_info_flags(uint32_t lo) { return (lo >> kCellInfoShift) & kCellInfoMask; }   // as they sit in the flag byte
CCX_HD uint32_t cell_x(uint32_t lo) { return (lo >> kCellXShift) & kCellByteMask; }
CCX_HD uint32_t cell_y(uint32_t lo) { return lo >> kCellYShift; }
CCX_HD uint32_t cell_at_dest(uint32_t lo, uint32_t tsh) { return (lo >> tsh) & 1u; }             // :663-683
CCX_HD uint32_t cell_terminated(uint32_t lo, uint32_t tsh) { return (lo >> (tsh + kCellTermShift)) & 1u; }   // terminateds[id] as the cell says
CCX_HD uint32_t cell_class(uint32_t lo, uint32_t tsh) { return (lo >> (tsh + kCellClassShift)) & kCellClassMask; }
CCX_HD int cell_distance(uint32_t hi, uint32_t tsh2) { return (int)(int16_t)(uint16_t)(hi >> tsh2); }

// ---- 2. the reward (rewards.py:44-182) ---------------------------------------------------------------------------------
// the constant of class 1 per reward mode; classes 2 / 3 are tram_door_reward / tram_area_reward, class 0 scales by
// distance_penalty_factor
template <typename P>   // (reward_mode, r_dest, r_nogoal, r_pen of KParams, or of the kernel-argument segment's copy)
CCX_HD double reward_class_a(const P& p) {
    return p.reward_mode == CCX_K_REWARD_BINARY ? p.r_nogoal : p.reward_mode == CCX_K_REWARD_CONSTANT_NEGATIVE ? p.r_pen : p.r_dest;
}
// Distances are integers and the reference negates the INTEGER before the one f64 multiply, so d == 0 gives +0.0 (never -0.0).
CCX_HD double cell_reward(uint32_t lo, uint32_t hi, uint32_t tsh, uint32_t tsh2, double rA, double rB, double rC, double rF) {
    const uint32_t cls = cell_class(lo, tsh);
    const int sd = cell_distance(hi, tsh2);
    double r = (double)sd * rF;
    r = (cls == 1u) ? rA : r;
    r = (cls == 2u) ? rB : r;
    r = (cls == 3u) ? rC : r;
    return r;
}
CCX_HD double reward_if_live(double r, uint32_t live) { return live ? r : 0.0; }                 // rewards.py:64: None unless live

// ---- 3. the flag bytes (include/ccx.h: CCX_AF_*, CCX_EF_*; collectivecrossing.py:214-259) ----------------------------
// out2 = the flags this step raises (terminated | truncated << 1), flags_before = the same pair BEFORE the step.
// live = neither flag was set before the step (rewards.py:64, truncateds.py:56); obs = live, or a flag is newly set by this
// step (:243, :763-767); the cell's own info bits; active (0/1); the destination bit.
CCX_HD uint32_t agent_live(uint32_t flags_before) { return flags_before == 0u ? 1u : 0u; }
CCX_HD uint32_t agent_flag_byte(uint32_t out2, uint32_t flags_before, uint32_t lo, uint32_t tsh, uint32_t act) {
    const uint32_t live = agent_live(flags_before);
    const uint32_t emit = (live | (out2 & ~flags_before)) != 0u ? 1u : 0u;
    return out2 | (live << 2) | (emit << 3) | cell_info_flags(lo) | (act << 6) | (cell_at_dest(lo, tsh) << 7);
}
// the env byte: ef = CCX_EF_ALL_TERMINATED | CCX_EF_ALL_TRUNCATED as raised; reset_bit = CCX_K_EF_RESET where an env that
// raises __all__ restarts from the pool, else 0: the bit appears next to a raised flag only
CCX_HD uint32_t env_flag_byte(uint32_t ef, uint32_t reset_bit) { return ef + (ef < 1u ? ef : 1u) * reset_bit; }

// ---- 4. the reset-pool cursor (include/ccx.h: ccx_set_reset_pool) -------------------------------------------------------
// entry of episode `episode` of global env `global_env` in a pool of P entries: (g + j * stride) mod P without overflow
// (P < 2^31).  stride = total_envs mod P, or 1 when P divides total_envs.
CCX_HD unsigned long long pool_stride_of(unsigned long long total_envs, unsigned long long P) {
    const unsigned long long s = total_envs % P;
    return s == 0ull ? 1ull % P : s;
}
CCX_HD unsigned long long pool_entry(unsigned long long global_env, unsigned long long episode, unsigned long long stride,
                                     unsigned long long P) {
    const unsigned long long gi = global_env % P;
    const unsigned long long ep = episode % P;
    return (gi + ep * stride) % P;
}

}  // namespace ccx
