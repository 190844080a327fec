// ccx_plan.hip -- launch-shape selection: a pure function of the batch, the grid, the caller's overrides and the device's CU
// count.  Host arithmetic only: no runtime call, no handle, no allocation, no environment.  ccx_api.hip (choose_shape) feeds
// it from a handle and applies the result; tests/test_shape_plan.py replays a recorded table of decisions through it on
// a machine without a GPU.
// The second function, plan_call / plan_launch at the end of the file, decides what is decided per CALL on top of a handle's
// two planned shapes: how the call is cut into launches, which kernel takes each launch and how that launch is driven (pacing,
// hand-off, rounds, what the step launch fuses).  ccx_api.hip asks it before every launch; tests/test_call_plan.py holds it
// against an independent restatement of the rules over a sweep, sizes no test could allocate included.
//
// A tile (EW envs) is served by a sim wave and, when outputs are written, writer waves on other SIMDs; one step of a tile
// is a latency chain of ~1.5k cycles whatever EW is, so the batch should be cut into at least ~512 tiles (1024 waves = one
// per SIMD of the 256 CUs) before tiles are made fuller.  Measured on 4096 envs x 8 agents: 64 lanes/wave (512 tiles)
// 0.252 ms per 250 steps, 32 lanes 0.280 ms, 16 lanes 0.344 ms.
// rows: the shape of launches that write observation rows (paced, sized for the row stream); !rows: the shape of launches
// without them (rewards, flag bytes, compact rows -- bound by the sim chain and by how many tiles are resident,
// profiles/r04_shape_sweep.json).
#include "ccx_plan.h"

#include <algorithm>
#include <cmath>
#include <cstdio>

#include "../../include/ccx.h"

namespace ccxp {

#ifdef CCX_PLAN_COVERAGE   // diagnostic build: how often each rule branch is taken (tests/golden/gen_shape_plan_golden.py --coverage)
#define CCXP_BRANCHES(X)                                                                                                   \
    X(lanes_override) X(lanes_default) X(tables_shrink_tile) X(tables_dropped_for_rounds) X(small_batch) X(half_tiles)     \
    X(writers_override) X(writers_no_rows) X(writers_small_batch) X(writers_large_tiles) X(writers_small_tiles)            \
    X(writers_between) X(tpb_override) X(tpb_single) X(tpb_no_rows_one_writer) X(tpb_pairs) X(one_round_one_writer)        \
    X(several_rounds_two_writers) X(several_rounds_one_writer) X(two_writer_class_many_rounds) X(block_thread_limit)       \
    X(singles_over_pairs) X(big_cell_table) X(big_cell_table_fuller) X(pair_rows) X(pair_rows_no_room)                     \
    X(tables_cost_tiles_per_block) X(tables_too_big_or_off) X(single_agent_tables_dropped) X(ring_16) X(ring_32)          \
    X(write_window_big) X(write_window_small) X(step_lanes_override) X(step_lanes_halved) X(step_kernel_refused)          \
    X(unpaced) X(paced) X(pace_fixed) X(pace_caller) X(pace_assumed)
enum {
#define CCXP_X(name) COVER_##name,
    CCXP_BRANCHES(CCXP_X)
#undef CCXP_X
    COVER_COUNT
};
long long g_cover[COVER_COUNT];
#define CCXP_COVER(name) (++g_cover[COVER_##name])
#else
#define CCXP_COVER(name) ((void)0)
#endif

int ceil_log2(int n) {
    int g = 0;
    while ((1 << g) < n) ++g;
    return g;
}

uint32_t to_fp(double ns) {
    const double v = ns / 10.0 * 256.0;
    return (uint32_t)(v < 1.0 ? 1.0 : (v > 4.0e9 ? 4.0e9 : v));
}

namespace {

constexpr size_t kLdsCu = 160u * 1024u;       // LDS of a CU
constexpr size_t kLdsTables = 96u * 1024u;    // a workgroup that keeps occupancy tables stays below this
constexpr size_t kWSlotBytes = 1056u;         // a writer wave's staging slot (ccx_rollout_dev.h: WSlot)

size_t cells_of(const PlanIn& in) { return (size_t)(in.width + 3) * (size_t)(in.height + 3); }
size_t mask_bytes(int glog) { return glog == 6 ? 8u : 4u; }
int units_of(const PlanIn& in, int ew) { return ew * in.N * (3 + 2 * in.N); }
int store_units(const PlanIn& in, int ew) { return (in.N % 2 == 0) ? units_of(in, ew) / 2 : units_of(in, ew); }
double tile_step_bytes(const PlanIn& in, int ew) { return (double)ew * in.N * (4.0 * (6 + 4 * in.N) + 10.0) + ew; }
int tiles_of(const PlanIn& in, int ew) { return (in.E + ew - 1) / ew; }

}  // namespace

LdsLayout lds_layout(const PlanIn& in, uint32_t ring_slots, size_t writer_slots, int tiles_per_block, int ew, bool with_tables) {
    const size_t cells = cells_of(in);
    LdsLayout l;
    l.occ_bytes = up16((size_t)ew * 2u * (cells + 1u) * mask_bytes(ceil_log2(in.N)));
    l.table = up16(((size_t)ew * in.N * (3 + 2 * in.N) + 2u) * 2u);
    l.off_tiles = up16(cells * 8u) + (in.reward_table ? up16(cells * 16u) : 0u);   // user reward table behind the cell table
    l.off_ws = ccx::tile_head_bytes(ring_slots);                                   // xch + hand-off words + stage ring
    l.off_occ = l.off_ws + writer_slots * kWSlotBytes;                             // WSlot(s) per writer
    l.tile_stride = up16(l.off_occ + (with_tables ? l.occ_bytes : 0));
    l.total = l.off_tiles + (size_t)tiles_per_block * l.tile_stride + l.table;
    return l;
}

size_t rounds(size_t tiles, size_t bytes_per_block, int tiles_per_block, int waves_per_block, int wave_cap, size_t max_per_cu,
              int num_cus) {
    const size_t by_waves = std::min<size_t>((size_t)(wave_cap / waves_per_block), max_per_cu);
    const size_t blocks = std::max<size_t>(1, std::min<size_t>(kLdsCu / std::max<size_t>(bytes_per_block, 1), by_waves));
    const size_t at_once = blocks * (size_t)tiles_per_block * (size_t)num_cus;
    return (tiles + at_once - 1) / at_once;
}

namespace {

constexpr size_t kNoCap = (size_t)1 << 20;

// what the rules below share: the inputs, what has been decided so far
struct Work {
    const PlanIn& in;
    int glog, G, max_ew;
    bool rows;
    bool drop_tables = false, small_batch = false, half_tiles = false, small_tiles = false;
    int ew = 1, tiles = 0, n4 = 0, writers = 0, tpb = 1;
    size_t wsw = 1;                                   // staging slots per writer
    LdsLayout lay(uint32_t ring, int tiles_pb, bool with_tables) const {
        return lds_layout(in, ring, (size_t)writers * wsw, tiles_pb, ew, with_tables);
    }
};

// Envs per wave.  Prefer the O(1) occupancy-table conflict masks: carry fewer envs per wave when that makes the per-env
// tables fit in LDS (only grids too large even for one env per wave fall back to the all-pairs compare).
void pick_envs_per_wave(Work& w) {
    const PlanIn& in = w.in;
    int ew;
    if (in.lanes_per_wave > 0) {
        CCXP_COVER(lanes_override);
        ew = in.lanes_per_wave / w.G;
    } else {
        CCXP_COVER(lanes_default);
        const int target_tiles = 512;
        ew = w.max_ew;
        while (ew > 1 && (in.E + ew - 1) / ew < target_tiles) ew >>= 1;
    }
    ew = std::max(1, std::min(ew, w.max_ew));
    if (in.lanes_per_wave == 0) {
        // (seven writer slots, whatever the writer count will be)
        auto need = [&](int e) { return lds_layout(in, 16, 7, 1, e, true); };
        // The tables cost LDS -- one per env, (cells + 1) x 8 bytes -- and LDS is what bounds how many tiles a CU holds: a 24 x 16
        // grid keeps three 8-env tiles per CU where five fit without tables, a 64 x 48 grid ONE two-env tile; single-agent envs
        // on 12 x 8 one 64-env tile.  A batch that needs more ROUNDS because of them pays a round's time for each (64 x 48,
        // 8 agents: 0.18-0.24 of the HBM peak with tables, 0.51-0.63 without; 24 x 16, 16 384 envs: 0.69 vs 0.93;
        // profiles/r04_big_grid_scan.txt).  The all-pairs masks cost the sim chain ~5.5 % per lane of the group (8 agents:
        // 0.47 vs 0.34 us per env-step; 32: 2.8 x).  For groups of <= 16 lanes the tables go (and the tile keeps its lanes)
        // where the rounds saved outweigh that (16 agents on 64 x 48: 0.25-0.35 of the peak with tables -- one 16-lane tile per
        // CU --, 0.77-0.88 without).
        int ew_fit = ew;
        if (need(1).total <= kLdsTables) while (ew_fit > 1 && need(ew_fit).total > kLdsTables) ew_fit >>= 1;
        if (w.glog <= 4 && in.occ_tables < 0) {
            const LdsLayout fit = need(ew_fit), full = need(ew);
            const size_t with_tables = rounds((size_t)tiles_of(in, ew_fit), fit.total, 1, 1, 5, 5, in.num_cus);
            const size_t without = rounds((size_t)tiles_of(in, ew), full.total - full.occ_bytes, 1, 1, 5, 5, in.num_cus);
            if ((double)without * (1.0 + 0.055 * w.G) < (double)with_tables) w.drop_tables = true;
        }
        if (w.drop_tables) CCXP_COVER(tables_dropped_for_rounds);
        else if (ew_fit != ew) CCXP_COVER(tables_shrink_tile);
        if (!w.drop_tables) ew = ew_fit;
    }
    w.ew = ew;
}

// Batches too small to be memory-bound (round 2): one env-step of a tile takes the sim chain's ~0.5 us
// whatever the tile holds, so what counts is that no writer wave takes longer than that and that every
// wave has a SIMD of its own.  Full 64-lane tiles with TWO writer waves each do both as long as
// 3 waves x tiles stays near the 1024 SIMDs: C2 geometry, us per env-step, full tiles + 2 writers vs the
// half-empty single-writer tiles chosen before: 1024 envs 0.53 vs 0.58, 2048 envs 0.54 vs 0.59 (0.63 vs
// 0.58 of the HBM peak), 3072 envs 0.63 vs 0.72 (0.81 vs 0.70).
void classify_small_batch(Work& w) {
    const PlanIn& in = w.in;
    if (!(in.lanes_per_wave == 0 && in.writers != 1 && in.waves_per_block == 0)) return;
    const long long full_tiles = (in.E + w.max_ew - 1) / w.max_ew;
    const int full_n4 = store_units(in, w.max_ew);
    if (!(full_n4 <= 64 * 12 && full_tiles * (1 + (in.writers > 0 ? in.writers : 2)) <= 1400 && full_tiles * w.max_ew >= 256)) return;
    // (only if the LDS tables of a full tile fit, with the writer slots of the writer count chosen below -- up to four for
    // small batches: a check against two let a 6 x 16 grid with one agent per env through whose full tile then lost its
    // occupancy tables, and with them the in-kernel policies; found by the round-3 hypothesis soak)
    if (lds_layout(in, 16, (size_t)(in.writers > 0 ? in.writers : 4), 1, w.max_ew, true).total > kLdsTables) return;
    CCXP_COVER(small_batch);
    w.small_batch = true;
    w.ew = w.max_ew;
    // Up to 128 full tiles (C2 geometry: 1024 envs) half the CUs would stand idle: HALF tiles with four writers
    // each put a tile on every CU and halve each writer's share (round 3, us per env-step with full outputs:
    // 1024 envs 0.355 vs 0.398-0.402 with full tiles and 3-4 writers, 512 envs 0.353 vs 0.395).  What remains
    // is the step's own latency chain sim -> hand-off -> writer (~0.35 us), not bytes.
    // (round 4 sweep: only where a full tile has >= 9 store iterations per step -- with fewer the row work is too
    // small to be worth two half-width sim waves: 3 agents, 256-2048 envs 0.37-0.39 vs 0.34 us per env-step)
    if (full_tiles <= 128 && w.max_ew >= 2 && in.writers == 0 && (!w.rows || full_n4 >= 64 * 9)) {
        CCXP_COVER(half_tiles);
        w.ew = w.max_ew / 2;
        w.half_tiles = true;
    }
}

// Writer waves per tile (round 4: re-derived from the E x N x output-mode sweep, profiles/r04_shape_sweep.json, which
// measures every (lanes, writers) candidate per point; the tables of DESIGN.md 4 are that file).
//
// Launches WITHOUT observation rows (rewards / flag bytes / compact rows: bound by the sim chain and by how many tiles
// are resident): two writers split by role, ONE from 1024 tiles on (8 agents, 16 384 envs: 0.55 vs 0.91 us per
// env-step with two; 32 agents, 32 768 envs: 4.1 vs 6.3) -- lane groups of 32 / 64 only from 16 384 tiles on (their
// compact rows keep a second writer busy), single-agent envs never (one writer: +30-40 %); with 257-512 tiles -- one
// per two SIMDs, C2's 4096 envs -- FOUR writers in one-tile workgroups (the two spare waves only poll): every agent
// count of the sweep is 4-6 % faster than with two (8 agents, 4096 envs: 0.319 vs 0.338 us per env-step;
// profiles/scratch/calls/r04_call19.sh, r04_call21.sh).
int writers_no_rows(int glog, int tiles) {
    if (tiles > 256 && tiles <= 512) return 4;   // one tile per two SIMDs: five-wave workgroups, one tile each
    return glog <= 2 ? 2 : glog <= 4 ? (tiles > 1280 ? 1 : 2) : (tiles >= 1500 ? 1 : 2);
}

// Small batches (unpaced, full or half tiles): writer 0 = small outputs, the others share the observation rows
// (KParams::writer0_small); three writers while 4 waves x tiles still fit the 1024 SIMDs (2048-env C2: 0.54 -> 0.485 us per
// step); round 3, with the sim chain at 0.27 us and the writer loops compiled per role: four writers up to 160 tiles (1024
// envs 0.39 -> 0.41 of the peak), three beyond (2048 envs: 0.81-0.82 with three, 0.80-0.81 with four).
int writers_small_batch(bool half_tiles, int tiles) { return half_tiles || tiles <= 160 ? 4 : 3; }

// Small tiles (<= 12 store iterations per step): with <= 8 iterations per tile (1-3 agents) THREE writers whatever the
// batch (3 agents, 8192 envs 0.38 vs 0.47 us with two; N = 1, 65 536 envs: 1.17 vs 2.40 us with the single throttled
// writer of rounds 1-3); with 9-12 iterations (C2's class) two writers split by role up to four tiles per CU (two six-wave
// workgroups; the rule used to read "while 3 waves per tile fit one round", i.e. up to 1365 tiles, and every batch of
// 8193 .. 10 920 envs of C2 ran at 0.49 of the peak with a third workgroup on some CUs: profiles/r04_ragged_c2.txt) --
// in pairs up to two tiles per CU (C2's 4096 envs), THREE in one-tile workgroups from there to four (5000 .. 8192 envs:
// 0.92-0.94 vs 0.89-0.93 with two, two runs of that table) --, beyond that ONE throttled writer as before: the sweep's
// short launches put three within 2 % of it, but the bench's settled launches do not (C2 geometry, secondary.workloads:
// 16 384 envs 0.881 vs 0.845 of the peak with three, 65 536 envs 0.818 vs 0.747).  TWO writers are a cliff in several
// rounds (6-wave workgroups: +35-80 %).
// (With everything on one writer C2's 4096 x 8 had 1580 clocks of work per step next to the sim's 1200 and held the tile at
// ~0.72 us per step -- bound by its writer wave, not by memory; with two the pace follows the memory side down to ~0.70 us:
// 0.86 -> 0.92 of the HBM peak in one call.)
int writers_small_tiles(int n4, int tiles, int num_cus) {
    return n4 <= 64 * 8 ? 3 : tiles <= 2 * num_cus ? 2 : tiles <= 4 * num_cus ? 3 : 1;
}

// writer waves per tile: enough that a writer handles <= ~6 store iterations per step.  Large tiles (> 24 store iterations
// per step): 3; tiles in between: 2, or 1 + four tiles per workgroup when that makes the batch fit one round (below).
int default_writers(const Work& w) {
    if (w.in.writers > 0) { CCXP_COVER(writers_override); return w.in.writers; }
    if (!w.rows) { CCXP_COVER(writers_no_rows); return writers_no_rows(w.glog, w.tiles); }
    if (w.small_batch) { CCXP_COVER(writers_small_batch); return writers_small_batch(w.half_tiles, w.tiles); }
    if (w.n4 > 64 * 24) { CCXP_COVER(writers_large_tiles); return 3; }
    if (w.small_tiles) { CCXP_COVER(writers_small_tiles); return writers_small_tiles(w.n4, w.tiles, w.in.num_cus); }
    CCXP_COVER(writers_between);
    return 2;
}

// tiles per workgroup: two small tiles share one cell table / one CU slot (with the throttle:
// 4.43e9 vs 4.23e9 env-steps/s on C2; 3 or 4 per workgroup leave CUs idle and lose 5-10 %)
int default_tiles_per_block(const Work& w) {
    const PlanIn& in = w.in;
    if (in.waves_per_block > 0) { CCXP_COVER(tpb_override); return in.waves_per_block; }
    if (w.small_batch || (!w.rows && w.writers == 4)) { CCXP_COVER(tpb_single); return 1; }
    // without rows (profiles/r04_noobs_scan.txt): two-writer tiles NEVER in pairs (six-wave workgroups: 0.45 vs 0.36 us
    // per env-step from 375 tiles on -- every batch between 2049 and 8191 envs of C2 but 4096), one-writer tiles in
    // pairs from 1500 tiles on (32 agents, 8192 envs: 1.07 vs 1.31 us)
    if (!w.rows && w.writers == 2) { CCXP_COVER(tpb_single); return 1; }
    if (!w.rows && w.writers == 1) { CCXP_COVER(tpb_no_rows_one_writer); return w.tiles >= 1500 ? 2 : 1; }
    // (one round of two-wave workgroups: +1-3 % over pairs, 10 000 .. 16 384 envs of C2)
    if (w.rows && w.small_tiles && w.writers == 1 && w.tiles <= 8 * in.num_cus) { CCXP_COVER(tpb_single); return 1; }
    if (w.rows && w.small_tiles && w.n4 > 64 * 8 && w.writers == 3) { CCXP_COVER(tpb_single); return 1; }
    // (never two writers in pairs: six-wave workgroups, 16 agents x 36 032 envs ran at 0.47)
    if ((w.tiles > 8192 && w.writers != 2) || (w.small_tiles && w.tiles >= 512)) { CCXP_COVER(tpb_pairs); return 2; }
    CCXP_COVER(tpb_single);
    return 1;
}

// One round beats two (round 2): a CU holds 16 wavefronts of this kernel (4 per SIMD at its ~100
// VGPRs).  If the batch needs more than that with the writer count above but fits with ONE writer
// wave per tile, and that writer's share stays <= 36 store iterations per step, every tile is
// resident for the whole launch and the tiles of a step sweep the slab exactly once -- C3 (4096 x 32:
// 2048 tiles x 4 waves = two rounds) 0.84 -> 0.87 of the HBM peak with 1 writer and 4 tiles per
// workgroup.  (C5, 67 KB per tile, already fits one round with 3 writers; one writer is too slow there.)
void several_rounds_rule(Work& w) {
    const PlanIn& in = w.in;
    if (!(w.rows && in.writers == 0 && in.waves_per_block == 0 && !w.small_tiles)) return;
    const long long cap = 16ll * in.num_cus;
    if ((long long)w.tiles * (1 + w.writers) > cap && (long long)w.tiles * 2 <= cap && w.n4 <= 64 * 36) {
        CCXP_COVER(one_round_one_writer);
        w.writers = 1;
        w.tpb = 4;
    } else if ((long long)w.tiles * (1 + w.writers) > cap && w.writers == 3 && w.n4 <= 64 * 36) {
        // several rounds anyway: two writers in one-tile workgroups keep five tiles per CU resident instead of four (C3
        // geometry, 8192 envs: 21.7 vs 25.2 us per env-step; 32 768 envs 1.01).  NOT with two tiles per workgroup:
        // six-wave workgroups leave a quarter of a CU's 16 wave slots empty (+40 % at 32 768 envs)
        // From 8192 tiles on ONE writer (eight tiles per CU resident): 16 384 envs 44.2 vs 49.3 us, 32 768 envs 90 vs 100.
        if (w.tiles < 8192) {
            CCXP_COVER(several_rounds_two_writers);
            w.writers = 2;
            w.tpb = 1;
        } else {
            CCXP_COVER(several_rounds_one_writer);
            w.writers = 1;
        }
    } else if (w.writers == 2 && w.tiles >= 8192 && w.n4 <= 64 * 36) {
        // the two-writer class (13-24 store iterations per tile: 12-20 agents) in many rounds: the same one writer, in
        // pairs (20 agents on 24 x 16, 32 768 envs: 0.74 vs 0.42 of the peak; 40 x 30: 0.70 vs 0.65;
        // profiles/r04_big_grid_scan.txt)
        CCXP_COVER(two_writer_class_many_rounds);
        w.writers = 1;
        w.tpb = 2;
    }
}

// Tile PAIRS hold fewer tiles per CU than single tiles where the waves are what bounds them (three writers: two
// eight-wave workgroups = 4 tiles against five four-wave ones): a batch that fits one round of singles but not of pairs
// takes singles (4 agents x 17 776 envs: 0.94 vs 1.40 us per env-step; profiles/r04_rows_456.txt).
void singles_over_pairs_rule(Work& w) {
    const PlanIn& in = w.in;
    if (!(in.writers == 0 && in.waves_per_block == 0 && w.tpb == 2 && w.lay(16, 1, false).off_tiles < 24u * 1024u)) return;
    auto rounds_tpb = [&](int t) {
        return rounds((size_t)w.tiles, w.lay(16, t, !w.drop_tables).total, t, t * (1 + w.writers), 20, kNoCap, in.num_cus);
    };
    if (rounds_tpb(1) < rounds_tpb(2)) {
        CCXP_COVER(singles_over_pairs);
        w.tpb = 1;
    }
}

// A CELL table that fills much of the LDS by itself (64 x 48: 27 KB, 80 x 60: 39 KB, 100 x 100: 85 KB -- one per
// workgroup) limits the workgroups per CU, and then the tiles per workgroup decide how much of the batch is resident:
// 100 x 100, 8 agents, 16 384 envs in one-tile workgroups = 256 tiles at a time, 0.35 of the HBM peak and 3.9 us per
// env-step without rows; four one-writer tiles per workgroup = 1024 at a time, 0.85 and 0.90 us
// (profiles/r04_big_grid_scan.txt).  Among the rule's own (writers, tiles) and the fuller workgroups -- the same writers
// with more tiles, ONE writer with up to four -- the one that needs the fewest rounds is taken (ties: the rule's writers,
// then fewer tiles per workgroup).
void big_cell_table_rule(Work& w) {
    const PlanIn& in = w.in;
    if (!(in.writers == 0 && in.waves_per_block == 0 && w.lay(16, 1, false).off_tiles >= 24u * 1024u)) return;
    CCXP_COVER(big_cell_table);
    auto rounds_with = [&](int writers, int t) {
        Work c = w;
        c.writers = writers;
        LdsLayout l = c.lay(16, t, !w.drop_tables);
        if (l.total > kLdsTables) l = c.lay(16, t, false);      // (tables that do not fit are not kept: below)
        if (l.total > kLdsCu) return (size_t)1 << 30;
        return rounds((size_t)w.tiles, l.total, t, t * (1 + writers), 16, kNoCap, in.num_cus);
    };
    int best_w = w.writers, best_t = w.tpb;
    size_t best = rounds_with(w.writers, w.tpb);
    for (int pass = 0; pass < 2; ++pass) {
        const int writers = pass == 0 ? w.writers : 1;
        for (int t = (pass == 0 ? w.tpb + 1 : 2); t * (1 + writers) <= 8; ++t) {
            const size_t r = rounds_with(writers, t);
            if (r < best) { best = r; best_w = writers; best_t = t; }
        }
    }
    if (best_w != w.writers || best_t != w.tpb) CCXP_COVER(big_cell_table_fuller);
    w.writers = best_w;
    w.tpb = best_t;
}

// The LDS carve-up (see ccx_kernels.hip): [cell table][tiles][u16 obs table]; decides the staging slots per writer, whether
// the occupancy tables stay, and the ring slots.  Fills the layout fields of p.kp and the LDS fields of p.shape.
void finish_layout(Work& w, ShapePlan& p) {
    const PlanIn& in = w.in;
    // Small batches (unpaced, writers split by role): a second staging slot per writer lets a row writer take TWO steps
    // per iteration whenever the sim wave is that far ahead (ccx_rollout_body.inc) -- if the LDS has the room.
    // (by default only with half tiles, <= 1024 envs of the C2 geometry: +3 % there; at 2048 envs the unpaced write stream is
    // the limit and two steps' stores back to back cost it 5-7 %: tunable pair_rows = 1 forces it for every small batch)
    if (w.small_batch && w.writers >= 2 && (in.pair_rows == 1 || (in.pair_rows < 0 && w.half_tiles))) {
        w.wsw = 2;
        if (w.lay(16, w.tpb, !w.drop_tables).total > kLdsTables) { CCXP_COVER(pair_rows_no_room); w.wsw = 1; }
        else CCXP_COVER(pair_rows);
    }
    const bool tables_can_fit = w.lay(16, 1, !w.drop_tables).total <= kLdsTables;   // (with one tile per workgroup; a 100 x 100 grid: never)
    if (in.waves_per_block == 0 && tables_can_fit)                                  // a default never costs the occupancy tables their LDS
        while (w.tpb > 1 && w.lay(16, w.tpb, !w.drop_tables).total > kLdsTables) { CCXP_COVER(tables_cost_tiles_per_block); --w.tpb; }
    LdsLayout l = w.lay(16, w.tpb, !w.drop_tables);
    int occ = 1;
    if (l.total > kLdsTables || in.occ_tables == 0 || w.drop_tables) {   // tables too big (or switched off, or given up for residency): all-pairs conflict masks instead
        CCXP_COVER(tables_too_big_or_off);
        occ = 0;
        l = w.lay(16, w.tpb, false);
    }
    // Single-agent envs: a table of (cells + 1) entries per env, 64 envs per wave -- 73 KB for a 12 x 8 grid, ONE tile per CU:
    // a batch of more than 64 x CUs envs ran in rounds at twice the time per env-step (17 768 envs: 0.83 us against 0.43 at
    // 15 800).  An agent alone in its env collides with nobody; the all-pairs masks cost it three VALU ops (+4 % while the
    // tables fit one round, half the time when they do not: profiles/r04_occ_tables.txt).
    const size_t num_blocks = (size_t)((w.tiles + w.tpb - 1) / w.tpb);
    if (occ && in.occ_tables < 0 && (w.drop_tables || (w.glog == 0 && num_blocks > (kLdsCu / l.total) * (size_t)in.num_cus))) {
        CCXP_COVER(single_agent_tables_dropped);
        occ = 0;
        l = w.lay(16, w.tpb, false);
    }
    // The hand-off ring takes 32 slots (8 KB) -- or 16 where that costs a CU a resident workgroup: LDS is what bounds the
    // residency of the big-tile shapes (C5-64: 40 KB per workgroup with 4 KB of ring, four per CU; with 8 KB only three).
    // (The sim wave proves "slot free" from a progress value it reads once per 16-step burst: 16 slots are the minimum
    // for which that stale value suffices almost always.)
    const size_t fit16 = std::min<size_t>(kLdsCu / l.total, 16u);
    uint32_t slots = ccx::kMaxStageSlots;
    l = w.lay(slots, w.tpb, occ != 0);
    if (l.total > 150u * 1024u || std::min<size_t>(kLdsCu / l.total, 16u) < fit16) slots = 16;
    if (slots == 16) CCXP_COVER(ring_16); else CCXP_COVER(ring_32);
    l = w.lay(slots, w.tpb, occ != 0);
    p.shape.occ = occ;
    p.shape.lds_bytes = l.total;
    p.shape.lds_bytes_observe = up16((size_t)w.tpb * kWSlotBytes + l.table);
    ccx::KParams& k = p.kp;
    k.off_tiles = (uint32_t)l.off_tiles; k.tile_stride = (uint32_t)l.tile_stride;
    k.off_ws = (uint32_t)l.off_ws; k.off_occ = (uint32_t)l.off_occ;
    k.occ_words = occ ? (uint32_t)(l.occ_bytes / 4u) : 0u;
    k.off_table = (uint32_t)(l.off_tiles + (size_t)w.tpb * l.tile_stride);
    k.stage_slots = slots;
    k.ws_per_writer = (uint32_t)w.wsw;
}

// Write-window defaults (measured round 2).  Large tiles (tens of KB per tile and step:
// C3, C5) drain 5-10 % faster when the tiles of a round are phased over the step
// period in tile order and groups of 16 adjacent tiles go to one XCD, dealt round-robin: the chip then
// writes one window that sweeps through the slab instead of 1000+ regions at once (C3 0.80 -> 0.86,
// C5-64 0.79 -> 0.89, C5-50 0.77 -> 0.83 of the HBM peak in one call).  Small tiles (C2: 10 KB per tile
// and step) show no difference while there are two of them per CU (4096 envs) and keep the common phase and
// the XCD-contiguous mapping; LARGER batches of small tiles are 1000+ regions at once again and gain the same
// way (C2 geometry, one call: 16 384 envs 0.879 -> 0.908, 32 768 envs in two rounds 0.830 -> 0.882).
void write_window(const Work& w, ccx::KParams& k) {
    const PlanIn& in = w.in;
    const bool big_tiles = !w.small_tiles || (long long)w.tiles >= 4ll * in.num_cus;
    k.pace_phase = (uint32_t)(in.pace_phase >= 0 ? in.pace_phase : (big_tiles ? 1 : 0));
    // groups of ~1 MiB of one step's slab per XCD: g workgroups with g * (bytes a workgroup writes per step)
    // closest to 1 MiB, a power of two in 1..32 (C5-64: 16 x 67 KB, C3: 8 x 137 KB)
    int auto_map = 0;
    if (big_tiles) {
        CCXP_COVER(write_window_big);
        const double wg_bytes = tile_step_bytes(in, w.ew) * w.tpb;
        int g = 1;
        while (g < 32 && wg_bytes * g * 1.41 < 1048576.0) g <<= 1;
        auto_map = 1;
        while ((1 << (auto_map - 1)) < g) ++auto_map;
    } else {
        CCXP_COVER(write_window_small);
    }
    k.tile_map = (uint32_t)(in.tile_map >= 0 ? in.tile_map : auto_map);
}

// Short launches (<= 16 steps, ccx_step.hip): a workgroup = one tile = a sim wave + row waves, as many tiles as the
// batch fills, halved only while there are fewer than one per two CUs (a one-step launch is bound by how fast its waves are
// dispatched and drained: with the row waves' table words preloaded, 512 tiles of 64 lanes + 2 row waves step C2's 4096 envs
// in 3.64 us, 1024 tiles of 32 + 1 in 3.72; 512 envs: 128 tiles of 32 lanes 3.04 us, 512 tiles of 8 lanes 3.30;
// profiles/r04_step_k1_shapes_*.txt, r04_step_scan.txt), never more envs per wave than the rollout shape (the observation address
// table of a smaller tile is a prefix of the rollout's).  Row waves: enough that one handles <= ~6 store iterations per step
// (small tiles) or 10-14 (large ones), at most 5 (C5-64: 14.9 us with five, 15.5 with seven).  Grids whose tables exceed
// the LDS keep the rollout kernel.
ccx::StepShape plan_step_shape(const PlanIn& in, int glog, int ew) {
    const int G = 1 << glog, cells = (int)cells_of(in);
    ccx::StepShape ss{};
    int sew = ew;
    if (in.step_lanes > 0) {
        CCXP_COVER(step_lanes_override);
        sew = std::max(1, std::min(ew, in.step_lanes / G));
    } else {
        while (sew > 1 && ((in.E + sew - 1) / sew < in.num_cus / 2 ||      // (profiles/r04_step_scan.txt)
                           ccx::step_lds_bytes(glog, sew, in.N, cells, in.reward_table != 0) > kLdsTables)) {
            CCXP_COVER(step_lanes_halved);
            sew >>= 1;    // (... and until the tile's tables fit: 40 x 30, 4096 envs took the rollout kernel for 8 KB)
        }
    }
    ss.glog = glog;
    ss.envs_per_wave = sew;
    ss.lds_bytes = ccx::step_lds_bytes(glog, sew, in.N, cells, in.reward_table != 0);
    const int sits = (store_units(in, sew) + 63) / 64;
    ss.row_waves = in.step_rows > 0 ? in.step_rows : sits <= 6 ? 1 : sits <= 12 ? 2 : sits <= 33 ? 3 : sits <= 45 ? 4 : 5;
    ss.num_blocks = (in.E + sew - 1) / sew;
    // (the step kernel carries its own tables whatever the rollout shape does about its; EVERY workgroup stages the cell
    //  table and zeroes its tables per launch: past ~24 MB of that per step the rollout kernel is the faster one -- 40 x 30,
    //  4096 envs: 60 MB, 10.2 vs 5.8 us per step; 80 x 60: 113 vs 6.8; profiles/r04_step_big_grid.txt)
    //  -- or three times the step's rows where those are the larger part: 20 agents on 40 x 30, 4096 envs: 11.9 vs 16.4 us)
    const double step_rows_bytes = (double)in.E * in.N * (6.0 + 4.0 * in.N) * 4.0;
    ss.ok = (ss.lds_bytes <= kLdsTables &&
             (double)ss.num_blocks * (double)ss.lds_bytes <= std::max(24.0e6, 3.0 * step_rows_bytes)) ? 1 : 0;
    if (!ss.ok) CCXP_COVER(step_kernel_refused);
    return ss;
}

}  // namespace

ShapePlan plan_shape(const PlanIn& in) {
    ShapePlan p{};
    Work w{in, ceil_log2(in.N), 1 << ceil_log2(in.N), 64 >> ceil_log2(in.N), in.rows != 0};
    pick_envs_per_wave(w);
    classify_small_batch(w);
    w.tiles = tiles_of(in, w.ew);
    w.n4 = store_units(in, w.ew);
    // Small tiles (<= 12 store iterations per step, e.g. C2's 9.5): ONE writer wave whose stores in
    // flight are bounded (many small tiles oversubscribe the HBM write queues; the bound is the
    // regulator when step pacing is off and a safety net when it is on).
    // Larger tiles: 2-3 writers, no throttle (measured: no effect).
    w.small_tiles = w.n4 <= 64 * 12;
    w.writers = std::min(default_writers(w), 7);
    w.tpb = default_tiles_per_block(w);
    several_rounds_rule(w);
    while (w.tpb > 1 && w.tpb * (1 + w.writers) > 8) { CCXP_COVER(block_thread_limit); --w.tpb; }   // <= 512 threads per workgroup
    singles_over_pairs_rule(w);
    big_cell_table_rule(w);
    finish_layout(w, p);

    ccx::LaunchShape& s = p.shape;
    s.glog = w.glog;
    s.envs_per_wave = w.ew;
    s.waves_per_block = w.tpb;
    s.writers = w.writers;
    // with step pacing (the default) the throttle is only a safety net against a collapse of the
    // drain rate when the pace is too fast; without pacing it is the regulator (16, see above)
    s.store_throttle = in.store_throttle > 0 ? in.store_throttle
                       : (in.store_throttle == 0 && w.small_tiles && w.writers == 1) ? (in.step_pace_ns == -1 ? 16 : 48) : 0;
    s.num_blocks = (w.tiles + w.tpb - 1) / w.tpb;
    ccx::KParams& k = p.kp;
    k.EW = w.ew; k.waves_per_block = w.tpb; k.units_per_wave = units_of(in, w.ew); k.writers = w.writers;
    k.wp_magic = (uint32_t)((0x100000000ull + (unsigned long long)(in.width + 3) - 1ull) / (unsigned long long)(in.width + 3));
    k.writer_vmcnt = (uint32_t)s.store_throttle;
    k.writer0_small = (in.writer_roles >= 0 ? in.writer_roles != 0 : (w.small_batch || w.small_tiles)) && w.writers >= 2 ? 1u : 0u;
    write_window(w, k);
    if (in.rows) p.step = plan_step_shape(in, w.glog, w.ew);
    p.small_batch = w.small_batch;
    p.small_tiles = w.small_tiles;
    return p;
}

// Step pacing (ccx_kernels.hip).  The schedule limits the rate at which the resident
// workgroups inject observation stores; its start value assumes a drain rate of 6.8 TB/s and the
// kernel retunes it after every long launch (bounds: 7.8 TB/s .. a sixth of the start rate).
PacePlan plan_pacing(const PlanIn& in, const ShapePlan& sp, int blocks_per_cu) {
    PacePlan pp{};
    const ccx::LaunchShape& s = sp.shape;
    pp.resident_blocks = std::min(s.num_blocks, std::max(blocks_per_cu, 1) * in.num_cus);
    pp.step_bytes = tile_step_bytes(in, s.envs_per_wave) * s.waves_per_block * pp.resident_blocks;
    // A batch whose resident tiles cannot even fill the drain rate at a fast 0.40 us per env-step is
    // bound by the step chain, not by memory: pacing could only cost it (a clock read per step).  (0.45 us until the end of
    // round 4: the chain has become faster than that, and C2 batches of 2160 .. 2430 envs ran unpaced INTO the cliff -- 2304
    // envs at 0.62 of the peak between 0.82 at 2048 and 0.83 at 2500; profiles/r04_small_batch.txt.)
    const bool can_saturate = pp.step_bytes / 7000.0 >= 400.0;
    pp.paced = !(!in.rows || in.step_pace_ns == -1 || (in.step_pace_ns == 0 && !can_saturate));
    if (pp.paced) CCXP_COVER(paced); else CCXP_COVER(unpaced);
    pp.ring_when_paced = in.rows && pp.step_bytes / 7000.0 < 550.0;
    pp.pace_adapt = (in.step_pace_ns == 0) ? 1u : 0u;
    {   // how many steps make a launch worth pacing (~12 us) / long enough to judge its lateness (~50 us), at the assumed rate
        const double step_ns = pp.step_bytes / 6800.0;
        const double a = std::ceil(50000.0 / (step_ns > 1.0 ? step_ns : 1.0));
        pp.adapt_min_k = (uint32_t)(a < 4.0 ? 4.0 : a > 64.0 ? 64.0 : a);
        pp.pace_min_k = pp.adapt_min_k / 4u < 2u ? 2u : pp.adapt_min_k / 4u;
    }
    pp.pace_min_fp = to_fp(pp.step_bytes / 8000.0);    // (the spec peak; round 2 stopped at 7.8 TB/s, which multi-tile-per-CU shapes now reach)
    pp.pace_max_fp = to_fp(pp.step_bytes / 1100.0);
    if (in.rows) {
        if (in.step_pace_ns > 0) {
            CCXP_COVER(pace_fixed);
            pp.pace_init_fp = to_fp((double)in.step_pace_ns);
            pp.pace_start_source = CCX_PACE_START_FIXED;
        } else if (in.pace_start_ns > 0.0f) {
            CCXP_COVER(pace_caller);
            pp.pace_init_fp = to_fp((double)in.pace_start_ns);
            pp.pace_start_source = CCX_PACE_START_CALLER;
        } else {
            CCXP_COVER(pace_assumed);
            pp.pace_init_fp = to_fp(pp.step_bytes / 6800.0);
            pp.pace_start_source = CCX_PACE_START_ASSUMED;
        }
    }
    return pp;
}

void materialize(const ShapePlan& sp, const PacePlan& pp, ccx::LaunchShape& s, ccx::KParams& k) {
    s = sp.shape;
    s.resident_blocks = pp.resident_blocks;
    s.step_bytes = pp.step_bytes;
    k = sp.kp;
    k.resident_blocks = (uint32_t)pp.resident_blocks;
    k.pace_adapt = pp.pace_adapt;
    k.adapt_min_k = pp.adapt_min_k; k.pace_min_k = pp.pace_min_k;
    k.pace_min_fp = pp.pace_min_fp; k.pace_max_fp = pp.pace_max_fp;
}

void plan_out(const ccx::LaunchShape& s, const ccx::KParams& k, const ccx::StepShape& ss, const PacePlan& pp, ccxi_plan_out* out) {
    int64_t* v = out->v;
    v[CCXI_F_glog] = s.glog; v[CCXI_F_envs_per_wave] = s.envs_per_wave; v[CCXI_F_waves_per_block] = s.waves_per_block;
    v[CCXI_F_writers] = s.writers; v[CCXI_F_store_throttle] = s.store_throttle; v[CCXI_F_resident_blocks] = s.resident_blocks;
    v[CCXI_F_step_bytes] = (int64_t)s.step_bytes; v[CCXI_F_occ] = s.occ; v[CCXI_F_num_blocks] = s.num_blocks;
    v[CCXI_F_lds_bytes] = (int64_t)s.lds_bytes; v[CCXI_F_lds_bytes_observe] = (int64_t)s.lds_bytes_observe;
    v[CCXI_F_kp_EW] = k.EW; v[CCXI_F_kp_waves_per_block] = k.waves_per_block; v[CCXI_F_kp_units_per_wave] = k.units_per_wave;
    v[CCXI_F_kp_writers] = k.writers; v[CCXI_F_off_tiles] = k.off_tiles; v[CCXI_F_tile_stride] = k.tile_stride;
    v[CCXI_F_off_ws] = k.off_ws; v[CCXI_F_off_occ] = k.off_occ; v[CCXI_F_occ_words] = k.occ_words;
    v[CCXI_F_off_table] = k.off_table; v[CCXI_F_stage_slots] = k.stage_slots; v[CCXI_F_ws_per_writer] = k.ws_per_writer;
    v[CCXI_F_writer_vmcnt] = k.writer_vmcnt; v[CCXI_F_writer0_small] = k.writer0_small; v[CCXI_F_pace_phase] = k.pace_phase;
    v[CCXI_F_tile_map] = k.tile_map; v[CCXI_F_wp_magic] = k.wp_magic;
    v[CCXI_F_step_ok] = ss.ok; v[CCXI_F_step_glog] = ss.glog; v[CCXI_F_step_envs_per_wave] = ss.envs_per_wave;
    v[CCXI_F_step_row_waves] = ss.row_waves; v[CCXI_F_step_num_blocks] = ss.num_blocks;
    v[CCXI_F_step_lds_bytes] = (int64_t)ss.lds_bytes;
    v[CCXI_F_kp_resident_blocks] = k.resident_blocks; v[CCXI_F_paced] = pp.paced ? 1 : 0;
    v[CCXI_F_ring_when_paced] = pp.ring_when_paced ? 1 : 0; v[CCXI_F_pace_adapt] = k.pace_adapt;
    v[CCXI_F_adapt_min_k] = k.adapt_min_k; v[CCXI_F_pace_min_k] = k.pace_min_k; v[CCXI_F_pace_min_fp] = k.pace_min_fp;
    v[CCXI_F_pace_max_fp] = k.pace_max_fp; v[CCXI_F_pace_init_fp] = pp.pace_init_fp;
    v[CCXI_F_pace_start_source] = pp.pace_start_source;
}

bool reward_table_fits(PlanIn in) {
    in.reward_table = 1;
    for (int rows = 1; rows >= 0; --rows) {
        in.rows = rows;
        if (plan_shape(in).shape.lds_bytes > 150u * 1024u) return false;
    }
    return true;
}

// ---- per call ----------------------------------------------------------------------------------------------------------
CallShape call_shape(const ccx::LaunchShape& s, const ccx::KParams& k, bool ring_when_paced, bool step_ok) {
    return CallShape{s.num_blocks, s.resident_blocks, s.step_bytes, k.pace_state != nullptr, k.pace_adapt, k.pace_min_k, k.adapt_min_k,
                     ring_when_paced, step_ok};
}

namespace {

// the handle's short launches take the step kernel at all (StepShape::ok and the tunable)
bool step_kernel_on(const CallFacts& f, const CallIn& c) { return f.shape[0].step_ok && c.step_kernel != 0; }

// L = 6 + 4N is 2 mod 4: one step's observation slab (E x N x L floats) is a multiple of 16 bytes only when E x N is even
bool odd_slab(const CallFacts& f, const CallIn& c) { return c.writes_obs && (obs_bytes(f.E, f.N) & 15u) != 0; }

}  // namespace

// The cutter: a call as one launch, or as several.
CallPlan plan_call(const CallFacts& f, const CallIn& c) {
    CallPlan p{};
    int max_k;
    if (c.mixed) {
        // the short-launch kernel's policy instantiations (ccx_step.hip, POL): policy + merge + step in ONE launch per
        // <= 16 steps, whatever max_launch_steps says (16 is even: every sub-launch's slice of the observation tensor stays
        // 16-byte aligned).  Handles whose short launches cannot use the step kernel (tables beyond the LDS, or the tunable)
        // run the composition itself, step by step: policy kernel, merge kernel, the one-step call of the action tensor.
        p.stepwise = !step_kernel_on(f, c);
        max_k = p.stepwise ? 1 : ccx::kStepMaxK;
    } else {
        // The writer waves address the small output streams (rewards, flag bytes, compact rows, chosen actions) with 32-bit
        // byte offsets from the stream's base: one launch must stay below 4 GiB per stream.  Longer rollouts are cut into
        // launches on the same stream (bit-identical: an env's trajectory does not depend on how a rollout is split).
        const unsigned long long per_step = (unsigned long long)f.E * (unsigned long long)f.N * 16ull;   // the widest stream
        const unsigned long long fit = 0xFFFFFFFFull / per_step;
        max_k = (int)std::min<unsigned long long>(fit > 1 ? fit - 1 : 1, 0x7FFFFFFFull);
        if (c.max_launch_steps > 0) max_k = std::min(max_k, c.max_launch_steps);   // (tests: force the cut)
        // with E x N odd every sub-launch must start on an EVEN step so that its slice of the tensor stays 16-byte
        // aligned (an odd cut failed on "obs buffer must be 16-byte aligned" after the first sub-launch had
        // already advanced the state); launches of ONE step cannot, and such a cut is refused before anything is launched
        if (odd_slab(f, c) && max_k > 1) max_k &= ~1;
        p.refused = c.K > max_k && odd_slab(f, c) && max_k == 1;
    }
    p.steps_per_launch = max_k;
    p.launches = p.refused ? 0 : (int)(((long long)c.K + max_k - 1) / max_k);
    return p;
}

LaunchPlan plan_launch(const CallFacts& f, const CallIn& c, int k) {
    LaunchPlan l{};
    // the step kernel takes what it has instantiations for: up to 16 steps from an action tensor (the mixed entry point:
    // with its scripted slots, with or without a tensor or actions_out), on handles whose tables fit its LDS
    const bool tensor_only = c.actions && c.policy == 0 && !c.actions_out;
    l.kernel = step_kernel_on(f, c) && (c.mixed || (k <= ccx::kStepMaxK && tensor_only)) ? KERNEL_STEP : KERNEL_ROLLOUT;
    if (l.kernel == KERNEL_STEP) {
        // Only a call of ONE step fuses (a call that is cut leaves both to the stand-alone kernels behind its LAST launch,
        // also where it is cut into single steps; same bytes), where an MSK / RSO instantiation exists (ccx_kernels.h); the
        // mixed launches have none for the restarted rows
        l.masks_fused = c.masks_bound && ccx::step_masks_fused(c.K, c.order != 0);
        l.reset_obs_fused = c.reset_obs_on && c.reset_obs_fused != 0 && ccx::step_reset_obs_fused(c.K, c.order != 0, c.mixed != 0);
        return l;   // (no pacing, no controller state, no capture query)
    }
    const bool writes_obs = c.writes_obs != 0;
    l.shape = !writes_obs && c.small_shape != 0 ? 1 : 0;      // rewards / flag bytes / compact rows only: the no-rows shape
    const CallShape& s = f.shape[l.shape];
    l.paced = ccx::launch_is_paced(s.paced, writes_obs, k, s.pace_min_k);
    l.adaptive = ccx::launch_is_adaptive(s.paced, s.pace_adapt != 0u, writes_obs, k, s.pace_min_k, s.adapt_min_k);
    // A launch that is being captured into a HIP graph is replayed with these very arguments: the controller
    // cannot adapt across replays (the slot flip happens once, at capture time), so such a launch runs
    // at the pace in effect and neither votes nor touches the controller's state.
    l.pace_adapt = l.adaptive && c.capturing ? 0u : s.pace_adapt;
    l.flip_slot = l.adaptive && !c.capturing;     // the kernel collected the votes for the next pace in the other slot
    // launches the kernel will not pace hand steps to the writer waves through sequence words (ccx_kernels.h: one
    // definition of the launch modes for the host and the kernel)
    l.hand_flags = ccx::launch_uses_flags(s.paced, writes_obs, k, s.pace_min_k, c.hand2) ? 1u : 0u;
    // Paced batches whose step period is close to the sim wave's own chain (C2: 2200 .. 3000 envs, 0.41-0.52 us per env-step)
    // keep the ring too: a barrier per step couples the chain to the writers and such tiles step in 0.46 us instead of 0.40
    // (2304 envs 0.77 -> 0.83 of the peak, 2816 envs 0.88 -> 0.91; from 3072 envs on there is nothing in it, and saturating
    // batches want the barrier: DESIGN 3.7; profiles/r04_small_batch.txt)
    if (c.hand2 == 1 && writes_obs && f.shape[0].ring_when_paced) l.hand_flags = 1u;
    // A grid of more workgroups than the device holds is launched ROUND BY ROUND: one launch per `resident_blocks`
    // workgroups, back to back on the stream.  In ONE launch the workgroups of the second round start as slots come free, each on
    // a schedule of its own, and the chip's write front -- one narrow window per env-step while the tiles march in step --
    // frays over several slabs.  A launch boundary between the rounds (~2 us against rounds of 100+ us) restarts every round in step.  The kernel sees
    // its place in the grid through block_base (env indices, tile phases) and knows that it is one round (launch_flags: the pace of a partial last round); the
    // controller's owner is tile 0 of the first launch and all rounds vote into the same slot, as in one launch.
    // Only where the rows of the launch exceed the ~4 GB footprint knee (a stream through more memory than that
    // sustains 5-8 % less, whatever the kernel does; profiles/r04_output_size.txt):
    // below it the boundary costs 1-2 % (32 768 envs x 64 steps: 0.887 -> 0.873), beyond it the rounds in step win 3-5 %
    // (65 536 x 64: 0.750 -> 0.785).
    // The rounds are made EQUAL (R = ceil(blocks / resident) launches of ceil(blocks / R) workgroups, each on a schedule
    // scaled to its fill): a grid just above a whole number of rounds -- 17 768 envs of C2: 1111 workgroups on 1024 slots --
    // otherwise spends a full round's time on its last few tiles (0.74-0.77 of the peak where 15 800 envs reach 0.91; balanced:
    // 0.86-0.87).  That alone is worth the boundary for a paced grid of TWO rounds whose second would be less than 30 % full
    // (17 000 .. 20 500 envs of C2: +4 .. +12 %; fuller second rounds and grids of three or more rounds: nothing or a loss --
    // profiles/r04_balanced_rounds.txt).
    const int resident = s.resident_blocks;
    const double rows_bytes = writes_obs ? (double)k * (double)obs_bytes(f.E, f.N) : 0.0;
    const int n_rounds = resident > 0 ? (s.num_blocks + resident - 1) / resident : 1;
    // ... and whose tiles can FOLLOW the scaled schedule: a tile with one throttled writer steps in ~1 us at best; where the
    // common pace is already short (5 agents: 1.3 us for a full device) half-full rounds would be asked for 0.7 us, be late,
    // vote, and drag the common pace up (N = 5, 17 776 envs: 0.52 of the peak that way; profiles/r04_cliff_scan2.txt)
    const bool thin_second_round = n_rounds == 2 && (double)(s.num_blocks - resident) < 0.3 * resident &&
                                   s.step_bytes / 7000.0 * (0.5 * s.num_blocks / resident) >= 1200.0;
    l.by_rounds = resident > 0 && s.num_blocks > resident &&
                  (c.round_launches >= 2 || (c.round_launches == 1 && (rows_bytes > 3.5e9 || (l.paced && thin_second_round))));
    l.per_round = l.by_rounds ? (s.num_blocks + n_rounds - 1) / n_rounds : s.num_blocks;
    l.rounds = (s.num_blocks + l.per_round - 1) / l.per_round;
    return l;
}

void call_out(const CallPlan& cp, int k, const LaunchPlan& lp, ccxi_call_out* out) {
    int64_t* v = out->v;
    v[CCXI_C_steps_per_launch] = cp.steps_per_launch; v[CCXI_C_launches] = cp.launches; v[CCXI_C_refused] = cp.refused ? 1 : 0;
    v[CCXI_C_stepwise] = cp.stepwise ? 1 : 0;
    v[CCXI_C_k] = k; v[CCXI_C_kernel] = lp.kernel; v[CCXI_C_shape] = lp.shape; v[CCXI_C_paced] = lp.paced ? 1 : 0;
    v[CCXI_C_adaptive] = lp.adaptive ? 1 : 0; v[CCXI_C_pace_adapt] = lp.pace_adapt; v[CCXI_C_flip_slot] = lp.flip_slot ? 1 : 0;
    v[CCXI_C_hand_flags] = lp.hand_flags; v[CCXI_C_by_rounds] = lp.by_rounds ? 1 : 0; v[CCXI_C_per_round] = lp.per_round;
    v[CCXI_C_rounds] = lp.rounds; v[CCXI_C_masks_fused] = lp.masks_fused ? 1 : 0;
    v[CCXI_C_reset_obs_fused] = lp.reset_obs_fused ? 1 : 0;
}

int plan_call_out(const CallFacts& f, const CallIn& c, int launch, ccxi_call_out* out) {
    if (c.K < 1 || f.E < 1 || f.N < 1 || launch < 0) return CCX_EINVAL;
    const CallPlan cp = plan_call(f, c);
    if (cp.refused) {
        call_out(cp, 0, LaunchPlan{}, out);
        return CCX_OK;
    }
    if (launch >= cp.launches) return CCX_EINVAL;
    const int k = (int)std::min<long long>(cp.steps_per_launch, (long long)c.K - (long long)launch * cp.steps_per_launch);
    call_out(cp, k, plan_launch(f, c, k), out);
    return CCX_OK;
}

}  // namespace ccxp

namespace ccx {
// LDS of the short-launch kernel (ccx_step.hip): its own formula -- the reward table is not rounded up
size_t step_lds_bytes(int glog, int ew, int N, int cells, bool reward_table) {
    (void)N;
    return ccxp::up16((size_t)cells * 8u) + (reward_table ? (size_t)cells * 16u : 0u) +
           ccxp::up16((size_t)ew * 2u * ((size_t)cells + 1u) * ccxp::mask_bytes(glog)) + 2u * ccxp::kWSlotBytes +
           256u /* move-order exchange */;
}
}  // namespace ccx

// ---- ccx_keys.h: the instantiation a launch of a call takes, from the plans and the call ----------------------------------
namespace {

struct KeyShapes {            // the two planned shapes of a handle, as far as the keys read them
    ccxp::CallFacts f;
    ccxp::ShapePlan sp[2];
};

KeyShapes key_shapes(const ccxi_plan_in& in, const int* blocks_per_cu) {
    KeyShapes ks{};
    ks.f = ccxp::CallFacts{in.E, in.N, {}};
    for (int i = 0; i < 2; ++i) {
        ccxp::PlanIn pin = in;
        pin.rows = i == 0 ? 1 : 0;
        ks.sp[i] = ccxp::plan_shape(pin);
        const ccxp::PacePlan pp = ccxp::plan_pacing(pin, ks.sp[i], blocks_per_cu[i]);
        ks.f.shape[i] = ccxp::CallShape{ks.sp[i].shape.num_blocks, pp.resident_blocks, pp.step_bytes, pp.paced, pp.pace_adapt,
                                        pp.pace_min_k, pp.adapt_min_k, pp.ring_when_paced, ks.sp[i].step.ok != 0};
    }
    return ks;
}

// the key of the launch of k steps that begins at step k0 of the call c (what ccx_api.hip hands to launch_step / launch_rollout)
ccxi_key launch_key(const ccxi_plan_in& in, const KeyShapes& ks, const ccxp::CallIn& c, const ccxi_key_facts& kf, int k0, int k) {
    const ccxp::LaunchPlan lp = ccxp::plan_launch(ks.f, c, k);
    if (lp.kernel == ccxp::KERNEL_STEP)
        return ccx::pack_key(ccx::step_key(ks.sp[0].step.glog, in.N, k, c.order != 0, c.mixed != 0, lp.masks_fused, lp.reset_obs_fused));
    const ccxp::ShapePlan& sp = ks.sp[lp.shape];
    const bool has_obs = kf.obs != 0;
    const size_t residue = ((size_t)kf.obs_residue + (size_t)k0 * ccxp::obs_bytes(in.E, in.N)) & 127u;   // (kout_at)
    return ccx::pack_key(ccx::rollout_key(ccx::RolloutFacts{
        sp.shape.glog, in.N, in.E, sp.kp.EW, sp.kp.units_per_wave, sp.shape.writers, sp.kp.writer0_small != 0u, sp.shape.occ != 0,
        has_obs || kf.reward || kf.agent_flags || kf.env_flags || kf.obs_compact || c.actions_out, has_obs, (uint32_t)residue,
        c.order != 0, c.policy != 0, in.reward_table != 0 || in.term_table != 0}));
}

int call_key(const ccxi_plan_in& in, const KeyShapes& ks, ccxp::CallIn c, const ccxi_key_facts& kf, int launch, ccxi_key* out) {
    if (c.K < 1 || in.E < 1 || in.N < 1) return CCX_EINVAL;
    c.writes_obs = kf.obs != 0;
    const ccxp::CallPlan cp = ccxp::plan_call(ks.f, c);
    *out = ccxi_key{CCXI_KEY_NONE, {}};
    if (cp.refused) return CCX_OK;
    if (launch < 0) launch = cp.launches - 1;          // (the last one)
    if (launch >= cp.launches) return CCX_EINVAL;
    const int k0 = launch * cp.steps_per_launch, k = std::min(cp.steps_per_launch, c.K - k0);
    if (cp.stepwise) {
        // ccx_api.hip: run_stepwise -- the one-step call of the actions the policy and merge kernels left, in the caller's order
        ccxp::CallIn one{};
        one.K = 1; one.actions = 1; one.order = c.order; one.writes_obs = c.writes_obs; one.capturing = c.capturing;
        one.hand2 = c.hand2; one.round_launches = c.round_launches; one.small_shape = c.small_shape; one.step_kernel = c.step_kernel;
        one.max_launch_steps = c.max_launch_steps; one.reset_obs_fused = c.reset_obs_fused;
        // (a step whose slice of the tensor is not 16-byte aligned writes its rows to the aligned staging slab)
        ccxi_key_facts kf1 = kf;
        kf1.obs_residue = (int32_t)(((size_t)kf.obs_residue + (size_t)k0 * ccxp::obs_bytes(in.E, in.N)) & 127u);
        if (kf1.obs_residue & 15) kf1.obs_residue = 0;
        *out = launch_key(in, ks, one, kf1, 0, 1);
        return CCX_OK;
    }
    *out = launch_key(in, ks, c, kf, k0, k);
    return CCX_OK;
}

}  // namespace

extern "C" {

int ccxi_call_key(const ccxi_plan_in* in, const int* blocks_per_cu, const ccxi_call_in* call, const ccxi_key_facts* facts, int launch,
                  ccxi_key* out) {
    if (!in || !blocks_per_cu || !call || !facts || !out) return CCX_EINVAL;
    return call_key(*in, key_shapes(*in, blocks_per_cu), *call, *facts, launch, out);
}

int ccxi_call_keys(const ccxi_plan_in* in, const int* blocks_per_cu, const ccxi_call_in* calls, const ccxi_key_facts* facts, int n,
                   ccxi_key* out) {
    if (!in || !blocks_per_cu || !calls || !facts || !out || n < 0) return CCX_EINVAL;
    const KeyShapes ks = key_shapes(*in, blocks_per_cu);
    for (int i = 0; i < n; ++i) {
        if (int rc = call_key(*in, ks, calls[i], facts[i], 0, out + 2 * i)) return rc;
        if (int rc = call_key(*in, ks, calls[i], facts[i], -1, out + 2 * i + 1)) return rc;
    }
    return CCX_OK;
}

int ccxi_observe_key(const ccxi_plan_in* in, ccxi_key* out) {
    if (!in || !out) return CCX_EINVAL;
    ccxp::PlanIn pin = *in;
    pin.rows = 1;
    *out = ccx::pack_key(ccx::observe_key(ccxp::plan_shape(pin).shape.glog, in->N));
    return CCX_OK;
}

}  // extern "C"

extern "C" {

const char* ccxi_plan_field_names(void) {
#define CCXI_X(name) #name ","
    return CCXI_PLAN_FIELDS(CCXI_X);
#undef CCXI_X
}

int ccxi_plan(const ccxi_plan_in* in, int blocks_per_cu, ccxi_plan_out* out) {
    if (!in || !out) return CCX_EINVAL;
    const ccxp::ShapePlan sp = ccxp::plan_shape(*in);
    const ccxp::PacePlan pp = ccxp::plan_pacing(*in, sp, blocks_per_cu);
    ccx::LaunchShape s;
    ccx::KParams k;
    ccxp::materialize(sp, pp, s, k);
    ccxp::plan_out(s, k, sp.step, pp, out);
    return CCX_OK;
}

const char* ccxi_call_field_names(void) {
#define CCXI_X(name) #name ","
    return CCXI_CALL_FIELDS(CCXI_X);
#undef CCXI_X
}

int ccxi_plan_call(const ccxi_plan_in* in, const int* blocks_per_cu, const ccxi_call_in* call, int launch, ccxi_call_out* out) {
    if (!in || !blocks_per_cu || !call || !out) return CCX_EINVAL;
    ccxp::CallFacts f{in->E, in->N, {}};
    for (int i = 0; i < 2; ++i) {
        ccxp::PlanIn pin = *in;
        pin.rows = i == 0 ? 1 : 0;
        const ccxp::ShapePlan sp = ccxp::plan_shape(pin);
        const ccxp::PacePlan pp = ccxp::plan_pacing(pin, sp, blocks_per_cu[i]);
        f.shape[i] = ccxp::CallShape{sp.shape.num_blocks, pp.resident_blocks, pp.step_bytes, pp.paced, pp.pace_adapt, pp.pace_min_k,
                                     pp.adapt_min_k, pp.ring_when_paced, sp.step.ok != 0};
    }
    return ccxp::plan_call_out(f, *call, launch, out);
}

#ifdef CCX_PLAN_COVERAGE
const char* ccxi_plan_coverage(void) {   // "branch=count,..."
    static char buf[4096];
    static const char* const names[] = {
#define CCXP_X(name) #name,
        CCXP_BRANCHES(CCXP_X)
#undef CCXP_X
    };
    size_t at = 0;
    for (int i = 0; i < ccxp::COVER_COUNT; ++i)
        at += (size_t)snprintf(buf + at, sizeof(buf) - at, "%s=%lld,", names[i], ccxp::g_cover[i]);
    return buf;
}
#endif

}  // extern "C"
