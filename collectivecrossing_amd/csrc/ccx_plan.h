// ccx_plan.h -- launch-shape selection as a pure function (ccx_plan.hip), and the two internal entry points that expose it
// to the tests.  Not installed, not part of the ABI of include/ccx.h.
#pragma once
#include <cstddef>
#include <cstdint>

#include "ccx_kernels.h"

// ---- internal C entry points (exported from libccx.so, NOT declared in include/ccx.h) --------------------------------
extern "C" {

// what the planner reads (every field an int32 but the last)
typedef struct ccxi_plan_in {
    int32_t E, N, width, height, num_cus;
    int32_t reward_table, term_table;                     // 1: a user reward / terminated table is set
    int32_t lanes_per_wave, waves_per_block, writers, store_throttle, step_pace_ns;   // the caller's overrides
    int32_t occ_tables, pair_rows, writer_roles, pace_phase, tile_map, step_lanes, step_rows;   // tunables
    int32_t rows;                                         // 1: launches that write observation rows, 0: launches without
    float pace_start_ns;
} ccxi_plan_in;

// one int64 per field, in this order (ccxi_plan_field_names() returns the names, comma-separated).  Pointers are reported
// as 0 / 1, step_bytes as a whole number of bytes; the step_* fields, ring_when_paced, pace_init_fp and
// pace_start_source belong to the rows shape and are 0 in the plan of the other one.
#define CCXI_PLAN_FIELDS(X)                                                                                              \
    X(glog) X(envs_per_wave) X(waves_per_block) X(writers) X(store_throttle) X(resident_blocks) X(step_bytes) X(occ)     \
    X(num_blocks) X(lds_bytes) X(lds_bytes_observe)                                                                      \
    X(kp_EW) X(kp_waves_per_block) X(kp_units_per_wave) X(kp_writers) X(off_tiles) X(tile_stride) X(off_ws) X(off_occ)   \
    X(occ_words) X(off_table) X(stage_slots) X(ws_per_writer) X(writer_vmcnt) X(writer0_small) X(pace_phase) X(tile_map) \
    X(wp_magic)                                                                                                          \
    X(step_ok) X(step_glog) X(step_envs_per_wave) X(step_row_waves) X(step_num_blocks) X(step_lds_bytes)                 \
    X(kp_resident_blocks) X(paced) X(ring_when_paced) X(pace_adapt) X(adapt_min_k) X(pace_min_k) X(pace_min_fp)          \
    X(pace_max_fp) X(pace_init_fp) X(pace_start_source)
enum {
#define CCXI_X(name) CCXI_F_##name,
    CCXI_PLAN_FIELDS(CCXI_X)
#undef CCXI_X
    CCXI_PLAN_NFIELDS
};
typedef struct ccxi_plan_out { int64_t v[CCXI_PLAN_NFIELDS]; } ccxi_plan_out;

const char* ccxi_plan_field_names(void);
// the pure planner: plan_shape + plan_pacing of `in` with the given occupancy figure.  Works without a GPU.
int ccxi_plan(const ccxi_plan_in* in, int blocks_per_cu, ccxi_plan_out* out);
// the plan of a live handle's rows (rows = 1) or no-rows shape, and the occupancy figure the runtime gives for it
int ccxi_handle_plan(const struct ccx_handle* h, int rows, ccxi_plan_out* out, int* blocks_per_cu);

// one stepping call, as the per-call planner reads it (every field an int32): the call itself, then the handle's tunables
typedef struct ccxi_call_in {
    int32_t K;                                            // env-steps of the call
    int32_t actions, order, actions_out;                  // 1: the call has an action tensor / a move order / an actions_out tensor
    int32_t policy;                                       // in-kernel policy of the rollout kernel (CCX_POLICY_*, 0 = the tensor)
    int32_t mixed;                                        // 1: the mixed-control entry point (ccx_rollout_mixed)
    int32_t writes_obs;                                   // 1: the call writes observation rows
    int32_t capturing;                                    // 1: the handle's stream is being captured into a graph
    int32_t masks_bound, reset_obs_on;                    // 1: the call may write the bound masks / the restarted rows in its launch
    int32_t hand2, round_launches, small_shape, step_kernel, max_launch_steps, reset_obs_fused;   // tunables
} ccxi_call_in;

// one int64 per field, in this order (ccxi_call_field_names()).  The first four describe the call, the rest ONE of its launches
// (`k` steps); a refused call has no launches and zeros there.
#define CCXI_CALL_FIELDS(X)                                                                                              \
    X(steps_per_launch) X(launches) X(refused) X(stepwise)                                                               \
    X(k) X(kernel) X(shape) X(paced) X(adaptive) X(pace_adapt) X(flip_slot) X(hand_flags) X(by_rounds) X(per_round)      \
    X(rounds) X(masks_fused) X(reset_obs_fused)
enum {
#define CCXI_X(name) CCXI_C_##name,
    CCXI_CALL_FIELDS(CCXI_X)
#undef CCXI_X
    CCXI_CALL_NFIELDS
};
typedef struct ccxi_call_out { int64_t v[CCXI_CALL_NFIELDS]; } ccxi_call_out;

const char* ccxi_call_field_names(void);
// the pure per-call planner: both shapes of `in` planned with their occupancy figures (blocks_per_cu[0]: rows, [1]: no rows;
// in->rows is ignored), then plan_call and plan_launch of launch number `launch` (0 .. launches - 1).  Works without a GPU.
int ccxi_plan_call(const ccxi_plan_in* in, const int* blocks_per_cu, const ccxi_call_in* call, int launch, ccxi_call_out* out);
// the same for a live handle: its two shapes and ITS tunables (the six tunable fields of `call` are ignored)
int ccxi_handle_call_plan(const struct ccx_handle* h, const ccxi_call_in* call, int launch, ccxi_call_out* out);

}  // extern "C"

namespace ccxp {

using PlanIn = ccxi_plan_in;

// Stage 1: everything that follows from the inputs alone.
struct ShapePlan {
    ccx::LaunchShape shape;   // all but resident_blocks / step_bytes (stage 2)
    ccx::KParams kp;          // the LAYOUT fields only: EW, waves_per_block, units_per_wave, writers, off_*, tile_stride, occ_words,
                              // stage_slots, ws_per_writer, writer_vmcnt, writer0_small, pace_phase, tile_map, wp_magic; the rest is zero
    ccx::StepShape step;      // the short-launch kernel's shape (rows shape only)
    bool small_batch;         // too small to be memory-bound: full or half tiles, writers split by role
    bool small_tiles;         // <= 12 store iterations per tile and step
};

// Stage 2: what needs the runtime's occupancy figure.
struct PacePlan {
    int resident_blocks;
    double step_bytes;        // bytes the resident workgroups write per env-step
    bool paced;               // launches of this shape are paced at all (KParams::pace_state is set)
    bool ring_when_paced;     // paced launches keep the sequence-word ring (step period close to the sim chain)
    uint32_t pace_adapt, adapt_min_k, pace_min_k, pace_min_fp, pace_max_fp;
    uint32_t pace_init_fp;    // the controller's start value and where it came from (CCX_PACE_START_*); rows shape only
    int pace_start_source;
};

// byte offsets of the rollout kernel's LDS carve-up: [cell table (+ reward table)][tiles][u16 obs table]
struct LdsLayout { size_t off_tiles, off_ws, off_occ, tile_stride, total, occ_bytes, table; };

inline size_t up16(size_t v) { return (v + 15u) & ~(size_t)15u; }
int ceil_log2(int n);
uint32_t to_fp(double ns);   // ns per env-step -> ticks of the 100 MHz clock x 256, clamped to 1 .. 4e9
inline float fp_to_ns(uint32_t fp) { return (float)((double)fp / 256.0 * 10.0); }   // ... and back

// THE LDS size model of the rollout kernel: a ring of `ring_slots`, `writer_slots` staging slots per tile, `tiles_per_block`
// tiles of `ew` envs, with or without the occupancy tables; the reward table comes from `in`.
LdsLayout lds_layout(const PlanIn& in, uint32_t ring_slots, size_t writer_slots, int tiles_per_block, int ew, bool with_tables);
// THE residency estimate: rounds a batch of `tiles` needs when a CU holds as many workgroups as its LDS, `wave_cap` wave
// slots and `max_per_cu` allow
size_t rounds(size_t tiles, size_t bytes_per_block, int tiles_per_block, int waves_per_block, int wave_cap, size_t max_per_cu,
              int num_cus);

ShapePlan plan_shape(const PlanIn& in);
PacePlan plan_pacing(const PlanIn& in, const ShapePlan& sp, int blocks_per_cu);
bool reward_table_fits(PlanIn in);   // both shapes of `in` with a reward table stay within the LDS of a CU

// the launch shape and the kernel-parameter template of a plan (pace_state, the tables and the config fields are the caller's)
void materialize(const ShapePlan& sp, const PacePlan& pp, ccx::LaunchShape& s, ccx::KParams& k);
// reads `paced`, `ring_when_paced`, `pace_init_fp` and `pace_start_source` from pp, everything else from s / k / step
void plan_out(const ccx::LaunchShape& s, const ccx::KParams& k, const ccx::StepShape& step, const PacePlan& pp, ccxi_plan_out* out);

// ---- Stage 3, per call: how a stepping call is cut into launches and how each launch is driven.  Pure like the
// rest: the caller says what the handle's two shapes are and what the call is.
using CallIn = ccxi_call_in;

// what a call's launches depend on of one planned shape
struct CallShape {
    int num_blocks, resident_blocks;
    double step_bytes;
    bool paced;                       // PacePlan::paced: KParams::pace_state is set
    uint32_t pace_adapt, pace_min_k, adapt_min_k;
    bool ring_when_paced, step_ok;    // rows shape only (PacePlan::ring_when_paced, StepShape::ok)
};
CallShape call_shape(const ccx::LaunchShape& s, const ccx::KParams& k, bool ring_when_paced, bool step_ok);
struct CallFacts {
    int E, N;
    CallShape shape[2];               // [0] launches that write observation rows, [1] launches without
};

struct CallPlan {
    int steps_per_launch, launches;   // every launch takes steps_per_launch steps but the last, which takes the rest
    bool refused;                     // an odd E x N slab that would have to be cut into launches of one step
    bool stepwise;                    // the unfused mixed-control step: one env-step per launch, actions produced in between
};
enum : int { KERNEL_STEP = 0, KERNEL_ROLLOUT = 1 };
struct LaunchPlan {
    int kernel;                       // KERNEL_STEP: the short-launch kernel (ccx_step.hip), KERNEL_ROLLOUT: the rollout kernel
    int shape;                        // index into CallFacts::shape; this and the next nine: rollout kernel only, 0 for the step kernel
    bool paced, adaptive;           // ccx_kernels.h: launch_is_paced / launch_is_adaptive of this launch
    uint32_t pace_adapt;              // KParams::pace_adapt as sent: cleared for an adaptive launch that is being captured
    bool flip_slot;                   // the host flips the controller's slot behind the launch (the kernel voted)
    uint32_t hand_flags;              // KParams::hand_flags
    bool by_rounds;                   // `rounds` launches of per_round workgroups (the last: the rest), block_base 0, per_round, ...
    int per_round, rounds;
    bool masks_fused, reset_obs_fused;   // the step launch writes the bound masks / the restarted rows itself
};

// bytes of the observation rows of `steps` env-steps: [steps][E][N][6 + 4N] floats
inline size_t obs_bytes(int E, int N, size_t steps = 1) { return steps * (size_t)E * (size_t)N * (size_t)(6 + 4 * N) * sizeof(float); }

CallPlan plan_call(const CallFacts& f, const CallIn& c);
LaunchPlan plan_launch(const CallFacts& f, const CallIn& c, int k);   // a launch of k steps of the call c
void call_out(const CallPlan& cp, int k, const LaunchPlan& lp, ccxi_call_out* out);
// the C entry points' tail: plan_call, then plan_launch of launch number `launch`
int plan_call_out(const CallFacts& f, const CallIn& c, int launch, ccxi_call_out* out);

}  // namespace ccxp
