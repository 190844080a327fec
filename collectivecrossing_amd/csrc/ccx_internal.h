// ccx_internal.h -- what the translation units of the C-ABI layer share (not installed, not part of the ABI).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstdio>
#include <vector>

#include "../../include/ccx.h"
#include "ccx_entry.h"
#include "ccx_kernels.h"

namespace ccxi {

// records the thread-local message returned by ccx_last_error() and hands the code back
int fail(int code, const char* fmt, ...) __attribute__((format(printf, 2, 3)));

// the grid of a launch over `rows` rows, rows_per_block to a workgroup: CCX_EINVAL for rows < 1 or more than 2^31 - 1 workgroups
int row_blocks(const char* who, int64_t rows, int64_t rows_per_block, unsigned& blocks);

// CCX_MLP's backward (ccx_mlp_backward.hip): enqueue head_grad_final_kernel over B block partials per element in
// ccx_mlp_grad.h's layout -- the final step of every backward that leaves its partials so (ccx_mlp_wide.hip)
int head_grad_final_launch(struct ::ccx_handle* h, int32_t L, int32_t H, int32_t O, double* partials, long long B, float* grad_w1t,
                           float* grad_b1, float* grad_w2, float* grad_b2);

// CCX_EPISODE_STATS (ccx_episode_stats.hip): zero the running accumulators and the latch of the masked envs on the handle's
// stream (the resets call it while tracking is on); free the buffers (ccx_destroy)
int episode_stats_reset(struct ::ccx_handle* h, const uint8_t* env_mask);
void episode_stats_destroy(struct ::ccx_handle* h);

// The pace controller of the rollout kernel (ccx_kernels.h: KParams::pace_state), host side.  apply() (ccx_api.hip) resets it
// with every new plan; prepare() is the ONE function that restarts it on the device.
struct PaceController {
    uint32_t* state = nullptr;        // device u32 [8]: current pace (ticks x 256) in [slot], votes in [slot ^ 1], floor, cliff memory
    uint32_t slot = 0;                // slot of `state` the next launch reads
    uint32_t init_fp = 0;             // value to (re)start the controller from
    bool dirty = true;                // `state` must be rewritten before a paced launch
    bool needs_calibration = false;   // the controller runs from the assumed start value: the first ADAPTIVE eager launch calibrates and restarts it
    int start_source = 0;             // CCX_PACE_START_*: where the start value came from
    float probe_gbs = 0.0f;           // write rate the calibration probe measured (GB/s), 0 = not run

    // Ahead of a launch of the rollout kernel that the plan calls `paced` / `adaptive` (ccx_plan.h: LaunchPlan), on a stream
    // that is `capturing` or not: (re)start the controller where it is due -- new handle, launch shape or setting --, with the
    // start value calibrated on the `obs_bytes` at `obs` that the launch is about to overwrite.  Enqueues memsets on the
    // handle's stream and, when it calibrates, synchronises it once; refuses to do either inside a capture.
    int prepare(const ::ccx_handle* h, bool paced, bool adaptive, bool capturing, float* obs, size_t obs_bytes);
};

}  // namespace ccxi

#define CCX_HIP(call)                                                                         \
    do {                                                                                      \
        hipError_t e_ = (call);                                                               \
        if (e_ != hipSuccess)                                                                 \
            return ccxi::fail(CCX_EHIP, "%s failed: %s (%s:%d)", #call, hipGetErrorString(e_), \
                              __FILE__, __LINE__);                                            \
    } while (0)

struct ccx_handle {
    ccx_params params{};
    int32_t E = 0, N = 0;
    int64_t env_offset = 0, total_envs = 0;
    int device = 0;
    hipStream_t stream = nullptr;
    ccx::KState st{};
    uint8_t* st_slab = nullptr;              // ONE allocation behind the seven state arrays (ccx_kernels.h: StateSlab)
    unsigned long long* cell_info = nullptr; // per-cell geometry table (ccx_step_rule.h: cell_word)
    double* reward_table = nullptr;          // device f64 [2][cells of the padded grid]: user reward table (ccx_set_reward_table), null = built-in
    std::vector<uint8_t> term_table[2];      // host u8 [(H+1)(W+1)] per agent type: user terminated table (ccx_set_terminated_table), empty = built-in
    uint8_t* placement_scratch = nullptr;    // u8 [E][N][2] work area of ccx_reset_seeded
    unsigned long long* counters = nullptr;  // 6 x u64 (+ 10 spare words used by diagnostic builds)
    const uint8_t* pool = nullptr;
    int64_t pool_size = 0;
    hipEvent_t ev_start = nullptr, ev_stop = nullptr;
    bool timed = false;
    bool timing = false;                                       // record HIP events around launches
    int lanes_per_wave = 0, waves_per_block = 0, writers = 0;  // user overrides (0 = default)
    int store_throttle = 0;                                    // 0 = default, -1 = off, >0 = stores in flight
    int step_pace_ns = 0;                                      // 0 = adaptive, -1 = off, >0 = fixed ns per env-step
    ccxi::PaceController pace;                                 // the pace controller's host side (the caller's settings: step_pace_ns above, pace_start_ns, pace_calibrate)
    uint16_t* obs_table = nullptr;                             // device: obs address table of the current shape
    std::vector<uint16_t> obs_table_host;
    int num_cus = 256;
    float pace_start_ns = 0.0f;                                // > 0: the adaptive controller starts here (ccx_set_step_pace_start)
    bool pace_calibrate = true;                                // measure the start value in-process (ccx_set_pace_calibration)
    int tun_pace_phase = -1, tun_tile_map = -1;                 // -1 = the library's choice for the launch shape
    int tun_writer_roles = -1;                                  // -1 = by batch size, 0 = writers share everything, 1 = writer 0 small outputs only
    int tun_hand2 = 1;                                          // sim -> writer hand-off: 0 barrier per step, 1 sequence words in unpaced launches, 2 always
    int tun_pair_rows = -1;                                     // -1 / 1: row writers of small batches may take two steps per iteration (a second staging slot each), 0: never
    int tun_max_launch_steps = 0;                               // > 0: cut rollouts into launches of at most this many steps
    double epsilon = 0.0;                                      // ccx_set_policy_epsilon, as given (the MT19937 stream compares doubles)
    int eps_stream = 0;                                        // CCX_EPS_STREAM_*: where the policies' exploration draws come from
    uint32_t* mt_state = nullptr;                              // device u32 [E][625]: one numpy RandomState per env (CCX_EPS_STREAM_MT19937)
    uint8_t* stream_actions = nullptr;                         // device u8 [E][N]: one step's actions of the unfused policy loop
    float* stream_obs = nullptr;                               // device f32 [E][N][L]: aligned staging slab of that loop
    bool check_inputs = false;                                 // ccx_set_check_inputs
    unsigned long long* input_errors = nullptr;                // device [2]: bad action bytes, bad order rows
    int tun_step_kernel = -1;                                   // launches of <= 16 steps: -1 / 1 the short-launch kernel (ccx_step.hip) where it applies, 0 always the rollout kernel
    int tun_step_rows = 0, tun_step_lanes = 0;                  // short-launch kernel: row waves per tile (0 = default), lanes per wave carrying agents (0 = default)
    ccx::StepShape step_shape{};
    bool ring_when_paced = false;                               // paced launches of this shape hand steps over through the sequence-word ring (step period close to the sim chain)
    int tun_occ_tables = -1;                                    // 0: the rollout kernel compares all pairs of an env instead of keeping LDS occupancy tables (-1: the library's choice)
    int tun_round_launches = 1;                                 // 1: a grid of several rounds of workgroups is launched round by round when its rows exceed ~3.5 GB, 2: always, 0: one launch
    int tun_small_shape = 1;                                    // 1: launches without observation rows take their own launch shape (shape_small), 0: the rows shape
    ccx::LaunchShape shape{};                                   // launches that write observation rows
    ccx::KParams kp{};
    ccx::LaunchShape shape_small{};                             // launches without them (rewards / flag bytes / compact rows)
    ccx::KParams kp_small{};
    uint32_t rng_lo = 0, rng_hi = 0;                            // seed of CCX_POLICY_RANDOM and of the epsilon draws (ccx_set_rng_seed)
    uint8_t* bound_masks = nullptr;                             // ccx_bind_action_masks: device u8 [E][N] (the caller's), null = not bound
    int reset_obs = 0;                                          // CCX_RESET_OBS_*: what obs[s][e] of a restarted env holds (ccx_set_reset_obs)
    float* bound_final_obs = nullptr;                           // ccx_bind_final_obs: the caller's side buffers for the terminal rows, null = dropped
    float* bound_final_compact = nullptr;
    int tun_reset_obs_fused = 1;                                // 0: NEXT-mode single steps take the fix-up kernel too (timing table only)
    bool stats_on = false;                                      // CCX_EPISODE_STATS: ccx_episode_stats_enable .. _disable
    uint8_t* stats_slab = nullptr;                              // ONE allocation behind every array of `stats` and the two work arrays
    ccx_episode_stats stats{};                                  // what ccx_episode_stats_view hands out
    int32_t* stats_count = nullptr;                             // device i32 [E]: records of the current update per env (log only)
    long long* stats_base = nullptr;                            // device i64 [E]: log slot of each env's first record of the update
    int tun_stats_naive = 0;                                    // 1: the accumulate kernel with one dependent load per step (timing table only)
    ccxi_key last_key{CCXI_KEY_NONE, {}};                       // ccx_keys.h: the instantiation the last stepping launch took, written by the launch path ...
    ccxi_key last_observe_key{CCXI_KEY_NONE, {}};               // ... and the one of the last ccx_observe / ccx_expand_observations
    uint32_t eps_thr = 0;                                       // epsilon * 2^32 of the scripted policies (ccx_set_policy_epsilon); the launchers copy the three into their KParams
};

// ---------------------------------------------------------------------------------------------
// The ring of CCX_REPLAY as the ABI passes it, and the launch of a kernel that gathers a minibatch of B records, EW to a wave
// (ccx_replay.hip, ccx_nstep.hip, ccx_prio.hip; the grid also ccx_minibatch.hip).  The device side is ccx_gather.h.
// ---------------------------------------------------------------------------------------------

// ring_steps and the eight arrays, in the order of RingArrays
#define CCX_RING_PARAMS int64_t ring_steps, float* ring_obs_c, float* ring_next_c, uint8_t* ring_actions, double* ring_reward, \
                        uint8_t* ring_done, uint8_t* ring_valid, uint8_t* ring_masks_next, int64_t* ring_state
#define CCX_RING_ARGS ring_steps, ring_obs_c, ring_next_c, ring_actions, ring_reward, ring_done, ring_valid, ring_masks_next, ring_state

namespace ccxi {

struct RingArrays {                    // the ring's own storage, [R][N] (compact: [R][N] float4)
    float4* obs_c;
    float4* next_c;
    uint8_t* actions;
    double* reward;
    uint8_t* done;
    uint8_t* valid;
    uint8_t* masks_next;
    long long* state;                  // {head, draws, 0, 0}
};

struct BatchOut {                      // the minibatch of B records, [B][N]
    float* obs;                        // [B][N][L] or null
    float* next_obs;                   // [B][N][L] or null
    uint8_t* actions;
    double* reward;
    uint8_t* done;
    uint8_t* valid;
    uint8_t* masks_next;
    int64_t* index;                    // [B]
};

struct FetchArgs {                     // what a kernel that fetches B records of the ring takes
    RingArrays ring;
    const int64_t* index_in;           // [B]: read where the kernel does not draw
    BatchOut out;
    long long B, R;
    int S, E, glog;
    uint32_t seed_lo, seed_hi;
};

inline unsigned blocks_of(int64_t n) { return (unsigned)((n + 255) / 256); }     // workgroups of 256 lanes, a lane per item (n <= 2^37: R N)

// the handle and the ring's S: R = S * E records are addressed with 32 bits
inline int check_ring_steps(const char* who, const ccx_handle* h, int64_t ring_steps) {
    if (!h) return fail(CCX_EINVAL, "NULL handle");
    if (ring_steps < 1 || ring_steps >= (1ll << 31) || ring_steps * (int64_t)h->E >= (1ll << 31))
        return fail(CCX_EINVAL, "%s: ring_steps = %lld out of range (1 <= S, S * E < 2^31)", who, (long long)ring_steps);
    return CCX_OK;
}

inline int check_ring(const char* who, const ccx_handle* h, CCX_RING_PARAMS, RingArrays& a) {
    if (int rc = check_ring_steps(who, h, ring_steps)) return rc;
    if (!ring_obs_c || !ring_next_c || !ring_actions || !ring_reward || !ring_done || !ring_valid || !ring_masks_next || !ring_state)
        return fail(CCX_EINVAL, "%s: NULL ring array", who);
    if (misaligned(16, ring_obs_c, ring_next_c)) return fail(CCX_EINVAL, "%s: the ring's compact arrays must be 16-byte aligned", who);
    if (misaligned(8, ring_reward, ring_state)) return fail(CCX_EINVAL, "%s: the ring's reward and state must be 8-byte aligned", who);
    a = RingArrays{reinterpret_cast<float4*>(ring_obs_c), reinterpret_cast<float4*>(ring_next_c), ring_actions, ring_reward, ring_done,
                   ring_valid, ring_masks_next, reinterpret_cast<long long*>(ring_state)};
    return CCX_OK;
}

inline int check_batch_size(const char* who, const ccx_handle* h, int64_t B) {
    if (B < 1 || B * (int64_t)h->N > (1ll << 31)) return fail(CCX_EINVAL, "%s: batch = %lld out of range (1 <= B <= 2^31 / N)", who, (long long)B);
    return CCX_OK;
}

// the grid of B records, EW to a wave, in workgroups of the handle's launch shape
inline int gather_grid(const char* who, const ccx_handle* h, int64_t B, dim3& grid, dim3& block) {
    const int64_t per_block = (int64_t)h->kp.EW * h->kp.waves_per_block;
    const int64_t blocks = (B + per_block - 1) / per_block;
    if (blocks > 0x7FFFFFFFll) return fail(CCX_EINVAL, "%s: batch = %lld needs too many workgroups", who, (long long)B);
    grid = dim3((unsigned)blocks);
    block = dim3(64 * h->shape.waves_per_block);
    return CCX_OK;
}

// Everything ccx_replay_sample / _fetch and ccx_nstep_sample / _fetch check and pass alike: the ring, the outputs, the batch
// and the index, the alignments, the grid.  The kernel takes the handle's kp next to A, lds_bytes_observe of LDS, and the
// 16-byte row stores where N is even.
inline int fetch_args(const char* who, const ccx_handle* h, CCX_RING_PARAMS, int64_t B, const int64_t* index_in, const BatchOut& out,
                      bool draw, FetchArgs& A, dim3& grid, dim3& block) {
    if (int rc = check_ring(who, h, CCX_RING_ARGS, A.ring)) return rc;
    if (!out.actions || !out.reward || !out.done || !out.valid || !out.masks_next || !out.index)
        return fail(CCX_EINVAL, "%s: NULL output (only obs and next_obs may be NULL)", who);
    if (!draw && !index_in) return fail(CCX_EINVAL, "%s: NULL index", who);
    if (int rc = check_batch_size(who, h, B)) return rc;
    if (misaligned(16, out.obs, out.next_obs)) return fail(CCX_EINVAL, "%s: obs and next_obs must be 16-byte aligned", who);
    if (misaligned(8, out.reward, out.index, index_in)) return fail(CCX_EINVAL, "%s: reward and index must be 8-byte aligned", who);
    A.index_in = index_in;
    A.out = out;
    A.B = B;
    A.R = ring_steps * (int64_t)h->E;
    A.S = (int)ring_steps;
    A.E = h->E;
    A.glog = h->shape.glog;
    A.seed_lo = h->rng_lo;
    A.seed_hi = h->rng_hi;
    return gather_grid(who, h, B, grid, block);
}

}  // namespace ccxi
