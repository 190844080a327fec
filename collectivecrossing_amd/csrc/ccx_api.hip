// ccx_api.hip -- the C-ABI of libccx (include/ccx.h) on top of the gfx950 kernels.
//
// Host-side only: argument validation, device memory for the SoA state, launch-shape selection,
// HIP-event timing.  No compute happens here and there is NO CPU fallback: every entry point that
// steps envs launches a kernel or fails with a ccx_status.
#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstdio>
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <new>
#include <string>
#include <vector>

#include "ccx_internal.h"
#include "ccx_plan.h"

namespace {

// a tile's observation region has at most 64 lanes x (3 + 2 * 64) float2 units (+ pad)
constexpr size_t kMaxObsUnits = 64u * (3u + 2u * 64u) + 2u;

thread_local char g_err[512] = "";

}  // namespace

namespace ccxi {
int fail(int code, const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    return code;
}

int row_blocks(const char* who, int64_t rows, int64_t rows_per_block, unsigned& blocks) {
    if (rows < 1) return fail(CCX_EINVAL, "%s: rows must be at least 1, got %lld", who, (long long)rows);
    const int64_t b = (rows + rows_per_block - 1) / rows_per_block;
    if (b > 0x7FFFFFFFll) return fail(CCX_EINVAL, "%s: %lld rows need more than 2^31 - 1 workgroups", who, (long long)rows);
    blocks = (unsigned)b;
    return CCX_OK;
}
}  // namespace ccxi
using ccxi::fail;
using ccxi::misaligned;
using ccxp::ceil_log2;

namespace {

// Per-cell geometry table of the padded grid (layout and rule: ccx_step_rule.h, cell_word).  This is
// config lowering, done once per handle: the reference evaluates the same predicates per agent
// per step (collectivecrossing.py:509-534, 551-563, 663-683; rewards.py:44-182).
std::vector<unsigned long long> build_cell_table(const ccx_params& p, const std::vector<uint8_t>* term_table = nullptr) {
    const int Wp = p.width + 3, Hp = p.height + 3;
    const ccx::CellGeometry g{p.width, p.height, p.division_y, p.tram_left, p.tram_right, p.door_left, p.door_right,
                              p.boarding_dest_y, p.exiting_dest_y};
    // terminateds[id] of agent type t on (x, y) by the user's table (ccx_set_terminated_table), -1 = the built-in rule
    auto user_term = [&](int t, int x, int y) {
        if (!term_table || term_table[t].empty() || x < 0 || x > p.width || y < 0 || y > p.height) return -1;
        return term_table[t][(size_t)y * (size_t)(p.width + 1) + (size_t)x] != 0 ? 1 : 0;
    };
    std::vector<unsigned long long> tab((size_t)Wp * Hp, 0ull);
    for (int y = -1; y <= p.height + 1; ++y)
        for (int x = -1; x <= p.width + 1; ++x)
            tab[(size_t)ccx::cell_index(x, y, Wp)] = ccx::cell_word(g, p.reward_mode, x, y, user_term(0, x, y), user_term(1, x, y));
    return tab;
}

// ---- launch-shape selection: the rules are the pure planner of ccx_plan.hip; everything that touches the handle or the
// device is here ------------------------------------------------------------------------------------------------------
ccxp::PlanIn plan_in_of(const ccx_handle* h, bool rows) {
    ccxp::PlanIn in{};
    in.E = h->E; in.N = h->N; in.width = h->params.width; in.height = h->params.height; in.num_cus = h->num_cus;
    in.reward_table = h->reward_table ? 1 : 0;
    in.term_table = (!h->term_table[0].empty() || !h->term_table[1].empty()) ? 1 : 0;
    in.lanes_per_wave = h->lanes_per_wave; in.waves_per_block = h->waves_per_block; in.writers = h->writers;
    in.store_throttle = h->store_throttle; in.step_pace_ns = h->step_pace_ns; in.pace_start_ns = h->pace_start_ns;
    in.occ_tables = h->tun_occ_tables; in.pair_rows = h->tun_pair_rows; in.writer_roles = h->tun_writer_roles;
    in.pace_phase = h->tun_pace_phase; in.tile_map = h->tun_tile_map;
    in.step_lanes = h->tun_step_lanes; in.step_rows = h->tun_step_rows;
    in.rows = rows ? 1 : 0;
    return in;
}

// the KParams fields that come from the handle's config, not from the launch shape
void fill_config(const ccx_handle* h, ccx::KParams& k) {
    const ccx_params& p = h->params;
    k.W = p.width; k.H = p.height; k.div = p.division_y;
    k.tl = p.tram_left; k.tr = p.tram_right; k.dl = p.door_left; k.dr = p.door_right;
    k.dc = (p.door_left + p.door_right) / 2;  // observations.py:70-71, rewards.py:81
    k.Nb = p.num_boarding; k.N = h->N; k.bdy = p.boarding_dest_y; k.edy = p.exiting_dest_y;
    k.reward_mode = p.reward_mode; k.term_mode = p.terminated_mode; k.max_steps = p.max_steps;
    k.E = h->E;
    k.reward_table = h->reward_table;
    k.off_rtab = h->reward_table ? (uint32_t)ccxp::up16((size_t)(p.width + 3) * (size_t)(p.height + 3) * 8u) : 0u;
    k.user_tables = (h->reward_table || !h->term_table[0].empty() || !h->term_table[1].empty()) ? 1u : 0u;
    k.r_dest = p.boarding_destination_reward; k.r_door = p.tram_door_reward;
    k.r_area = p.tram_area_reward; k.r_f = p.distance_penalty_factor;
    k.r_nogoal = p.no_goal_reward; k.r_pen = p.step_penalty;
    k.env_offset = h->env_offset;
    k.pool_size = h->pool_size;
    // cursor stride of the reset pool: entry (global_env + episode * stride) mod P.  total_envs mod P keeps
    // the walk independent of the world size; when P divides total_envs that would be 0 and every env
    // would restart from ONE placement forever, so the stride is 1 then (env e walks e, e+1, e+2, ...)
    k.pool_stride = h->pool_size > 0 ? (long long)ccx::pool_stride_of((unsigned long long)h->total_envs, (unsigned long long)h->pool_size) : 0;
}

// THE place that writes a plan into the handle: h->shape* / h->kp*, h->step_shape and the controller's start (h->pace); it also uploads the
// observation address table of the rows shape (ccx_kernels.h: obs_unit_addr).  Shape changes are rare and never happen
// inside a graph capture: wait for launches that still read the old table, then copy.
int apply(ccx_handle* h, bool rows, const ccxp::ShapePlan& sp, const ccxp::PacePlan& pp) {
    ccx::LaunchShape& s = rows ? h->shape : h->shape_small;
    ccx::KParams& k = rows ? h->kp : h->kp_small;
    ccxp::materialize(sp, pp, s, k);
    fill_config(h, k);
    k.pace_state = pp.paced ? h->pace.state : nullptr;
    if (rows) {
        h->ring_when_paced = pp.ring_when_paced;
        h->obs_table_host.assign((size_t)k.units_per_wave + 2u, 0);
        for (int w = 0; w < k.units_per_wave; ++w) h->obs_table_host[(size_t)w] = ccx::obs_unit_addr((uint32_t)w, h->N, s.glog);
        CCX_HIP(hipStreamSynchronize(h->stream));
        CCX_HIP(hipMemcpy(h->obs_table, h->obs_table_host.data(), h->obs_table_host.size() * sizeof(uint16_t),
                          hipMemcpyHostToDevice));
        h->pace.init_fp = pp.pace_init_fp;
        h->pace.start_source = pp.pace_start_source;
        h->pace.dirty = true;
        h->pace.needs_calibration = false;
        h->step_shape = sp.step;
    }
    k.obs_table = h->obs_table;
    return CCX_OK;
}

int choose_shape(ccx_handle* h) {
    CCX_HIP(hipSetDevice(h->device));
    for (const bool rows : {true, false}) {
        const ccxp::PlanIn in = plan_in_of(h, rows);
        const ccxp::ShapePlan sp = ccxp::plan_shape(in);
        const int per_cu = ccx::rollout_blocks_per_cu(sp.shape, h->N);
        const int rc = apply(h, rows, sp, ccxp::plan_pacing(in, sp, per_cu));
        if (rc) return rc;
    }
    return CCX_OK;
}

// the kernel parameters of a launch: the planned template of a shape plus the handle's run-time policy state
ccx::KParams launch_params(const ccx_handle* h, bool small_shape = false) {
    ccx::KParams kp = small_shape ? h->kp_small : h->kp;
    kp.rng_lo = h->rng_lo; kp.rng_hi = h->rng_hi; kp.eps_thr = h->eps_thr;
    return kp;
}

int validate_params(const ccx_params* p) {
    if (!p) return fail(CCX_EINVAL, "params is NULL");
    const int n = p->num_boarding + p->num_exiting;
    if (p->num_boarding < 0 || p->num_exiting < 0 || n < 1)
        return fail(CCX_EINVAL, "need at least one agent (got %d boarding + %d exiting)",
                    p->num_boarding, p->num_exiting);
    if (n > 64)
        return fail(CCX_EINVAL, "%d agents per env: libccx supports at most 64 (one wavefront "
                    "lane per agent); the reference itself caps the total at 50 (configs.py:166)", n);
    if (p->width < 1 || p->width > 100 || p->height < 1 || p->height > 100)
        return fail(CCX_EINVAL, "grid %dx%d outside 1..100 (configs.py:39-40)", p->width, p->height);
    if (p->division_y < 1 || p->division_y > 100) return fail(CCX_EINVAL, "division_y out of range");
    if (p->reward_mode < 0 || p->reward_mode > 3) return fail(CCX_EINVAL, "unknown reward_mode %d", p->reward_mode);
    if (p->terminated_mode < 0 || p->terminated_mode > 1)
        return fail(CCX_EINVAL, "unknown terminated_mode %d", p->terminated_mode);
    if (p->truncated_mode != 0) return fail(CCX_EINVAL, "unknown truncated_mode %d", p->truncated_mode);
    if (p->max_steps < 1) return fail(CCX_EINVAL, "max_steps must be >= 1");
    return CCX_OK;
}

int begin_timed(ccx_handle* h) {
    if (h->timing) CCX_HIP(hipEventRecord(h->ev_start, h->stream));
    return CCX_OK;
}
int end_timed(ccx_handle* h) {
    if (h->timing) {
        CCX_HIP(hipEventRecord(h->ev_stop, h->stream));
        h->timed = true;
    }
    return CCX_OK;
}

#ifdef CCX_LAG_TRACE
int* g_lag_buf = nullptr;
#endif

// Start-up calibration of the pace controller.  The adaptive controller needs a start value within
// a few per cent of the rate at which THIS box drains THIS process's write stream; round 2 shipped four learned values
// for the four bench shapes and started every other shape from an assumed 6.8 TB/s.  Now the first paced launch of a
// handle / launch shape measures it: a pure write stream (the writer waves' own store instruction) into the caller's
// trajectory buffer -- the memory the rollout is about to overwrite anyway -- for ~2.5 ms (which also takes the memory
// side through its start-up transient), best pass wins.  The paced rollouts of all shapes settle at 1.05-1.15 x that
// rate (round 3: C2 7.3-7.6 TB/s vs fills of 6.4-7.1 in the same process), so the controller starts 5 % above the
// measured rate and keeps descending at its fast rate until a launch comes in late.  Synchronises the stream once; skipped inside a stream capture, with a caller's start value
// (ccx_set_step_pace_start), with a fixed pace, or with ccx_set_pace_calibration(h, 0) / CCX_PACE_CALIBRATION=0.
// The probe itself: the best rate of `bytes` written to `obs`, in GB/s (0: nothing measured).
int probe_write_rate(const ccx_handle* h, float* obs, size_t bytes, double& best_gbs) {
    hipEvent_t e0 = nullptr, e1 = nullptr;
    CCX_HIP(hipEventCreate(&e0));
    if (hipError_t ee = hipEventCreate(&e1); ee != hipSuccess) {
        (void)hipEventDestroy(e0);
        return fail(CCX_EHIP, "hipEventCreate failed: %s", hipGetErrorString(ee));
    }
    double spent_ms = 0.0;
    int rc = CCX_OK;
    best_gbs = 0.0;
    for (int pass = 0; pass < 24 && spent_ms < 2.5 && rc == CCX_OK; ++pass) {
        float ms = 0.0f;
        hipError_t e = hipEventRecord(e0, h->stream);
        if (e == hipSuccess) e = ccx::launch_write_probe(h->stream, obs, bytes, h->num_cus * 8);
        if (e == hipSuccess) e = hipEventRecord(e1, h->stream);
        if (e == hipSuccess) e = hipEventSynchronize(e1);
        if (e == hipSuccess) e = hipEventElapsedTime(&ms, e0, e1);
        if (e != hipSuccess) rc = fail(CCX_EHIP, "pace calibration probe failed: %s", hipGetErrorString(e));
        else if (ms > 0.0f) {
            spent_ms += ms;
            best_gbs = std::max(best_gbs, (double)bytes / ((double)ms * 1.0e6));
        }
    }
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
    return rc;
}

}  // namespace

int ccxi::PaceController::prepare(const ccx_handle* h, bool paced, bool adaptive, bool capturing, float* obs, size_t obs_bytes) {
    // (re)start the pace controller: new handle, new launch shape or new setting
    // Never inside a stream capture: the memsets would become graph nodes and every replay would re-zero the
    // controller's state, and the calibration must synchronise.  Only a launch that would actually run them
    // is refused while capturing; a controller that has been started (by ANY eager paced launch of the shape) and merely
    // waits for its calibration captures fine and runs at the pace in effect (K = 16..63 on the C2 shape).
    if (dirty && !h->kp.pace_state) {
        dirty = false;                      // rollouts of this shape are not paced at all
        needs_calibration = false;
    }
    if (dirty && paced) {                   // (launches that are not paced never look at the controller: nothing to do yet)
        if (capturing)
            return fail(CCX_EINVAL, "the pace controller of this handle must be (re)started (new handle, launch shape or "
                        "setting): run one eager rollout of this shape (any paced length: >= %u steps) before capturing it "
                        "into a graph, or switch pacing off (ccx_set_step_pace(h, -1))", h->kp.pace_min_k);
        needs_calibration = h->kp.pace_adapt != 0u && h->pace_calibrate && h->pace_start_ns <= 0.0f;
    }
    const bool calibrate_now = needs_calibration && adaptive && !capturing;
    if (!(dirty && paced) && !calibrate_now) return CCX_OK;
    if (calibrate_now) {
        const size_t bytes = std::min<size_t>(obs_bytes & ~(size_t)15, (size_t)3 << 30);
        if (bytes >= ((size_t)16 << 20)) {                    // (else: too small a buffer to say anything about a stream)
            double gbs = 0.0;
            const int rc = probe_write_rate(h, obs, bytes, gbs);
            if (rc) return rc;
            if (gbs > 1000.0 && gbs < 12000.0) {              // (a sane measurement; else keep the assumption)
                probe_gbs = (float)gbs;
                init_fp = std::min(std::max(ccxp::to_fp(h->shape.step_bytes / (gbs * 1.05)), h->kp.pace_min_fp), h->kp.pace_max_fp);
                start_source = CCX_PACE_START_CALIBRATED;
            }
        }
        needs_calibration = false;
    }
    CCX_HIP(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(state), 0, 8, h->stream));   // floor, cliff memory = 0
    CCX_HIP(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(state + slot), (int)init_fp, 1, h->stream));
    // A start value from the caller (ccx_set_step_pace_start: the pace a previous handle of this shape settled at)
    // is also the controller's first FLOOR: a process that already knows its pace skips the descent into a first
    // collapse; the floor decays as always.  A CALIBRATED start gets no floor: the probe is a lower bound of what
    // the paced stream reaches (measured: the paced rollouts settle 5-15 % above a plain fill of the same buffer),
    // so the controller descends from it at its fast rate (1.6 % per launch) until the memory side says stop.
    if (h->step_pace_ns == 0 && h->pace_start_ns > 0.0f)
        CCX_HIP(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(state + 2), (int)init_fp, 1, h->stream));
    // (a paced launch too short to calibrate on runs from the assumption; the first adaptive eager one calibrates
    // and restarts: needs_calibration)
    dirty = false;
    return CCX_OK;
}

namespace {

// ---- one stepping call: what ccx_step, ccx_rollout, ccx_rollout_policy and ccx_rollout_mixed hand to the launch code ----
struct StepCall {     // (the first five fields in the order of ccx_rollout's arguments: the entry points fill them by position)
    int K = 1;                             // env-steps
    const uint8_t* actions = nullptr;      // u8 [K][E][N]; null where `policy` drives every slot
    const uint8_t* order = nullptr;        // u8 [K][E][N] or null
    int auto_reset = 0;
    ccx::KOut out{};
    int policy = 0;                        // in-kernel policy of the rollout kernel (0 = the action tensor)
    uint8_t* actions_out = nullptr;        // ... and where its actions go
    bool inputs_checked = false;           // the entry point has enqueued the input check of the whole call itself
    bool mixed = false;                    // ccx_rollout_mixed: `pol` names the scripted slots and their policy (its actions_out: ours)
    ccx::StepPolicy pol{};
    // what the step kernel may do in its own launch instead of leaving it to finish_call (never given to a sub-launch of a cut)
    uint8_t* masks = nullptr;
    const ccx::StepResetObs* rso = nullptr;
};

// how a call's launches went: the status, and what the launch did itself of the epilogue's work (finish_call does the rest)
struct Launched {
    int rc;
    bool masks_written = false, reset_obs_written = false;
    Launched(int rc_ = CCX_OK) : rc(rc_) {}
};

// ---- the prologue: every check and query the entry points share, each stated once -----------------------------------
template <class Out>   // (ccx_step_out, ccx_rollout_out: the same five pointers)
ccx::KOut kout_of(const Out* out) {
    return out ? ccx::KOut{out->obs, out->reward, out->agent_flags, out->env_flags, out->obs_compact} : ccx::KOut{};
}

// the outputs of step s of a [K][...] trajectory
ccx::KOut kout_at(const ccx_handle* h, const ccx::KOut& ko, int s) {
    const size_t EN = (size_t)h->E * h->N, L = (size_t)(6 + 4 * h->N);
    ccx::KOut o = ko;
    if (o.obs) o.obs += (size_t)s * EN * L;
    if (o.reward) o.reward += (size_t)s * EN;
    if (o.agent_flags) o.agent_flags += (size_t)s * EN;
    if (o.env_flags) o.env_flags += (size_t)s * (size_t)h->E;
    if (o.obs_compact) o.obs_compact += (size_t)s * EN * 4u;
    return o;
}

// the kernels store rows in 16-byte units (ccx_step_finish with an odd agent count: 8) and rewards as doubles
int check_out_align(const ccx::KOut& ko, unsigned obs_align = 16, const char* reward_what = "reward buffer") {
    if (misaligned(obs_align, ko.obs)) return fail(CCX_EINVAL, "obs buffer must be %u-byte aligned", obs_align);
    if (misaligned(8, ko.reward)) return fail(CCX_EINVAL, "%s must be 8-byte aligned", reward_what);
    if (misaligned(16, ko.obs_compact)) return fail(CCX_EINVAL, "obs_compact buffer must be 16-byte aligned");
    return CCX_OK;
}

int need_pool_for_auto_reset(const ccx_handle* h, int auto_reset) {
    if (auto_reset && (!h->pool || h->pool_size <= 0))
        return fail(CCX_EINVAL, "auto_reset needs a reset pool (ccx_set_reset_pool)");
    return CCX_OK;
}

// ccx_set_check_inputs: count the bad bytes of `steps` steps of a caller's tensors (skip_slots: slots a policy scripts)
int enqueue_input_check(ccx_handle* h, int steps, const uint8_t* actions, const uint8_t* order, unsigned long long skip_slots = 0ull) {
    if (!h->check_inputs || (!actions && !order)) return CCX_OK;
    hipError_t ce = ccx::launch_check_inputs(h->stream, actions, order, (size_t)steps * (size_t)h->E, h->N, h->input_errors, skip_slots);
    if (ce != hipSuccess) return fail(CCX_EHIP, "input check kernel launch failed: %s", hipGetErrorString(ce));
    return CCX_OK;
}

bool stream_is_capturing(const ccx_handle* h) {
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(h->stream, &cap) == hipSuccess) return cap != hipStreamCaptureStatusNone;
    (void)hipGetLastError();
    return false;
}

// ---- what the planner is asked (ccx_plan.hip: plan_call, plan_launch): the handle's two shapes, the call and the tunables ----
ccxp::CallFacts call_facts(const ccx_handle* h) {
    return ccxp::CallFacts{h->E, h->N, {ccxp::call_shape(h->shape, h->kp, h->ring_when_paced, h->step_shape.ok != 0),
                                        ccxp::call_shape(h->shape_small, h->kp_small, false, false)}};
}

ccxp::CallIn call_in(const ccx_handle* h, const StepCall& c) {
    ccxp::CallIn in{};
    in.K = c.K; in.actions = c.actions != nullptr; in.order = c.order != nullptr; in.actions_out = c.actions_out != nullptr;
    in.policy = c.policy; in.mixed = c.mixed; in.writes_obs = c.out.obs != nullptr;
    in.masks_bound = c.masks != nullptr; in.reset_obs_on = c.rso != nullptr;
    in.hand2 = h->tun_hand2; in.round_launches = h->tun_round_launches; in.small_shape = h->tun_small_shape;
    in.step_kernel = h->tun_step_kernel; in.max_launch_steps = h->tun_max_launch_steps; in.reset_obs_fused = h->tun_reset_obs_fused;
    return in;
}

// ---- the short launch: the step kernel (ccx_step.hip), CollectiveCrossingEnv.step itself -- no pacing, no controller state,
// no capture query; with the scripted slots of a mixed-control call
Launched launch_short(ccx_handle* h, const StepCall& c, const ccxp::LaunchPlan& lp) {
    int rc = c.inputs_checked ? CCX_OK : enqueue_input_check(h, c.K, c.actions, c.order);
    if (!rc) rc = begin_timed(h);
    if (rc) return rc;
    const ccx::StepPolicy pol{c.pol.scripted, c.pol.policy, c.actions_out};
    // (bound action masks, CCX_RESET_OBS_NEXT: this launch serves them itself where the plan says so; finish_call the rest)
    uint8_t* const m = lp.masks_fused ? c.masks : nullptr;
    const ccx::StepResetObs* const r = lp.reset_obs_fused ? c.rso : nullptr;
    hipError_t e = ccx::launch_step(h->step_shape, h->stream, launch_params(h), h->st_slab, h->cell_info, c.actions, c.order, c.K,
                                    c.auto_reset, h->pool, c.out, h->counters, c.mixed ? &pol : nullptr, m, r, &h->last_key);
    if (e != hipSuccess) return fail(CCX_EHIP, "step kernel launch failed: %s", hipGetErrorString(e));
    Launched l(end_timed(h));
    l.masks_written = m != nullptr, l.reset_obs_written = r != nullptr;
    return l;
}

// ---- the paced launch: the rollout kernel.  First its controller, then the launch itself, round by round where the plan
// says so
int launch_paced(ccx_handle* h, const StepCall& c, const ccxp::LaunchPlan& lp, bool capturing) {
    int rc = h->pace.prepare(h, lp.paced, lp.adaptive, capturing, c.out.obs, ccxp::obs_bytes(h->E, h->N, (size_t)c.K));
    if (rc) return rc;
    h->kp.pace_slot = h->pace.slot;
    if (!c.inputs_checked) rc = enqueue_input_check(h, c.K, c.actions, c.order);
    if (rc) return rc;
    ccx::LaunchShape shape = lp.shape ? h->shape_small : h->shape;
    ccx::KParams kp = launch_params(h, lp.shape != 0);
    kp.pace_slot = h->pace.slot;
    kp.launch_flags = lp.by_rounds ? (uint32_t)ccx::CCX_K_LAUNCH_ROUND : 0u;
    kp.hand_flags = lp.hand_flags;
    kp.pace_adapt = lp.pace_adapt;
#ifdef CCX_LAG_TRACE
    {
        static int* lag_buf = nullptr;
        if (!lag_buf) CCX_HIP(hipMalloc(&lag_buf, 16 * 4096 * sizeof(int)));
        CCX_HIP(hipMemsetAsync(lag_buf, 0x80, 16 * 4096 * sizeof(int), h->stream));
        kp.lag_trace = lag_buf;
        const int tiles_ = shape.num_blocks * shape.waves_per_block;
        kp.lag_every = tiles_ >= 16 ? tiles_ / 16 : 1;
        g_lag_buf = lag_buf;
    }
#endif
    rc = begin_timed(h);
    if (rc) return rc;
    // (one launch of the whole grid is the one "round" of a plan that is not by rounds: per_round = the grid)
    const int num_blocks = shape.num_blocks;
    hipError_t e = hipSuccess;
    for (int b0 = 0; b0 < num_blocks && e == hipSuccess; b0 += lp.per_round) {
        shape.num_blocks = std::min(lp.per_round, num_blocks - b0);
        kp.block_base = (uint32_t)b0;
        e = ccx::launch_rollout(shape, h->stream, kp, h->st, h->cell_info, c.actions,
                                c.order, c.K, c.auto_reset, h->pool, c.out, h->counters, c.policy, c.actions_out, &h->last_key);
    }
    if (e != hipSuccess) return fail(CCX_EHIP, "rollout kernel launch failed: %s", hipGetErrorString(e));
    if (lp.flip_slot) h->pace.slot ^= 1u;
    return end_timed(h);
}

// one launch of a call: the step kernel where the plan says so, else the rollout kernel.  Only the latter asks whether the
// stream is being captured, and a capturing stream has the launch planned again with that answer.
Launched launch_one(ccx_handle* h, const StepCall& c, const ccxp::CallFacts& f, const ccxp::CallIn& in) {
    const int rc = check_out_align(c.out);
    if (rc) return rc;
    CCX_HIP(hipSetDevice(h->device));
    ccxp::LaunchPlan lp = ccxp::plan_launch(f, in, c.K);
    if (lp.kernel == ccxp::KERNEL_STEP) return launch_short(h, c, lp);
    const bool capturing = stream_is_capturing(h);
    if (capturing) {
        ccxp::CallIn captured = in;
        captured.capturing = 1;
        lp = ccxp::plan_launch(f, captured, c.K);
    }
    return launch_paced(h, c, lp, capturing);
}

// ---- the cutter: a call as one launch, or as several of the plan's length --------------------------------------------------
Launched run_rollout(ccx_handle* h, const StepCall& c) {
    const ccxp::CallFacts f = call_facts(h);
    const ccxp::CallIn in = call_in(h, c);
    const ccxp::CallPlan cp = ccxp::plan_call(f, in);
    if (cp.refused)
        return fail(CCX_EINVAL, "a rollout of an odd number of agent slots (E x N = %lld) cannot be cut into launches of "
                    "one step: its per-step observation slabs are not 16-byte aligned (raise max_launch_steps to >= 2)",
                    (long long)h->E * h->N);
    if (cp.launches == 1) return launch_one(h, c, f, in);
    const size_t EN = (size_t)h->E * h->N;
    for (int k0 = 0; k0 < c.K; k0 += cp.steps_per_launch) {
        StepCall sub = c;
        sub.K = std::min(cp.steps_per_launch, c.K - k0);
        if (c.actions) sub.actions = c.actions + (size_t)k0 * EN;
        if (c.order) sub.order = c.order + (size_t)k0 * EN;
        if (c.actions_out) sub.actions_out = c.actions_out + (size_t)k0 * EN;
        sub.out = kout_at(h, c.out, k0);
        // (the sub-launches get neither `masks` nor `rso`: the plan fuses them into a call of one step only)
        sub.masks = nullptr;
        sub.rso = nullptr;
        const Launched l = launch_one(h, sub, f, in);
        if (l.rc) return l;
    }
    return CCX_OK;
}

// CCX_RESET_OBS: does this call have rows to redirect at all?  (Without auto-reset or a pool no step raises CCX_EF_RESET.)
bool reset_obs_on(const ccx_handle* h, const ccx::KOut& ko, int auto_reset) {
    return h->reset_obs == CCX_RESET_OBS_NEXT && auto_reset != 0 && h->pool != nullptr && h->pool_size > 0 &&
           (ko.obs != nullptr || ko.obs_compact != nullptr);
}

int check_reset_obs(const ccx_handle* h, const ccx::KOut& ko, int auto_reset) {
    if (!reset_obs_on(h, ko, auto_reset)) return CCX_OK;
    if (!ko.env_flags)
        return fail(CCX_EINVAL, "CCX_RESET_OBS_NEXT: a call with auto-reset that asks for obs or obs_compact must pass env_flags "
                    "too (the restarted envs are found there)");
    const unsigned align = (h->N % 2) == 0 ? 16u : 8u;
    if (ko.obs && misaligned(align, h->bound_final_obs)) return fail(CCX_EINVAL, "final_obs buffer must be %u-byte aligned", align);
    if (ko.obs_compact && misaligned(16, h->bound_final_compact))
        return fail(CCX_EINVAL, "final_compact buffer must be 16-byte aligned");
    return CCX_OK;
}

// ---- the epilogue of EVERY call that advanced the state by K steps, behind its last launch, for what `l` did not do itself:
// ccx_bind_action_masks -- the masks of the final state at the bound pointer (the stand-alone mask kernel);
// CCX_RESET_OBS_NEXT -- the restarted rows at the CCX_EF_RESET pairs of a call that wrote rows with auto-reset (the fix-up
// kernel, once for the whole call, from the episode counters the last launch left: ccx_reset_obs.hip)
int finish_call(ccx_handle* h, int K, const ccx::KOut& ko, int auto_reset, const Launched& l) {
    if (l.rc) return l.rc;
    if (h->bound_masks && !l.masks_written) {
        hipError_t e = ccx::launch_action_masks(h->stream, launch_params(h), h->st, h->cell_info, h->bound_masks);
        if (e != hipSuccess) return fail(CCX_EHIP, "action mask kernel launch failed: %s", hipGetErrorString(e));
    }
    if (!l.reset_obs_written && reset_obs_on(h, ko, auto_reset)) {
        hipError_t e = ccx::launch_reset_obs(h->stream, launch_params(h), h->st, K, ko.env_flags, h->pool, ko.obs, ko.obs_compact,
                                             ko.obs ? h->bound_final_obs : nullptr, ko.obs_compact ? h->bound_final_compact : nullptr);
        if (e != hipSuccess) return fail(CCX_EHIP, "reset-observation kernel launch failed: %s", hipGetErrorString(e));
    }
    return CCX_OK;
}

// ---- the loop that steps ONE env-step per launch (the MT19937 policy loop, the unfused mixed-control step) ---------------
// Its scratch buffers, allocated on first use and never inside a stream capture: one step's actions (unless the caller's
// actions_out takes them) and, where a step's slice of the observation tensor is not 16-byte aligned (E x N x L x 4 not a
// multiple of 16), an aligned staging slab.
int stepwise_scratch(ccx_handle* h, const StepCall& c, const char* what) {
    const size_t EN = (size_t)h->E * h->N, slab = ccxp::obs_bytes(h->E, h->N);
    const bool own_actions = !c.actions_out && !h->stream_actions;
    const bool staging = c.out.obs && (slab & 15u) && c.K > 1 && !h->stream_obs;
    if (!own_actions && !staging) return CCX_OK;
    if (stream_is_capturing(h))
        return fail(CCX_EINVAL, "%s allocates scratch buffers on first use: run one eager call of this shape before "
                    "capturing it into a graph", what);
    if (own_actions) CCX_HIP(hipMalloc(&h->stream_actions, EN));
    if (staging) CCX_HIP(hipMalloc(&h->stream_obs, slab));
    return CCX_OK;
}

// `produce_actions(s, acts)` enqueues what leaves step s's actions at `acts`; the step goes through the ordinary launch
// path, its observation rows staged where their slice is misaligned
template <class Produce>
Launched run_stepwise(ccx_handle* h, const StepCall& c, const char* what, Produce produce_actions) {
    const size_t EN = (size_t)h->E * h->N, slab = ccxp::obs_bytes(h->E, h->N);
    int rc = stepwise_scratch(h, c, what);
    for (int s = 0; s < c.K && !rc; ++s) {
        uint8_t* const acts = c.actions_out ? c.actions_out + (size_t)s * EN : h->stream_actions;
        StepCall step{1, acts, c.order ? c.order + (size_t)s * EN : nullptr, c.auto_reset, kout_at(h, c.out, s)};
        step.inputs_checked = c.inputs_checked;
        float* const obs_dst = step.out.obs;
        const bool staged = misaligned(16, obs_dst);
        if (staged) {
            if (!h->stream_obs) return fail(CCX_EINVAL, "obs buffer must be 16-byte aligned");   // (a misaligned BASE)
            step.out.obs = h->stream_obs;
        }
        rc = produce_actions(s, acts);
        if (!rc) rc = run_rollout(h, step).rc;
        if (!rc && staged) CCX_HIP(hipMemcpyAsync(obs_dst, h->stream_obs, slab, hipMemcpyDeviceToDevice, h->stream));
    }
    return rc;
}

}  // namespace

extern "C" {

int ccx_abi_version(void) { return CCX_ABI_VERSION; }

const char* ccx_build_info(void) {
    static char buf[128];
    snprintf(buf, sizeof(buf), "libccx 0.5.0 abi %d gfx950 hip %d.%d", CCX_ABI_VERSION,
             HIP_VERSION_MAJOR, HIP_VERSION_MINOR);
    return buf;
}

const char* ccx_last_error(void) { return g_err; }

int32_t ccx_obs_len(int32_t num_agents) { return 2 + 4 + 4 * num_agents; }

int ccx_create(const ccx_params* params, int32_t num_envs, int64_t env_offset, int64_t total_envs,
               int device, void* stream, ccx_handle** out) {
    if (!out) return fail(CCX_EINVAL, "out is NULL");
    *out = nullptr;
    int rc = validate_params(params);
    if (rc) return rc;
    if (num_envs < 1) return fail(CCX_EINVAL, "num_envs must be >= 1 (got %d)", num_envs);
    if ((long long)num_envs * (params->num_boarding + params->num_exiting) >= (1ll << 28))
        return fail(CCX_EINVAL, "num_envs x agents = %lld exceeds 2^28 (per-lane byte offsets are 32-bit)",
                    (long long)num_envs * (params->num_boarding + params->num_exiting));
    if (total_envs <= 0) total_envs = num_envs;
    // (as a difference: env_offset + num_envs overflows for offsets near INT64_MAX and would let a bad shard through)
    if (env_offset < 0 || total_envs < num_envs || env_offset > total_envs - num_envs)
        return fail(CCX_EINVAL, "env_offset %lld + num_envs %d exceeds total_envs %lld",
                    (long long)env_offset, num_envs, (long long)total_envs);
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1)
        return fail(CCX_ENODEVICE, "no HIP device visible: libccx has no CPU path");
    if (device < 0 || device >= ndev) return fail(CCX_EINVAL, "device %d out of range (%d visible)", device, ndev);
    hipDeviceProp_t prop;
    CCX_HIP(hipGetDeviceProperties(&prop, device));
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        return fail(CCX_ENODEVICE, "device %d is %s; libccx carries gfx950 (MI355X) code only", device,
                    prop.gcnArchName);
    CCX_HIP(hipSetDevice(device));

    ccx_handle* h = new (std::nothrow) ccx_handle();
    if (!h) return fail(CCX_ENOMEM, "host allocation failed");
    h->params = *params;
    h->E = num_envs;
    h->N = params->num_boarding + params->num_exiting;
    h->env_offset = env_offset;
    h->total_envs = total_envs;
    h->device = device;
    h->stream = reinterpret_cast<hipStream_t>(stream);
    const size_t en = (size_t)h->E * h->N;
    hipError_t e = hipSuccess;
    auto alloc = [&](void** p, size_t bytes) {
        if (e == hipSuccess) e = hipMalloc(p, bytes);
    };
    {   // the seven state arrays: ONE allocation (ccx_kernels.h: StateSlab), so that the short-launch kernel needs one pointer
        const ccx::StateSlab sl = ccx::state_slab(h->E, h->N);
        alloc((void**)&h->st_slab, sl.total);
        if (e == hipSuccess) {
            h->st.x = reinterpret_cast<int32_t*>(h->st_slab + sl.x);
            h->st.y = reinterpret_cast<int32_t*>(h->st_slab + sl.y);
            h->st.active = h->st_slab + sl.active;
            h->st.terminated = h->st_slab + sl.terminated;
            h->st.truncated = h->st_slab + sl.truncated;
            h->st.step_count = reinterpret_cast<int32_t*>(h->st_slab + sl.step_count);
            h->st.episode = reinterpret_cast<int32_t*>(h->st_slab + sl.episode);
        }
    }
    alloc((void**)&h->counters, ccx::counter_words(h->E) * sizeof(unsigned long long));
    alloc((void**)&h->placement_scratch, en * 2);
    alloc((void**)&h->pace.state, 8 * sizeof(uint32_t));
    alloc((void**)&h->input_errors, 2 * sizeof(unsigned long long));
    alloc((void**)&h->obs_table, kMaxObsUnits * sizeof(uint16_t));
    if (hipDeviceGetAttribute(&h->num_cus, hipDeviceAttributeMultiprocessorCount, h->device) != hipSuccess ||
        h->num_cus < 1)
        h->num_cus = 256;
    const std::vector<unsigned long long> cell_tab = build_cell_table(*params);
    alloc((void**)&h->cell_info, cell_tab.size() * sizeof(unsigned long long));
    if (e == hipSuccess)
        e = hipMemcpy(h->cell_info, cell_tab.data(), cell_tab.size() * sizeof(unsigned long long),
                      hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipEventCreate(&h->ev_start);
    if (e == hipSuccess) e = hipEventCreate(&h->ev_stop);
    if (e == hipSuccess) e = hipMemsetAsync(h->st.x, 0, en * 4, h->stream);
    if (e == hipSuccess) e = hipMemsetAsync(h->st.y, 0, en * 4, h->stream);
    if (e == hipSuccess) e = hipMemsetAsync(h->st.active, 1, en, h->stream);
    if (e == hipSuccess) e = hipMemsetAsync(h->st.terminated, 0, en, h->stream);
    if (e == hipSuccess) e = hipMemsetAsync(h->st.truncated, 0, en, h->stream);
    if (e == hipSuccess) e = hipMemsetAsync(h->st.step_count, 0, (size_t)h->E * 4, h->stream);
    if (e == hipSuccess) e = hipMemsetAsync(h->st.episode, 0, (size_t)h->E * 4, h->stream);
    if (e == hipSuccess)
        e = hipMemsetAsync(h->counters, 0, ccx::counter_words(h->E) * sizeof(unsigned long long), h->stream);
    if (e == hipSuccess) e = hipMemsetAsync(h->input_errors, 0, 2 * sizeof(unsigned long long), h->stream);
    if (e != hipSuccess) {
        int code = (e == hipErrorOutOfMemory) ? CCX_ENOMEM : CCX_EHIP;
        fail(code, "ccx_create: %s", hipGetErrorString(e));
        ccx_destroy(h);
        return code;
    }
    if (const char* ev = getenv("CCX_PACE_CALIBRATION")) h->pace_calibrate = !(ev[0] == '0' && ev[1] == 0);
    rc = choose_shape(h);
    if (rc) {
        ccx_destroy(h);
        return rc;
    }
    *out = h;
    return CCX_OK;
}

void ccx_destroy(ccx_handle* h) {
    if (!h) return;
    (void)hipSetDevice(h->device);
    (void)hipStreamSynchronize(h->stream);
    (void)hipFree(h->st_slab);
    (void)hipFree(h->counters);
    (void)hipFree(h->pace.state);
    (void)hipFree(h->input_errors);
    (void)hipFree(h->obs_table);
    (void)hipFree(h->cell_info);
    (void)hipFree(h->reward_table);
    (void)hipFree(h->placement_scratch);
    (void)hipFree(h->mt_state);
    (void)hipFree(h->stream_actions);
    (void)hipFree(h->stream_obs);
    ccxi::episode_stats_destroy(h);
    if (h->ev_start) (void)hipEventDestroy(h->ev_start);
    if (h->ev_stop) (void)hipEventDestroy(h->ev_stop);
    delete h;
}

int32_t ccx_num_envs(const ccx_handle* h) { return h ? h->E : 0; }
int32_t ccx_num_agents(const ccx_handle* h) { return h ? h->N : 0; }

int ccx_state_view(ccx_handle* h, ccx_state* out) {
    if (!h || !out) return fail(CCX_EINVAL, "NULL argument");
    out->x = h->st.x;
    out->y = h->st.y;
    out->active = h->st.active;
    out->terminated = h->st.terminated;
    out->truncated = h->st.truncated;
    out->step_count = h->st.step_count;
    out->episode = h->st.episode;
    return CCX_OK;
}

int ccx_set_state_host(ccx_handle* h, const ccx_state* src) {
    if (!h || !src) return fail(CCX_EINVAL, "NULL argument");
    const size_t en = (size_t)h->E * h->N;
    if (src->x)
        for (size_t t = 0; t < en; ++t)
            if (src->x[t] < 0 || src->x[t] > h->params.width)
                return fail(CCX_EINVAL, "x[%zu] = %d outside 0..width=%d (collectivecrossing.py:515)", t,
                            src->x[t], h->params.width);
    if (src->y)
        for (size_t t = 0; t < en; ++t)
            if (src->y[t] < 0 || src->y[t] > h->params.height)
                return fail(CCX_EINVAL, "y[%zu] = %d outside 0..height=%d (collectivecrossing.py:515)", t,
                            src->y[t], h->params.height);
    const uint8_t* flags[3] = {src->active, src->terminated, src->truncated};
    for (const uint8_t* f : flags)
        if (f)
            for (size_t t = 0; t < en; ++t)
                if (f[t] > 1) return fail(CCX_EINVAL, "flag value %u at %zu is not 0/1", f[t], t);
    if (src->step_count)
        for (int32_t e = 0; e < h->E; ++e)
            if (src->step_count[e] < 0) return fail(CCX_EINVAL, "negative step_count");
    if (src->episode)
        for (int32_t e = 0; e < h->E; ++e)
            if (src->episode[e] < 0) return fail(CCX_EINVAL, "negative episode");
    CCX_HIP(hipSetDevice(h->device));
    CCX_HIP(hipStreamSynchronize(h->stream));
    if (src->x) CCX_HIP(hipMemcpy(h->st.x, src->x, en * 4, hipMemcpyHostToDevice));
    if (src->y) CCX_HIP(hipMemcpy(h->st.y, src->y, en * 4, hipMemcpyHostToDevice));
    if (src->active) CCX_HIP(hipMemcpy(h->st.active, src->active, en, hipMemcpyHostToDevice));
    if (src->terminated) CCX_HIP(hipMemcpy(h->st.terminated, src->terminated, en, hipMemcpyHostToDevice));
    if (src->truncated) CCX_HIP(hipMemcpy(h->st.truncated, src->truncated, en, hipMemcpyHostToDevice));
    if (src->step_count)
        CCX_HIP(hipMemcpy(h->st.step_count, src->step_count, (size_t)h->E * 4, hipMemcpyHostToDevice));
    if (src->episode) CCX_HIP(hipMemcpy(h->st.episode, src->episode, (size_t)h->E * 4, hipMemcpyHostToDevice));
    return CCX_OK;
}

int ccx_get_state_host(ccx_handle* h, ccx_state* dst) {
    if (!h || !dst) return fail(CCX_EINVAL, "NULL argument");
    const size_t en = (size_t)h->E * h->N;
    CCX_HIP(hipSetDevice(h->device));
    CCX_HIP(hipStreamSynchronize(h->stream));
    if (dst->x) CCX_HIP(hipMemcpy(dst->x, h->st.x, en * 4, hipMemcpyDeviceToHost));
    if (dst->y) CCX_HIP(hipMemcpy(dst->y, h->st.y, en * 4, hipMemcpyDeviceToHost));
    if (dst->active) CCX_HIP(hipMemcpy(dst->active, h->st.active, en, hipMemcpyDeviceToHost));
    if (dst->terminated) CCX_HIP(hipMemcpy(dst->terminated, h->st.terminated, en, hipMemcpyDeviceToHost));
    if (dst->truncated) CCX_HIP(hipMemcpy(dst->truncated, h->st.truncated, en, hipMemcpyDeviceToHost));
    if (dst->step_count)
        CCX_HIP(hipMemcpy(dst->step_count, h->st.step_count, (size_t)h->E * 4, hipMemcpyDeviceToHost));
    if (dst->episode) CCX_HIP(hipMemcpy(dst->episode, h->st.episode, (size_t)h->E * 4, hipMemcpyDeviceToHost));
    return CCX_OK;
}

int ccx_set_reset_pool(ccx_handle* h, const uint8_t* pool_xy, int64_t pool_size) {
    if (!h) return fail(CCX_EINVAL, "NULL handle");
    if ((pool_xy == nullptr) != (pool_size == 0) || pool_size < 0 || pool_size >= (1ll << 31))
        return fail(CCX_EINVAL, "bad reset pool (ptr %p, size %lld)", (const void*)pool_xy, (long long)pool_size);
    if (misaligned(2, pool_xy)) return fail(CCX_EINVAL, "pool must be 2-byte aligned");
    h->pool = pool_xy;
    h->pool_size = pool_size;
    return choose_shape(h);
}

int ccx_reset_from_pool(ccx_handle* h, const uint8_t* env_mask) {
    if (!h) return fail(CCX_EINVAL, "NULL handle");
    if (!h->pool || h->pool_size <= 0) return fail(CCX_EINVAL, "no reset pool set (ccx_set_reset_pool)");
    CCX_HIP(hipSetDevice(h->device));
    hipError_t e = ccx::launch_reset_from_pool(h->stream, h->kp, h->st, env_mask, h->pool);
    if (e != hipSuccess) return fail(CCX_EHIP, "reset kernel launch failed: %s", hipGetErrorString(e));
    if (h->stats_on) return ccxi::episode_stats_reset(h, env_mask);
    return CCX_OK;
}

namespace {
// counters[7] collects placements that did not converge (the reference would spin forever)
int finish_placement(ccx_handle* h, const char* what) {
    unsigned long long fails = 0;
    CCX_HIP(hipStreamSynchronize(h->stream));
    CCX_HIP(hipMemcpy(&fails, h->counters + 7, sizeof(fails), hipMemcpyDeviceToHost));
    if (fails) {
        CCX_HIP(hipMemset(h->counters + 7, 0, sizeof(fails)));
        return fail(CCX_EINVAL, "%s: %llu placement(s) found no free cell within %d draws per agent "
                    "(the reference's rejection sampling would not terminate either)", what, fails, 1 << 16);
    }
    return CCX_OK;
}
}  // namespace

int ccx_fill_reset_pool_seeded(ccx_handle* h, uint8_t* pool_xy, int64_t pool_size, uint64_t seed0) {
    if (!h || !pool_xy) return fail(CCX_EINVAL, "NULL argument");
    if (pool_size < 1 || pool_size >= (1ll << 31)) return fail(CCX_EINVAL, "bad pool_size %lld", (long long)pool_size);
    CCX_HIP(hipSetDevice(h->device));
    hipError_t e = ccx::launch_seeded_placement(h->stream, h->kp, (int)pool_size, nullptr, seed0, pool_xy,
                                                h->st, nullptr, nullptr, 1 << 16, h->counters + 7);
    if (e != hipSuccess) return fail(CCX_EHIP, "placement kernel launch failed: %s", hipGetErrorString(e));
    return finish_placement(h, "ccx_fill_reset_pool_seeded");
}

int ccx_reset_seeded(ccx_handle* h, const uint64_t* seeds, const uint8_t* env_mask) {
    if (!h || !seeds) return fail(CCX_EINVAL, "NULL argument");
    CCX_HIP(hipSetDevice(h->device));
    hipError_t e = ccx::launch_seeded_placement(h->stream, h->kp, h->E, seeds, 0, nullptr, h->st, env_mask,
                                                h->placement_scratch, 1 << 16, h->counters + 7);
    if (e != hipSuccess) return fail(CCX_EHIP, "placement kernel launch failed: %s", hipGetErrorString(e));
    if (h->stats_on) {
        const int rc = ccxi::episode_stats_reset(h, env_mask);
        if (rc != CCX_OK) return rc;
    }
    return finish_placement(h, "ccx_reset_seeded");
}

int ccx_policy_actions(ccx_handle* h, int32_t policy, uint8_t* actions) {
    if (!h || !actions) return fail(CCX_EINVAL, "NULL argument");
    if (policy != CCX_POLICY_GREEDY && policy != CCX_POLICY_WAITING) return fail(CCX_EINVAL, "unknown policy %d", policy);
    CCX_HIP(hipSetDevice(h->device));
    hipError_t e = h->eps_stream == CCX_EPS_STREAM_MT19937
        ? ccx::launch_policy_stream_actions(h->stream, launch_params(h), h->st, h->cell_info, actions, policy, h->mt_state, h->epsilon)
        : ccx::launch_greedy_actions(h->stream, launch_params(h), h->st, h->cell_info, actions, policy);
    if (e != hipSuccess) return fail(CCX_EHIP, "policy kernel launch failed: %s", hipGetErrorString(e));
    return CCX_OK;
}

int ccx_greedy_actions(ccx_handle* h, uint8_t* actions) {
    if (!h || !actions) return fail(CCX_EINVAL, "NULL argument");
    CCX_HIP(hipSetDevice(h->device));
    ccx::KParams kp = launch_params(h);
    kp.eps_thr = 0u;                               // (always the deterministic policy; ccx_policy_actions has the epsilon)
    hipError_t e = ccx::launch_greedy_actions(h->stream, kp, h->st, h->cell_info, actions, CCX_POLICY_GREEDY);
    if (e != hipSuccess) return fail(CCX_EHIP, "greedy kernel launch failed: %s", hipGetErrorString(e));
    return CCX_OK;
}

int ccx_observe(ccx_handle* h, float* obs) {
    if (!h || !obs) return fail(CCX_EINVAL, "NULL argument");
    if (misaligned(16, obs)) return fail(CCX_EINVAL, "obs buffer must be 16-byte aligned");
    CCX_HIP(hipSetDevice(h->device));
    hipError_t e = ccx::launch_observe(h->shape, h->stream, h->kp, h->st, obs, &h->last_observe_key);
    if (e != hipSuccess) return fail(CCX_EHIP, "observe kernel launch failed: %s", hipGetErrorString(e));
    return CCX_OK;
}

int ccx_expand_observations(ccx_handle* h, const float* obs_compact, int64_t rows, float* obs) {
    if (!h || !obs_compact || !obs) return fail(CCX_EINVAL, "NULL argument");
    if (rows < 0 || rows * (int64_t)h->N >= (1ll << 31)) return fail(CCX_EINVAL, "rows = %lld out of range", (long long)rows);
    if (misaligned(16, obs, obs_compact))
        return fail(CCX_EINVAL, "obs and obs_compact must be 16-byte aligned");
    CCX_HIP(hipSetDevice(h->device));
    hipError_t e = ccx::launch_expand(h->shape, h->stream, h->kp, obs_compact, rows, obs, &h->last_observe_key);
    if (e != hipSuccess) return fail(CCX_EHIP, "expand kernel launch failed: %s", hipGetErrorString(e));
    return CCX_OK;
}

int ccx_step(ccx_handle* h, const uint8_t* actions, const uint8_t* order, const ccx_step_out* out) {
    if (!h || !actions) return fail(CCX_EINVAL, "NULL argument");
    StepCall c{1, actions, order, 0, kout_of(out)};
    c.masks = h->bound_masks;
    return finish_call(h, 1, c.out, 0, run_rollout(h, c));
}

int ccx_step_begin(ccx_handle* h, const uint8_t* actions, const uint8_t* order) {
    if (!h || !actions) return fail(CCX_EINVAL, "NULL argument");
    CCX_HIP(hipSetDevice(h->device));
    int rc = enqueue_input_check(h, 1, actions, order);
    if (!rc) rc = begin_timed(h);
    if (rc) return rc;
    hipError_t e = ccx::launch_step_begin(h->stream, h->kp, h->st, ceil_log2(h->N), actions, order, h->counters);
    if (e != hipSuccess) return fail(CCX_EHIP, "step_begin kernel launch failed: %s", hipGetErrorString(e));
    return end_timed(h);
}

int ccx_step_finish(ccx_handle* h, const double* reward, const int8_t* terminated, const uint8_t* truncated,
                    const ccx_step_out* out, uint8_t* term_present, int32_t auto_reset) {
    if (!h) return fail(CCX_EINVAL, "NULL handle");
    int rc = need_pool_for_auto_reset(h, auto_reset);
    if (rc) return rc;
    const ccx::KOut ko = kout_of(out);
    // (odd agent counts write the rows in 8-byte units: csrc/ccx_split_step.hip, PAIR = false)
    rc = check_out_align(ko, (h->N % 2) == 0 ? 16 : 8, "reward buffers");
    if (!rc && misaligned(8, reward)) rc = fail(CCX_EINVAL, "reward buffers must be 8-byte aligned");
    if (!rc) rc = check_reset_obs(h, ko, auto_reset);
    if (rc) return rc;
    CCX_HIP(hipSetDevice(h->device));
    rc = begin_timed(h);
    if (rc) return rc;
    hipError_t e = ccx::launch_step_finish(h->shape, h->stream, h->kp, h->st, h->cell_info, reward, terminated, truncated, ko,
                                           term_present, auto_reset ? 1 : 0, h->pool, h->counters);
    if (e != hipSuccess) return fail(CCX_EHIP, "step_finish kernel launch failed: %s", hipGetErrorString(e));
    return finish_call(h, 1, ko, auto_reset, end_timed(h));
}

int ccx_rollout(ccx_handle* h, int32_t num_steps, const uint8_t* actions, const uint8_t* order,
                int32_t auto_reset, const ccx_rollout_out* out) {
    if (!h || !actions) return fail(CCX_EINVAL, "NULL argument");
    if (num_steps < 1) return fail(CCX_EINVAL, "num_steps must be >= 1");
    int rc = need_pool_for_auto_reset(h, auto_reset);
    if (rc) return rc;
    StepCall c{num_steps, actions, order, auto_reset ? 1 : 0, kout_of(out)};
    rc = check_reset_obs(h, c.out, auto_reset);
    if (rc) return rc;
    const ccx::StepResetObs rso{c.out.obs ? h->bound_final_obs : nullptr, c.out.obs_compact ? h->bound_final_compact : nullptr};
    c.masks = h->bound_masks;
    c.rso = reset_obs_on(h, c.out, auto_reset) ? &rso : nullptr;
    return finish_call(h, num_steps, c.out, auto_reset, run_rollout(h, c));
}

int ccx_rollout_policy(ccx_handle* h, int32_t num_steps, int32_t policy, int32_t auto_reset,
                       const ccx_rollout_out* out, uint8_t* actions_out) {
    if (!h) return fail(CCX_EINVAL, "NULL handle");
    if (num_steps < 1) return fail(CCX_EINVAL, "num_steps must be >= 1");
    if (policy != CCX_POLICY_GREEDY && policy != CCX_POLICY_WAITING && policy != CCX_POLICY_RANDOM)
        return fail(CCX_EINVAL, "unknown policy %d", policy);
    int rc = need_pool_for_auto_reset(h, auto_reset);
    if (rc) return rc;
    const StepCall c{num_steps, nullptr, nullptr, auto_reset ? 1 : 0, kout_of(out), policy, actions_out};
    rc = check_reset_obs(h, c.out, auto_reset);
    if (rc) return rc;
    if (h->eps_stream == CCX_EPS_STREAM_MT19937 && policy != CCX_POLICY_RANDOM && h->epsilon > 0.0) {
        // The reference's stream is sequential per env: the policy runs as its own kernel between the steps (policy -> step
        // -> policy ..., each a launch on the handle's stream) instead of inside the fused one.  Meant for replaying the
        // reference's epsilon episodes action for action, not for throughput.
        CCX_HIP(hipSetDevice(h->device));
        auto mt_policy = [&](int, uint8_t* acts) {
            hipError_t e = ccx::launch_policy_stream_actions(h->stream, launch_params(h), h->st, h->cell_info, acts, policy, h->mt_state,
                                                             h->epsilon);
            return e == hipSuccess ? (int)CCX_OK : fail(CCX_EHIP, "policy kernel launch failed: %s", hipGetErrorString(e));
        };
        return finish_call(h, num_steps, c.out, auto_reset, run_stepwise(h, c, "the stepwise policy loop", mt_policy));
    }
    // (grids whose occupancy tables exceed the LDS run the in-kernel policies through the all-pairs exchange: round 4)
    return finish_call(h, num_steps, c.out, auto_reset, run_rollout(h, c));
}

int ccx_rollout_mixed(ccx_handle* h, int32_t num_steps, int32_t policy, uint64_t scripted_slots,
                      const uint8_t* actions, const uint8_t* order, int32_t auto_reset,
                      const ccx_rollout_out* out, uint8_t* actions_out) {
    if (!h) return fail(CCX_EINVAL, "NULL handle");
    if (num_steps < 1) return fail(CCX_EINVAL, "num_steps must be >= 1");
    if (policy != CCX_POLICY_GREEDY && policy != CCX_POLICY_WAITING)
        return fail(CCX_EINVAL, "a mixed-control step scripts CCX_POLICY_GREEDY or CCX_POLICY_WAITING (got policy %d)", policy);
    const uint64_t all_slots = h->N >= 64 ? ~0ull : ((1ull << h->N) - 1ull);
    if (scripted_slots & ~all_slots)
        return fail(CCX_EINVAL, "scripted_slots 0x%llx names agent slots at or above N = %d",
                    (unsigned long long)scripted_slots, h->N);
    if (!actions && scripted_slots != all_slots)
        return fail(CCX_EINVAL, "actions may be NULL only when scripted_slots covers all %d slots (got 0x%llx)", h->N,
                    (unsigned long long)scripted_slots);
    int rc = need_pool_for_auto_reset(h, auto_reset);
    if (rc) return rc;
    if (h->eps_stream == CCX_EPS_STREAM_MT19937 && h->epsilon > 0.0)
        return fail(CCX_EINVAL, "a mixed-control step cannot draw from the MT19937 exploration stream: that stream is "
                    "sequential per env and walked by a kernel of its own (ccx_policy_actions); select "
                    "CCX_EPS_STREAM_COUNTER or set epsilon to 0");
    StepCall c{num_steps, actions, order, auto_reset ? 1 : 0, kout_of(out), 0, actions_out, /*inputs_checked=*/true};
    c.mixed = true;
    c.pol = ccx::StepPolicy{scripted_slots, policy, nullptr};
    c.masks = h->bound_masks;
    rc = check_out_align(c.out);
    if (!rc) rc = check_reset_obs(h, c.out, auto_reset);
    if (rc) return rc;
    CCX_HIP(hipSetDevice(h->device));
    const size_t EN = (size_t)h->E * h->N;
    // ccx_set_check_inputs: the caller's bytes outside the mask and the order rows, once, on either path
    rc = enqueue_input_check(h, num_steps, actions, order, scripted_slots);
    if (rc) return rc;
    // policy + merge + step in the launches of the step kernel (the cutter, like every other call) ...
    if (!ccxp::plan_call(call_facts(h), call_in(h, c)).stepwise)
        return finish_call(h, num_steps, c.out, auto_reset, run_rollout(h, c));
    // ... or, on handles whose short launches cannot use the step kernel, the composition itself, step by step on the handle's
    // stream -- policy kernel, merge kernel, the existing step path.
    auto policy_then_merge = [&](int s, uint8_t* acts) {
        hipError_t e = ccx::launch_greedy_actions(h->stream, launch_params(h), h->st, h->cell_info, acts, policy);
        if (e != hipSuccess) return fail(CCX_EHIP, "policy kernel launch failed: %s", hipGetErrorString(e));
        if (scripted_slots != all_slots) {
            e = ccx::launch_merge_actions(h->stream, acts, actions + (size_t)s * EN, scripted_slots, h->N, EN);
            if (e != hipSuccess) return fail(CCX_EHIP, "merge kernel launch failed: %s", hipGetErrorString(e));
        }
        return (int)CCX_OK;
    };
    return finish_call(h, num_steps, c.out, auto_reset, run_stepwise(h, c, "the unfused mixed-control step", policy_then_merge));
}

int ccx_action_masks(ccx_handle* h, uint8_t* masks) {
    if (!h || !masks) return fail(CCX_EINVAL, "NULL argument");
    CCX_HIP(hipSetDevice(h->device));
    hipError_t e = ccx::launch_action_masks(h->stream, launch_params(h), h->st, h->cell_info, masks);
    if (e != hipSuccess) return fail(CCX_EHIP, "action mask kernel launch failed: %s", hipGetErrorString(e));
    return CCX_OK;
}

namespace {
// ccx_get_masks_fused, ccx_get_reset_obs_fused: the plan of the first launch of such a call from an action tensor, with masks
// bound and restarted rows to write
ccxp::LaunchPlan query_plan(const ccx_handle* h, int num_steps, int has_order, int mixed) {
    StepCall c;
    c.K = num_steps;
    c.mixed = mixed != 0;
    ccxp::CallIn in = call_in(h, c);
    in.actions = 1; in.order = has_order != 0; in.masks_bound = 1; in.reset_obs_on = 1;
    const ccxp::CallFacts f = call_facts(h);
    return ccxp::plan_launch(f, in, std::min(num_steps, ccxp::plan_call(f, in).steps_per_launch));
}
}  // namespace

int ccx_bind_action_masks(ccx_handle* h, uint8_t* masks_or_null) {
    if (!h) return fail(CCX_EINVAL, "NULL handle");
    h->bound_masks = masks_or_null;
    return CCX_OK;
}

int ccx_get_masks_fused(ccx_handle* h, int32_t num_steps, int32_t has_order, int32_t mixed, int32_t* fused) {
    if (!h || !fused) return fail(CCX_EINVAL, "NULL argument");
    if (num_steps < 1) return fail(CCX_EINVAL, "num_steps must be >= 1");
    *fused = query_plan(h, num_steps, has_order, mixed).masks_fused ? 1 : 0;
    return CCX_OK;
}

int ccx_set_reset_obs(ccx_handle* h, int32_t mode) {
    if (!h) return fail(CCX_EINVAL, "NULL handle");
    if (mode != CCX_RESET_OBS_TERMINAL && mode != CCX_RESET_OBS_NEXT)
        return fail(CCX_EINVAL, "unknown reset-observation mode %d (CCX_RESET_OBS_TERMINAL, CCX_RESET_OBS_NEXT)", mode);
    h->reset_obs = mode;
    return CCX_OK;
}

int ccx_bind_final_obs(ccx_handle* h, float* final_obs_or_null, float* final_compact_or_null) {
    if (!h) return fail(CCX_EINVAL, "NULL handle");
    h->bound_final_obs = final_obs_or_null;
    h->bound_final_compact = final_compact_or_null;
    return CCX_OK;
}

int ccx_get_reset_obs_fused(ccx_handle* h, int32_t num_steps, int32_t has_order, int32_t mixed, int32_t* fused) {
    if (!h || !fused) return fail(CCX_EINVAL, "NULL argument");
    if (num_steps < 1) return fail(CCX_EINVAL, "num_steps must be >= 1");
    *fused = query_plan(h, num_steps, has_order, mixed).reset_obs_fused ? 1 : 0;
    return CCX_OK;
}

namespace {
// CCX_CHECK_INPUTS: after a stream sync, turn what check_inputs_kernel counted into CCX_EINVAL (once)
int report_input_errors(ccx_handle* h) {
    if (!h->check_inputs) return CCX_OK;
    unsigned long long bad[2] = {0, 0};
    CCX_HIP(hipMemcpy(bad, h->input_errors, sizeof(bad), hipMemcpyDeviceToHost));
    if (!bad[0] && !bad[1]) return CCX_OK;
    CCX_HIP(hipMemset(h->input_errors, 0, sizeof(bad)));
    return fail(CCX_EINVAL, "invalid inputs since the last check: Invalid action: %llu action byte(s) outside "
                "{0,1,2,3,4} and not CCX_ACTION_ABSENT; Unknown agent ID / duplicate: %llu move-order row(s) that are "
                "not a permutation of 0..N-1 (collectivecrossing.py:685-711); such entries were stepped as "
                "'no move' / an undefined order", bad[0], bad[1]);
}
}  // namespace

int ccx_set_reward_table(ccx_handle* h, const double* boarding_per_cell, const double* exiting_per_cell) {
    if (!h) return fail(CCX_EINVAL, "NULL handle");
    if ((boarding_per_cell == nullptr) != (exiting_per_cell == nullptr))
        return fail(CCX_EINVAL, "give a table for both agent types, or NULL for both (back to the built-in reward)");
    CCX_HIP(hipSetDevice(h->device));
    CCX_HIP(hipStreamSynchronize(h->stream));               // (launches in flight still read the old table)
    if (!boarding_per_cell) {
        (void)hipFree(h->reward_table);
        h->reward_table = nullptr;
        return choose_shape(h);
    }
    const int W1 = h->params.width + 1, H1 = h->params.height + 1, Wp = h->params.width + 3, Hp = h->params.height + 3;
    const size_t cells = (size_t)Wp * (size_t)Hp;
    if (!ccxp::reward_table_fits(plan_in_of(h, true))) {    // (asked before anything is uploaded; a table set earlier goes)
        (void)hipFree(h->reward_table);
        h->reward_table = nullptr;
        (void)choose_shape(h);
        return fail(CCX_EINVAL, "the reward table of a %d x %d grid (%zu bytes of LDS) does not fit next to the kernel's tables",
                    h->params.width, h->params.height, cells * 16u);
    }
    std::vector<double> tab(2u * cells, 0.0);                // padded grid, border cells 0 (never occupied)
    const double* src[2] = {boarding_per_cell, exiting_per_cell};
    for (int t = 0; t < 2; ++t)
        for (int y = 0; y < H1; ++y)
            for (int x = 0; x < W1; ++x)
                tab[(size_t)t * cells + (size_t)ccx::cell_index(x, y, Wp)] = src[t][(size_t)y * W1 + x];
    if (!h->reward_table) CCX_HIP(hipMalloc(&h->reward_table, tab.size() * sizeof(double)));
    CCX_HIP(hipMemcpy(h->reward_table, tab.data(), tab.size() * sizeof(double), hipMemcpyHostToDevice));
    return choose_shape(h);
}

int ccx_set_terminated_table(ccx_handle* h, const uint8_t* boarding_per_cell, const uint8_t* exiting_per_cell) {
    if (!h) return fail(CCX_EINVAL, "NULL handle");
    if ((boarding_per_cell == nullptr) != (exiting_per_cell == nullptr))
        return fail(CCX_EINVAL, "give a table for both agent types, or NULL for both (back to the built-in strategy)");
    if (boarding_per_cell && h->params.terminated_mode != CCX_TERM_INDIVIDUAL_AT_DESTINATION)
        return fail(CCX_EINVAL, "a terminated table replaces individual_at_destination (terminated_mode 0): per agent, from its own cell");
    const size_t n = (size_t)(h->params.width + 1) * (size_t)(h->params.height + 1);
    const uint8_t* src[2] = {boarding_per_cell, exiting_per_cell};
    for (int t = 0; t < 2; ++t) {
        h->term_table[t].clear();
        if (src[t]) h->term_table[t].assign(src[t], src[t] + n);
    }
    CCX_HIP(hipSetDevice(h->device));
    CCX_HIP(hipStreamSynchronize(h->stream));
    const std::vector<unsigned long long> cell_tab = build_cell_table(h->params, h->term_table);
    CCX_HIP(hipMemcpy(h->cell_info, cell_tab.data(), cell_tab.size() * sizeof(unsigned long long), hipMemcpyHostToDevice));
    return choose_shape(h);        // (KParams::user_tables)
}

int ccx_set_check_inputs(ccx_handle* h, int32_t enabled) {
    if (!h) return fail(CCX_EINVAL, "NULL handle");
    h->check_inputs = enabled != 0;
    return CCX_OK;
}

int ccx_check_inputs(ccx_handle* h) {
    if (!h) return fail(CCX_EINVAL, "NULL handle");
    CCX_HIP(hipSetDevice(h->device));
    CCX_HIP(hipStreamSynchronize(h->stream));
    return report_input_errors(h);
}

int ccx_set_rng_seed(ccx_handle* h, uint64_t seed) {
    if (!h) return fail(CCX_EINVAL, "NULL handle");
    h->rng_lo = (uint32_t)seed;
    h->rng_hi = (uint32_t)(seed >> 32);
    return CCX_OK;
}

int ccx_set_policy_epsilon(ccx_handle* h, double epsilon) {
    if (!h) return fail(CCX_EINVAL, "NULL handle");
    if (!(epsilon >= 0.0 && epsilon <= 1.0)) return fail(CCX_EINVAL, "epsilon must be in [0, 1] (got %g)", epsilon);
    const double t = epsilon * 4294967296.0;
    h->eps_thr = t >= 4294967295.0 ? 0xFFFFFFFFu : (uint32_t)t;
    h->epsilon = epsilon;
    return CCX_OK;
}

int ccx_set_policy_stream(ccx_handle* h, int32_t kind, const uint32_t* seeds, uint32_t seed) {
    if (!h) return fail(CCX_EINVAL, "NULL handle");
    if (kind != CCX_EPS_STREAM_COUNTER && kind != CCX_EPS_STREAM_MT19937)
        return fail(CCX_EINVAL, "unknown epsilon stream %d", kind);
    if (kind == CCX_EPS_STREAM_MT19937) {
        if (h->N > 64) return fail(CCX_EINVAL, "the MT19937 stream walks an env's agents with one 64-lane wave: <= 64 agents");
        CCX_HIP(hipSetDevice(h->device));
        if (!h->mt_state) CCX_HIP(hipMalloc(&h->mt_state, (size_t)h->E * ccx::kMtStateWords * sizeof(uint32_t)));
        uint32_t* seeds_dev = nullptr;
        if (seeds) {   // (host array: a handful of words per env, staged through the placement scratch's neighbour)
            CCX_HIP(hipMalloc(&seeds_dev, (size_t)h->E * sizeof(uint32_t)));
            hipError_t ce = hipMemcpyAsync(seeds_dev, seeds, (size_t)h->E * sizeof(uint32_t), hipMemcpyHostToDevice, h->stream);
            if (ce != hipSuccess) {
                (void)hipFree(seeds_dev);
                return fail(CCX_EHIP, "seed upload failed: %s", hipGetErrorString(ce));
            }
        }
        hipError_t e = ccx::launch_policy_stream_seed(h->stream, h->mt_state, seeds_dev, seed, h->E);
        hipError_t se = hipStreamSynchronize(h->stream);      // (the seeds array may be freed by the caller on return)
        if (seeds_dev) (void)hipFree(seeds_dev);
        if (e != hipSuccess || se != hipSuccess) {
            // (a half-seeded generator array must not be handed out by ccx_get_policy_stream or walked by a policy kernel)
            (void)hipFree(h->mt_state);
            h->mt_state = nullptr;
            h->eps_stream = CCX_EPS_STREAM_COUNTER;
            return fail(CCX_EHIP, "stream seeding failed: %s", hipGetErrorString(e != hipSuccess ? e : se));
        }
    }
    h->eps_stream = kind;
    return CCX_OK;
}

int ccx_get_policy_stream(ccx_handle* h, int32_t* kind, uint32_t* state) {
    if (!h) return fail(CCX_EINVAL, "NULL handle");
    if (kind) *kind = h->eps_stream;
    if (state) {
        if (!h->mt_state) return fail(CCX_EINVAL, "no MT19937 stream has been seeded on this handle (ccx_set_policy_stream)");
        CCX_HIP(hipSetDevice(h->device));
        CCX_HIP(hipStreamSynchronize(h->stream));
        CCX_HIP(hipMemcpy(state, h->mt_state, (size_t)h->E * ccx::kMtStateWords * sizeof(uint32_t), hipMemcpyDeviceToHost));
    }
    return CCX_OK;
}

int ccx_zero_counters(ccx_handle* h) {
    if (!h) return fail(CCX_EINVAL, "NULL handle");
    CCX_HIP(hipSetDevice(h->device));
    CCX_HIP(hipMemsetAsync(h->counters, 0, ccx::counter_words(h->E) * sizeof(unsigned long long), h->stream));
    return CCX_OK;
}

int ccx_read_counters(ccx_handle* h, ccx_counters* out_host) {
    if (!h || !out_host) return fail(CCX_EINVAL, "NULL argument");
    static_assert(sizeof(ccx_counters) == 6 * sizeof(unsigned long long), "counter layout");
    CCX_HIP(hipSetDevice(h->device));
    CCX_HIP(ccx::launch_reduce_counters(h->stream, h->counters, h->E));
    CCX_HIP(hipStreamSynchronize(h->stream));
    CCX_HIP(hipMemcpy(out_host, h->counters, sizeof(ccx_counters), hipMemcpyDeviceToHost));
    return report_input_errors(h);
}

int ccx_counters_device_ptr(ccx_handle* h, uint64_t** out) {
    if (!h || !out) return fail(CCX_EINVAL, "NULL argument");
    CCX_HIP(hipSetDevice(h->device));
    CCX_HIP(ccx::launch_reduce_counters(h->stream, h->counters, h->E));
    *out = reinterpret_cast<uint64_t*>(h->counters);
    return CCX_OK;
}

int ccx_set_timing(ccx_handle* h, int32_t enabled) {
    if (!h) return fail(CCX_EINVAL, "NULL handle");
    h->timing = enabled != 0;
    if (!h->timing) h->timed = false;
    return CCX_OK;
}

int ccx_last_launch_ms(ccx_handle* h, float* ms) {
    if (!h || !ms) return fail(CCX_EINVAL, "NULL argument");
    if (!h->timed) return fail(CCX_EINVAL, "no timed launch yet (enable with ccx_set_timing(h, 1))");
    CCX_HIP(hipSetDevice(h->device));
    CCX_HIP(hipEventSynchronize(h->ev_stop));
    CCX_HIP(hipEventElapsedTime(ms, h->ev_start, h->ev_stop));
    return CCX_OK;
}

int ccx_set_launch_shape(ccx_handle* h, int32_t lanes_per_wave, int32_t waves_per_block) {
    if (!h) return fail(CCX_EINVAL, "NULL handle");
    const int G = 1 << ceil_log2(h->N);
    if (lanes_per_wave != 0 && (lanes_per_wave < G || lanes_per_wave > 64 || lanes_per_wave % G))
        return fail(CCX_EINVAL, "lanes_per_wave %d must be a multiple of the env lane group %d and <= 64",
                    lanes_per_wave, G);
    if (waves_per_block < 0 || waves_per_block > 4) return fail(CCX_EINVAL, "waves_per_block must be 0..4");
    h->lanes_per_wave = lanes_per_wave;
    h->waves_per_block = waves_per_block;
    return choose_shape(h);
}

int ccx_set_writers(ccx_handle* h, int32_t writers_per_tile) {
    if (!h) return fail(CCX_EINVAL, "NULL handle");
    if (writers_per_tile < 0 || writers_per_tile > 7) return fail(CCX_EINVAL, "writers_per_tile must be 0..7");
    h->writers = writers_per_tile;
    return choose_shape(h);
}

int ccx_set_store_throttle(ccx_handle* h, int32_t max_stores_in_flight) {
    if (!h) return fail(CCX_EINVAL, "NULL handle");
    if (max_stores_in_flight < -1 || max_stores_in_flight > 63)
        return fail(CCX_EINVAL, "max_stores_in_flight must be -1 (off), 0 (default) or 1..63");
    h->store_throttle = max_stores_in_flight;
    return choose_shape(h);
}

int ccx_set_step_pace(ccx_handle* h, int32_t ns_per_env_step) {
    if (!h) return fail(CCX_EINVAL, "NULL handle");
    if (ns_per_env_step < -1) return fail(CCX_EINVAL, "ns_per_env_step must be -1 (off), 0 (adaptive) or > 0");
    h->step_pace_ns = ns_per_env_step;
    return choose_shape(h);
}

int ccx_set_step_pace_start(ccx_handle* h, float ns_per_env_step) {
    if (!h) return fail(CCX_EINVAL, "NULL handle");
    if (!(ns_per_env_step >= 0.0f) || ns_per_env_step > 1.0e7f)
        return fail(CCX_EINVAL, "ns_per_env_step must be 0 (library default) or a positive number of nanoseconds");
    h->pace_start_ns = ns_per_env_step;
    return choose_shape(h);
}

int ccx_set_pace_calibration(ccx_handle* h, int32_t enabled) {
    if (!h) return fail(CCX_EINVAL, "NULL handle");
    h->pace_calibrate = enabled != 0;
    return choose_shape(h);
}

int ccx_get_pace_start(ccx_handle* h, float* ns_per_env_step, int32_t* source, float* probe_gbs) {
    if (!h) return fail(CCX_EINVAL, "NULL handle");
    if (ns_per_env_step) *ns_per_env_step = h->kp.pace_state ? ccxp::fp_to_ns(h->pace.init_fp) : 0.0f;
    if (source) *source = h->kp.pace_state ? h->pace.start_source : CCX_PACE_START_UNPACED;
    if (probe_gbs) *probe_gbs = h->pace.probe_gbs;
    return CCX_OK;
}

int ccx_set_tunable(ccx_handle* h, const char* name, int32_t value) {
    if (!h || !name) return fail(CCX_EINVAL, "NULL argument");
    struct { const char* name; int* slot; int lo, hi; } table[] = {
        {"pace_phase", &h->tun_pace_phase, -1, 3},
        {"tile_map", &h->tun_tile_map, -1, 6},
        {"hand2", &h->tun_hand2, 0, 2},
        {"writer_roles", &h->tun_writer_roles, -1, 1},
        {"max_launch_steps", &h->tun_max_launch_steps, 0, 0x7FFFFFFF},
        {"pair_rows", &h->tun_pair_rows, -1, 1},
        {"small_shape", &h->tun_small_shape, 0, 1},
        {"round_launches", &h->tun_round_launches, 0, 2},
        {"occ_tables", &h->tun_occ_tables, -1, 1},
        {"step_kernel", &h->tun_step_kernel, -1, 1},
        {"step_rows", &h->tun_step_rows, 0, 7},
        {"step_lanes", &h->tun_step_lanes, 0, 64},
        {"stats_naive", &h->tun_stats_naive, 0, 1},
        {"reset_obs_fused", &h->tun_reset_obs_fused, 0, 1},
    };
    for (auto& t : table)
        if (strcmp(name, t.name) == 0) {
            if (value < t.lo || value > t.hi)
                return fail(CCX_EINVAL, "tunable %s must be %d..%d (got %d)", name, t.lo, t.hi, value);
            *t.slot = value;
            return choose_shape(h);
        }
    std::string names;
    for (auto& t : table) names.append(names.empty() ? "" : ", ").append(t.name);
    return fail(CCX_EINVAL, "unknown tunable '%s' (%s)", name, names.c_str());
}

int ccx_get_step_pace(ccx_handle* h, float* ns_per_env_step) {
    if (!h || !ns_per_env_step) return fail(CCX_EINVAL, "NULL argument");
    CCX_HIP(hipSetDevice(h->device));
    uint32_t fp = h->pace.init_fp;
    if (!h->kp.pace_state) {   // off, or adaptive on a batch too small to be memory-bound
        fp = 0;
    } else if (!h->pace.dirty) {
        CCX_HIP(hipStreamSynchronize(h->stream));
        uint32_t st[4];
        CCX_HIP(hipMemcpy(st, h->pace.state, sizeof(st), hipMemcpyDeviceToHost));
        fp = st[h->pace.slot] > st[2] ? st[h->pace.slot] : st[2];
    }
    *ns_per_env_step = ccxp::fp_to_ns(fp);
    return CCX_OK;
}

int ccx_get_pace_state(ccx_handle* h, float* out6) {
    if (!h || !out6) return fail(CCX_EINVAL, "NULL argument");
    CCX_HIP(hipSetDevice(h->device));
    CCX_HIP(hipStreamSynchronize(h->stream));
    uint32_t st[8];
    CCX_HIP(hipMemcpy(st, h->pace.state, sizeof(st), hipMemcpyDeviceToHost));
    const auto ns = ccxp::fp_to_ns;
    const bool dirty = h->pace.dirty;
    out6[0] = dirty ? ns(h->pace.init_fp) : ns(st[h->pace.slot]);   // the vote the next launch reads
    out6[1] = dirty ? 0.0f : ns(st[2]);                             // floor
    out6[2] = dirty ? 0.0f : (float)st[3];                          // launches since the last collapse
    out6[3] = h->kp.pace_state ? 1.0f : 0.0f;
    out6[4] = dirty ? 0.0f : ns(st[4]);                             // pace of the last collapse (the cliff)
    out6[5] = dirty ? 0.0f : (float)st[5];                          // confirmations of that cliff
    return CCX_OK;
}

int ccx_get_residency(ccx_handle* h, int32_t* resident_workgroups, int32_t* workgroups) {
    if (!h) return fail(CCX_EINVAL, "NULL handle");
    if (resident_workgroups) *resident_workgroups = h->shape.resident_blocks;
    if (workgroups) *workgroups = h->shape.num_blocks;
    return CCX_OK;
}

int ccx_get_launch_shape(ccx_handle* h, int32_t* lanes_per_wave, int32_t* waves_per_block,
                         int32_t* group_lanes, int32_t* num_blocks) {
    if (!h) return fail(CCX_EINVAL, "NULL handle");
    if (lanes_per_wave) *lanes_per_wave = h->shape.envs_per_wave << h->shape.glog;
    if (waves_per_block) *waves_per_block = h->shape.waves_per_block;
    if (group_lanes) *group_lanes = 1 << h->shape.glog;
    if (num_blocks) *num_blocks = h->shape.num_blocks;
    return CCX_OK;
}

int ccx_get_step_shape(ccx_handle* h, int32_t* ok, int32_t* lanes_per_wave, int32_t* row_waves,
                       int32_t* num_blocks, int32_t* lds_bytes) {
    if (!h) return fail(CCX_EINVAL, "NULL handle");
    const ccx::StepShape& ss = h->step_shape;
    if (ok) *ok = (ss.ok && h->tun_step_kernel != 0) ? 1 : 0;
    if (lanes_per_wave) *lanes_per_wave = ss.envs_per_wave << ss.glog;
    if (row_waves) *row_waves = ss.row_waves;
    if (num_blocks) *num_blocks = ss.num_blocks;
    if (lds_bytes) *lds_bytes = (int32_t)ss.lds_bytes;
    return CCX_OK;
}

int ccx_get_writer_shape(ccx_handle* h, int32_t* writers_per_tile, int32_t* max_stores_in_flight) {
    if (!h) return fail(CCX_EINVAL, "NULL handle");
    if (writers_per_tile) *writers_per_tile = h->shape.writers;
    if (max_stores_in_flight) *max_stores_in_flight = h->shape.store_throttle;
    return CCX_OK;
}

int ccx_host_device_pointer(ccx_handle* h, void* pinned_host, void** device_ptr) {
    if (!h || !pinned_host || !device_ptr) return fail(CCX_EINVAL, "NULL argument");
    CCX_HIP(hipSetDevice(h->device));
    hipPointerAttribute_t attr{};
    hipError_t e = hipPointerGetAttributes(&attr, pinned_host);
    if (e != hipSuccess || attr.type != hipMemoryTypeHost) {
        (void)hipGetLastError();
        return fail(CCX_EINVAL, "pointer is not page-locked host memory registered with HIP");
    }
    void* d = nullptr;
    CCX_HIP(hipHostGetDevicePointer(&d, pinned_host, 0));
    *device_ptr = d;
    return CCX_OK;
}

int ccx_set_stream(ccx_handle* h, void* stream) {
    if (!h) return fail(CCX_EINVAL, "NULL handle");
    CCX_HIP(hipSetDevice(h->device));
    CCX_HIP(hipStreamSynchronize(h->stream));   // work queued on the old stream finishes first
    h->stream = reinterpret_cast<hipStream_t>(stream);
    return CCX_OK;
}

int ccx_synchronize(ccx_handle* h) {
    if (!h) return fail(CCX_EINVAL, "NULL handle");
    CCX_HIP(hipSetDevice(h->device));
    CCX_HIP(hipStreamSynchronize(h->stream));
    return report_input_errors(h);
}

// ---- internal (ccx_plan.h): what a live handle launches with, for the tests of the launch-shape planner ---------------
int ccxi_handle_plan(const ccx_handle* h, int rows, ccxi_plan_out* out, int* blocks_per_cu) {
    if (!h || !out) return fail(CCX_EINVAL, "NULL argument");
    const ccx::LaunchShape& s = rows ? h->shape : h->shape_small;
    const ccx::KParams& k = rows ? h->kp : h->kp_small;
    ccxp::PacePlan pp{};
    pp.paced = k.pace_state != nullptr;
    if (rows) {
        pp.ring_when_paced = h->ring_when_paced;
        pp.pace_init_fp = h->pace.init_fp;
        pp.pace_start_source = h->pace.start_source;
    }
    ccxp::plan_out(s, k, rows ? h->step_shape : ccx::StepShape{}, pp, out);
    if (blocks_per_cu) *blocks_per_cu = ccx::rollout_blocks_per_cu(s, h->N);   // (the query choose_shape made for this shape)
    return CCX_OK;
}

int ccxi_handle_call_plan(const ccx_handle* h, const ccxi_call_in* call, int launch, ccxi_call_out* out) {
    if (!h || !call || !out) return fail(CCX_EINVAL, "NULL argument");
    ccxp::CallIn in = *call;
    in.hand2 = h->tun_hand2; in.round_launches = h->tun_round_launches; in.small_shape = h->tun_small_shape;
    in.step_kernel = h->tun_step_kernel; in.max_launch_steps = h->tun_max_launch_steps; in.reset_obs_fused = h->tun_reset_obs_fused;
    if (ccxp::plan_call_out(call_facts(h), in, launch, out) != CCX_OK)
        return fail(CCX_EINVAL, "K = %d has no launch number %d", in.K, launch);
    return CCX_OK;
}

// (ccx_keys.h)
int ccxi_handle_last_key(const ccx_handle* h, int which, ccxi_key* out) {
    if (!h || !out || which < 0 || which > 1) return fail(CCX_EINVAL, "bad argument");
    *out = which ? h->last_observe_key : h->last_key;
    return CCX_OK;
}

#ifdef CCX_LAG_TRACE
int ccx_debug_lag_trace(int* host) {   // diagnostic build only (make variant DEFS=-DCCX_LAG_TRACE): [16][4096] ints of the last launch
    if (!g_lag_buf) return -1;
    return (int)hipMemcpy(host, g_lag_buf, 16 * 4096 * sizeof(int), hipMemcpyDeviceToHost);
}
#endif
}  // extern "C"
