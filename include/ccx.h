/*
 * ccx.h -- C-ABI of libccx, the MI355X (gfx950) batched CollectiveCrossing step library.
 *
 * The reference (nima-siboni/collectivecrossing v0.1.3) has NO FFI: its hot path is the pure
 * Python method CollectiveCrossingEnv.step (src/collectivecrossing/collectivecrossing.py:161-261)
 * plus the strategy objects it calls.  Every entry point below names the reference function(s) it
 * replaces (file:line relative to the reference root); INTEGRATION.md shows the ctypes binding a
 * maintainer of the reference would add.
 *
 * Conventions
 *   - plain C, no torch / HIP types in signatures; device pointers travel as void* / typed pointers.
 *   - every function returns 0 (CCX_OK) or a negative ccx_status; ccx_last_error() returns the
 *     message of the last failure on the calling thread.
 *   - all array arguments are DEVICE pointers unless the name ends in _host.
 *   - array layout is struct-of-arrays, ENV-MAJOR: index [e*N + a] for per-agent arrays ("[E][N]"),
 *     agent slot a in 0..N-1, boarding agents first (a < num_boarding  <=> "boarding_{a}",
 *     otherwise "exiting_{a-num_boarding}"), exactly the reference's dict insertion order
 *     (collectivecrossing.py:101-150).
 *   - a handle is bound to one device and one HIP stream; calls are asynchronous on that stream
 *     unless stated otherwise; a handle is not thread-safe (neither is the reference env).
 */
#ifndef CCX_H
#define CCX_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CCX_ABI_VERSION 5

typedef enum ccx_status {
    CCX_OK = 0,
    CCX_EINVAL = -1,     /* bad argument / unsupported configuration            */
    CCX_ENOMEM = -2,     /* device or host allocation failed                    */
    CCX_EHIP = -3,       /* a HIP runtime call failed (message has the detail)  */
    CCX_ENODEVICE = -4   /* no usable gfx950 device                             */
} ccx_status;

/* reward_configs.py registry names -> enum (rewards.py:186-191) */
enum { CCX_REWARD_DEFAULT = 0, CCX_REWARD_SIMPLE_DISTANCE = 1, CCX_REWARD_BINARY = 2,
       CCX_REWARD_CONSTANT_NEGATIVE = 3 };
/* terminateds.py:86-89 */
enum { CCX_TERM_INDIVIDUAL_AT_DESTINATION = 0, CCX_TERM_ALL_AT_DESTINATION = 1 };
/* truncateds.py:99-102 ("custom" has the same arithmetic as "max_steps", truncateds.py:64-95) */
enum { CCX_TRUNC_MAX_STEPS = 0 };

/* scripted policies evaluated on the device (src/baseline_policies/) */
enum { CCX_POLICY_GREEDY = 1, CCX_POLICY_WAITING = 2, CCX_POLICY_RANDOM = 3 };

/* action codes, actions.py:8-24; CCX_ACTION_ABSENT = agent not in action_dict (it does not move,
 * collectivecrossing.py:197-202 only iterates over the dict's items) */
enum { CCX_ACTION_RIGHT = 0, CCX_ACTION_UP = 1, CCX_ACTION_LEFT = 2, CCX_ACTION_DOWN = 3,
       CCX_ACTION_WAIT = 4, CCX_ACTION_ABSENT = 255 };

/*
 * Lowered, POD form of CollectiveCrossingConfig (configs.py:15-77) + the four strategy configs.
 * Geometry is ABSOLUTE (already passed through utils/geometry.py:34-40):
 *   tram_left = width/2 - tram_length/2, tram_right = width/2 + tram_length/2,
 *   door_left/right = tram_left + cfg.tram_door_left/right.
 */
typedef struct ccx_params {
    int32_t width, height, division_y;
    int32_t tram_left, tram_right, door_left, door_right;
    int32_t num_boarding, num_exiting;
    int32_t boarding_dest_y, exiting_dest_y;
    int32_t reward_mode, terminated_mode, truncated_mode;
    int32_t max_steps;
    int32_t _pad0;
    /* DefaultRewardConfig (reward_configs.py:24-57); distance_penalty_factor is shared with
     * SimpleDistanceRewardConfig (reward_configs.py:60-77) */
    double boarding_destination_reward, tram_door_reward, tram_area_reward, distance_penalty_factor;
    /* BinaryRewardConfig (reward_configs.py:80-101), ConstantNegativeRewardConfig (:104-121) */
    double goal_reward, no_goal_reward, step_penalty;
} ccx_params;

typedef struct ccx_handle ccx_handle;

/* per-agent result byte of one step ("agent_flags", u8 [E][N]) */
#define CCX_AF_TERMINATED   0x01u /* terminateds[id] (always present, terminateds.py:40-82)             */
#define CCX_AF_TRUNCATED    0x02u /* truncateds[id]; meaningful only with CCX_AF_LIVE (truncateds.py:56)  */
#define CCX_AF_LIVE         0x04u /* agent was neither terminated nor truncated BEFORE this step:         */
                                  /*   rewards[id] and truncateds[id] exist (rewards.py:64, truncateds.py:56) */
#define CCX_AF_OBS          0x08u /* observations[id]/infos[id] emitted (collectivecrossing.py:243-254)   */
#define CCX_AF_IN_TRAM_AREA 0x10u /* infos[id]["in_tram_area"]   (collectivecrossing.py:551-554)          */
#define CCX_AF_AT_DOOR      0x20u /* infos[id]["at_door"]        (collectivecrossing.py:556-563)          */
#define CCX_AF_ACTIVE       0x40u /* infos[id]["active"]                                                  */
#define CCX_AF_AT_DEST      0x80u /* infos[id]["at_destination"] (collectivecrossing.py:663-683)          */

/* per-env result byte of one step ("env_flags", u8 [E]) */
#define CCX_EF_ALL_TERMINATED 0x01u /* terminateds["__all__"] (collectivecrossing.py:256,258) */
#define CCX_EF_ALL_TRUNCATED  0x02u /* truncateds["__all__"]  (collectivecrossing.py:257,259) */
#define CCX_EF_RESET          0x04u /* rollout only: the env was auto-reset after this step    */

/* SoA state of the batch: the Agent dataclass (types.py:16-83) + env._step_count. */
typedef struct ccx_state {
    int32_t* x;           /* [E][N] */
    int32_t* y;           /* [E][N] */
    uint8_t* active;      /* [E][N] Agent.active      */
    uint8_t* terminated;  /* [E][N] Agent.terminated  */
    uint8_t* truncated;   /* [E][N] Agent.truncated   */
    int32_t* step_count;  /* [E]    env._step_count   */
    int32_t* episode;     /* [E]    number of auto-resets so far (selects the reset-pool entry) */
} ccx_state;

/* outputs of one step for the whole batch; any pointer may be NULL to skip that output */
typedef struct ccx_step_out {
    float*   obs;          /* [E][N][L], L = 6 + 4N, DefaultObservation (observations.py:43-94) */
    double*  reward;       /* [E][N] f64, meaningful where CCX_AF_LIVE (rewards.py:44-182)      */
    uint8_t* agent_flags;  /* [E][N] CCX_AF_*                                                   */
    uint8_t* env_flags;    /* [E]    CCX_EF_*                                                   */
    float*   obs_compact;  /* [E][N][4] CCX_OBS_COMPACT, see below                                 */
} ccx_step_out;

/* trajectory outputs of a K-step rollout; step s of env e lives at [s][e]...; NULL skips */
typedef struct ccx_rollout_out {
    float*   obs;          /* [K][E][N][L] */
    double*  reward;       /* [K][E][N]    */
    uint8_t* agent_flags;  /* [K][E][N]    */
    uint8_t* env_flags;    /* [K][E]       */
    float*   obs_compact;  /* [K][E][N][4] */
} ccx_rollout_out;

/*
 * CCX_OBS_COMPACT -- an OPTIONAL second observation output for consumers that live on the GPU (next to,
 * never instead of, the DefaultObservation layout).  A DefaultObservation row (observations.py:79-92) is six
 * per-row numbers plus, for EVERY agent j of the env, (x_j, y_j, type_j, active_j): the N rows of an env
 * repeat the same 4N numbers N times (152 of the 162 bytes a C2 agent-step writes).  obs_compact holds each
 * agent's four numbers ONCE per env and step: f32 [..][E][N][4] = (x, y, type 0 boarding / 1 exiting,
 * active 0/1), 16 bytes per agent-step instead of 16N + 24.  ccx_expand_observations turns compact rows back
 * into the DefaultObservation rows with the very gather ccx_observe uses, bit for bit (rows = envs, or
 * steps x envs for a trajectory): a policy network can consume the compact tensor directly, or expand just
 * the mini-batch it samples.  The row constants (door centre, division_y, door_left, door_right) are those
 * of the handle.
 */
int ccx_expand_observations(ccx_handle* h, const float* obs_compact /* [rows][N][4] */, int64_t rows,
                            float* obs /* [rows][N][L] */);

/*
 * CCX_RENDER -- rgb_array frames of the board, the picture of the reference's draw_matplotlib (rendering.py) drawn with
 * integer arithmetic (the same geometry, palette, alpha values and layer order; not matplotlib's anti-aliased pixels).
 *   Frame of cell size cp = cell_px (1..64): H*cp rows x W*cp columns, HWC RGB u8, covering the axes [0, W] x [0, H];
 *   row 0 is the top (y = H).  The centre of pixel (r, c) is X = (c + 1/2)/cp, Y = H - (r + 1/2)/cp; in HALF-PIXEL
 *   units u = 2c + 1 = 2cp X and v = 2cp H - 2r - 1 = 2cp Y every test below is exact.
 *   Blend: alpha byte a = round(255 alpha) (0.3 -> 77, 0.5 -> 128, 0.7 -> 179, 0.8 -> 204, 0.9 -> 230);
 *   out = (a src + (255 - a) dst + 127) / 255 per channel, integer division, one layer after another.
 *   A rectangle [x0, x1) x [y0, y1) covers the pixels with 2cp x0 <= u < 2cp x1 and 2cp y0 <= v < 2cp y1.  Layers, in the
 *   reference's draw order:
 *     1. background #f8f9fa;
 *     2. tram area #e3f2fd a 179: [tram_left, tram_right + 1) x [division_y, H);
 *     3. waiting area #fff3e0 a 179: [0, W) x [0, division_y);
 *     4. exit row #f44336 a 204: [0, W) x [exiting_dest_y, +1), only when exiting_dest_y < division_y;
 *     5. seats row #2196f3 a 204: [tram_left, tram_right + 1) x [y_s, +1), y_s = boarding_dest_y, or H - 1 when
 *        boarding_dest_y == H; only when boarding_dest_y >= division_y;
 *     6. walls #424242 a 230, one layer (the union of the pieces, blended once), t = max(1, (cp + 5) / 10) pixels thick
 *        (0.1 cell rounded, never thinner than 1 px).  Snapping: a wall on the line x = k takes the t columns from
 *        cp k - t/2, a wall on the line y = division_y the t rows from cp (H - division_y) - t/2, each run shifted
 *        inside the frame where it would leave it.  Pieces: vertical walls on x = tram_left and x = tram_right + 1 in
 *        the rows above division_y (r < cp (H - division_y)); horizontal wall rows over [tram_left, door_left + 1/2)
 *        when door_left > tram_left and over [door_right - 1/2, tram_right + 1) when door_right < tram_right;
 *     7. door interior #90caf9 a 204: [door_left + 1/2, door_right - 1/2) x [division_y, +1), when
 *        door_right - door_left - 1 > 0;
 *     8. agents, every slot whatever its flags (the reference draws all of env._agents), in slot order (boarding
 *        first): three concentric discs on the GRID POINT (x, y), k = 4, 3, 2 (radius k/10) with a 77, 128, 204, face
 *        #f44336 boarding / #2196f3 exiting.  With dx = u - 2cp x, dy = v - 2cp y the pixel is inside disc k iff
 *        25 (dx^2 + dy^2) <= k^2 cp^2, and takes the edge colour #8b0000 / #00008b (same alpha) iff it is inside and
 *        k cp <= 10 or 25 (dx^2 + dy^2) > (k cp - 10)^2 (a 1-px ring).  Discs are clipped to the frame;
 *     9. grid lines #808080 a 179, only when cp >= 4: columns c with c % cp == 0 or c == W cp - 1, rows r with
 *        r % cp == 0 or r == H cp - 1 (1-px lines at the integer coordinates, the lines x = W / y = 0 on the last
 *        column / row), above the agents (matplotlib's axisbelow = 'line').
 *   Left out: text labels, agent numbers, title, ticks and legend.
 *
 * ccx_render: one frame per row of env_ids (device i32 [rows]; NULL = all E envs, rows == E) from the handle's current
 *   state.  An id outside [0, E) gives a frame of the static layers only (no agents).
 * ccx_render_compact: one frame per compact row (CCX_OBS_COMPACT, f32 [rows][N][4], e.g. a [K][E][N][4] trajectory);
 *   type != 0 draws an exiting agent; an agent whose (x, y) lies outside [0, W] x [0, H] is not drawn, others are
 *   truncated to integers.
 * frames: device u8 [rows][H cp][W cp][3], 16-byte aligned.  Both only launch on the handle's stream (no host sync, no
 * allocation: they capture into a HIP graph after ccx_step).  CCX_EINVAL for tiny frames whose agents do not fit a
 * workgroup's LDS (a few agents per pixel); a larger cell_px renders them.
 */
int ccx_render(ccx_handle* h, const int32_t* env_ids /* [rows] or NULL = all E */, int64_t rows, int cell_px,
               uint8_t* frames /* [rows][H*cell_px][W*cell_px][3] */);
int ccx_render_compact(ccx_handle* h, const float* obs_compact /* [rows][N][4] */, int64_t rows, int cell_px,
                       uint8_t* frames);

/* device-side counters accumulated by ccx_rollout (u64 each; ccx_read_counters copies to host) */
typedef struct ccx_counters {
    uint64_t env_steps;        /* env-steps executed                                      */
    uint64_t agent_steps;      /* env_steps * N (all slots)                               */
    uint64_t live_agent_steps; /* agent-steps of agents with CCX_AF_LIVE                  */
    uint64_t episodes;         /* auto-resets performed                                   */
    uint64_t moves;            /* successful position changes (collectivecrossing.py:408) */
    uint64_t arrivals;         /* deactivations (collectivecrossing.py:210-212)           */
} ccx_counters;


/* library / build info ------------------------------------------------------------------------ */
int         ccx_abi_version(void);
const char* ccx_build_info(void);      /* "libccx <ver> gfx950 hip <ver>" */
const char* ccx_last_error(void);      /* thread-local message of the last failing call */

/* observation length L = 2 + 4 + 4N (observations.py:113-118) */
int32_t ccx_obs_len(int32_t num_agents);

/*
 * Create a batch of num_envs independent environments on `device`, using HIP stream `stream`
 * (a hipStream_t passed as void*; NULL = the device's default stream).  env_offset is the global
 * index of this handle's env 0 and total_envs the global batch size (multi-GPU sharding: the
 * reset-pool entry of env e, episode j depends on env_offset + e, j, total_envs and the pool size only
 * (see ccx_set_reset_pool), so the trajectory of a global env does not depend on how many GPUs the
 * batch is split over).
 * Replaces CollectiveCrossingEnv.__init__ (collectivecrossing.py:44-89) for E instances.
 * All agents start at (0,0), active, step_count 0: call ccx_set_state / ccx_reset_from_pool next.
 */
int ccx_create(const ccx_params* params, int32_t num_envs, int64_t env_offset, int64_t total_envs,
               int device, void* stream, ccx_handle** out);
void ccx_destroy(ccx_handle* h);

int32_t ccx_num_envs(const ccx_handle* h);
int32_t ccx_num_agents(const ccx_handle* h);

/* pointers to the handle's own device-resident SoA state (valid until ccx_destroy) */
int ccx_state_view(ccx_handle* h, ccx_state* out);

/*
 * Overwrite / read back the state (tests reach into env._agents[...] the same way, e.g. the
 * reference's test_collective_crossing.py:139-143).  Host pointers; NULL members are skipped.
 * Synchronous.  set_state validates 0 <= x <= width, 0 <= y <= height (cells that exist,
 * collectivecrossing.py:515) and flags in {0,1}.
 */
int ccx_set_state_host(ccx_handle* h, const ccx_state* src);
int ccx_get_state_host(ccx_handle* h, ccx_state* dst);

/*
 * Reset pool: P seeded initial placements, u8 xy pairs [P][N][2], produced on the host by the
 * reference's rejection-sampling reset (collectivecrossing.py:91-150) for seeds seed0..seed0+P-1.
 * Device pointer; the library keeps the pointer (caller keeps the allocation alive).
 * Cursor: env e (global index g = env_offset + e) starts episode j from entry (g + j * stride) mod P
 * with stride = total_envs mod P, or 1 when P divides total_envs (so that every env still walks
 * through the pool instead of restarting from one placement forever).
 * Supported range: 0 <= env_offset, env_offset + num_envs <= total_envs <= INT64_MAX (g and total_envs are taken
 * as 64-bit integers), P < 2^31, and episode counters 0 <= j <= INT32_MAX (the state keeps j as int32: set
 * episode counters so that no restart takes one past INT32_MAX; beyond it the entry is undefined).
 */
int ccx_set_reset_pool(ccx_handle* h, const uint8_t* pool_xy, int64_t pool_size);

/* (Re)start every env whose mask byte is non-zero (mask NULL = all) from its pool entry for the
 * env's current episode index; clears flags and step_count.  = reset() body :97-150 */
int ccx_reset_from_pool(ccx_handle* h, const uint8_t* env_mask);

/*
 * Seeded placement ON THE DEVICE, bit-identical to reset(seed=s) of the reference INCLUDING its
 * random stream (gymnasium np_random = numpy Generator(PCG64(SeedSequence(s))), rejection sampling
 * of collectivecrossing.py:100-150).  Synchronous; CCX_EINVAL if a placement finds no free cell
 * within 65536 draws per agent (the reference would loop forever).
 *   ccx_fill_reset_pool_seeded: pool_xy[p] = placement of seed seed0 + p, p < pool_size (device
 *     buffer u8 [pool_size][N][2] of the caller; pass it to ccx_set_reset_pool afterwards).
 *   ccx_reset_seeded: env e (mask NULL or mask[e] != 0) restarts from reset(seed=seeds[e]):
 *     positions, active = 1, flags and step_count cleared (seeds: device u64 [E]).
 */
int ccx_fill_reset_pool_seeded(ccx_handle* h, uint8_t* pool_xy, int64_t pool_size, uint64_t seed0);
int ccx_reset_seeded(ccx_handle* h, const uint64_t* seeds, const uint8_t* env_mask);

/*
 * Batched GreedyPolicy with epsilon = 0 (src/baseline_policies/greedy_policy.py:33-449): the action
 * the reference's scripted policy picks for every agent of env.agents from the CURRENT state,
 * actions u8 [E][N]; agents that are terminated or truncated get CCX_ACTION_ABSENT (the rollout loop
 * of scripts/run_greedy_policy_demo.py:67-109 only asks the policy for env.agents).
 */
int ccx_greedy_actions(ccx_handle* h, uint8_t* actions);
/* same for any scripted policy: CCX_POLICY_GREEDY, or CCX_POLICY_WAITING = WaitingPolicy with
 * epsilon = 0 (src/baseline_policies/waiting_policy.py:33-131: boarding agents outside the tram area
 * wait until every exiting agent that is still in env.agents stands on its destination row) */
int ccx_policy_actions(ccx_handle* h, int32_t policy, uint8_t* actions);

/* DefaultObservation of the CURRENT state for every agent (what reset() returns, :153-159). */
int ccx_observe(ccx_handle* h, float* obs /* [E][N][L] */);

/*
 * One step of every env = CollectiveCrossingEnv.step (collectivecrossing.py:161-261):
 *   actions u8 [E][N] (CCX_ACTION_*), order u8 [E][N] or NULL: order[e][k] = slot of the agent
 *   moved k-th (a permutation of 0..N-1; NULL = 0,1,..,N-1 = dict order of possible_agents).
 */
int ccx_step(ccx_handle* h, const uint8_t* actions, const uint8_t* order, const ccx_step_out* out);

/*
 * The SPLIT step: ccx_step cut at the reference's own seam, for callers that evaluate reward / termination / truncation
 * strategies THEMSELVES as batched array code between the halves (collectivecrossing_amd/strategies.py: the array-form
 * plugin interface; the reference accepts any registered class, rewards.py:16-38, terminateds.py:86-114,
 * truncateds.py:64-128).  Both calls only enqueue one kernel on the handle's stream: no host synchronisation, no
 * allocation, and they capture into a HIP graph.  They serve every config ccx_create accepts (no LDS tables).
 *
 * ccx_step_begin = collectivecrossing.py:188-212: step_count += 1, the ordered move resolution with exactly the semantics
 *   of ccx_step (same actions / order contract, CCX_ACTION_ABSENT, ccx_set_check_inputs counting), deactivation on
 *   arrival.  Writes x, y, active, step_count of the state; touches no flag and no output.  A move-order row that is not a
 *   permutation is invalid input, but its effect is defined here and confined to its own env: an order byte >= N names
 *   no agent and moves nothing, a slot named twice moves at most once (named again after it was blocked it tries again).
 *   That rule is ccx_step_begin's alone: for such a row ccx_step and ccx_rollout step an undefined order (see
 *   ccx_set_check_inputs, which counts the row on every path), so begin + finish and ccx_step agree for valid rows only.
 * ccx_step_finish = :214-259 on the state begin left.
 *   reward      device f64 [E][N] or NULL;  terminated  device i8 [E][N]: 1 / 0 / -1 (-1 = the strategy returned None:
 *   no dict entry) or NULL;  truncated  device u8 [E][N] or NULL.  NULL = the handle's built-in rule (including installed
 *   position-only tables), computed in the kernel.
 *   LIVE = not terminated and not truncated BEFORE the step (the state's flags, which begin does not touch).  Reward and
 *   truncation entries exist exactly for LIVE agents (the convention of every built-in class); values at other agents
 *   are ignored.  Termination entries exist where the value is not -1.
 *   Effects, in the reference's order: terminated |= (t == 1); truncated |= (LIVE and u != 0); CCX_AF_TERMINATED /
 *   CCX_AF_TRUNCATED = those two values of this step; CCX_AF_OBS for agents not done, or done in this step; the other
 *   flag bits as ccx_step defines them; CCX_EF_ALL_TERMINATED = every termination entry that exists is true and at least
 *   one exists; CCX_EF_ALL_TRUNCATED likewise over the LIVE agents; out->reward = the caller's value where LIVE, +0.0
 *   elsewhere; obs / obs_compact rows as ccx_step writes them; env_steps, agent_steps and live_agent_steps count the step
 *   (moves and arrivals were counted by begin).
 *   out: as for ccx_step (NULL members are skipped); obs must be 16-byte aligned, 8-byte for an odd number of agents.  term_present (device u8 [E][N], may be NULL) receives 1 where a
 *   termination entry exists.
 *   auto_reset != 0: an env whose step raised either __all__ flag restarts from the reset pool after its outputs are
 *   written: CCX_EF_RESET, episode += 1, the cursor of ccx_set_reset_pool -- what ccx_rollout does.
 * ccx_step_begin + ccx_step_finish(NULL, NULL, NULL) leaves the state and writes the bytes ccx_step does.
 */
int ccx_step_begin(ccx_handle* h, const uint8_t* actions, const uint8_t* order);
int ccx_step_finish(ccx_handle* h, const double* reward, const int8_t* terminated, const uint8_t* truncated,
                    const ccx_step_out* out, uint8_t* term_present, int32_t auto_reset);

/*
 * K fused steps in one launch (state stays in registers between steps).
 *   actions u8 [K][E][N]; order u8 [K][E][N] or NULL.
 *   auto_reset != 0: an env whose step raised terminateds["__all__"] or truncateds["__all__"] is
 *   restarted from the reset pool before its next step (the rollout loop
 *   `if done: env.reset(seed=...)` of the reference's demos, scripts/run_greedy_policy_demo.py:67-109).
 *   out may be NULL (no trajectory); counters are accumulated into the handle.
 */
int ccx_rollout(ccx_handle* h, int32_t num_steps, const uint8_t* actions, const uint8_t* order,
                int32_t auto_reset, const ccx_rollout_out* out);

/*
 * K fused steps with the actions chosen ON THE DEVICE by a scripted policy from the pre-step state
 * (policy -> step -> policy ..., the loop of scripts/run_greedy_policy_demo.py:67-109 inside one
 * launch).  CCX_POLICY_GREEDY = GreedyPolicy with epsilon = 0 (greedy_policy.py:33-449); move order
 * is slot order (env.agents order).  actions_out (u8 [K][E][N], may be NULL) receives the chosen
 * actions, CCX_ACTION_ABSENT for agents outside env.agents.
 */
int ccx_rollout_policy(ccx_handle* h, int32_t num_steps, int32_t policy, int32_t auto_reset,
                       const ccx_rollout_out* out, uint8_t* actions_out);
/*
 * MIXED CONTROL: K steps in which the agent slots of a mask are driven by a scripted policy and the others by the caller's
 * tensor -- training one side against a scripted other side.  The reference serves that per agent
 * (policy.get_action(agent_id, obs, env), greedy_policy.py / waiting_policy.py; the loop of
 * scripts/run_greedy_policy_demo.py:67-109 with a network answering for some ids); here it is ONE launch per <= 16 steps.
 *   policy          CCX_POLICY_GREEDY or CCX_POLICY_WAITING
 *   scripted_slots  bit a = agent slot a (boarding slots first), the same for every env of the handle; a bit at or
 *                   above N is CCX_EINVAL
 *   actions         u8 [K][E][N]; bytes in scripted slots are ignored (and not counted by ccx_set_check_inputs); may be
 *                   NULL when scripted_slots covers all N slots
 *   order           u8 [K][E][N] or NULL, as for ccx_step
 *   actions_out     u8 [K][E][N] or NULL: receives the merged actions
 * Every step is, bit for bit, this composition of existing calls:
 *     pa      = ccx_policy_actions(h, policy)        from the pre-step state; honours ccx_set_policy_epsilon
 *     merged  = scripted_slots has bit a ? pa[e][a] : actions[e][a]
 *     ccx_step(h, merged, order, out)                (with auto_reset: ccx_rollout of one step)
 * so a scripted agent that is terminated or truncated gets CCX_ACTION_ABSENT, and epsilon > 0 takes the counter-based
 * draws keyed on the env's own counters (the draws of the composition).  With CCX_EPS_STREAM_MT19937 selected AND
 * epsilon > 0 the call returns CCX_EINVAL: that stream is sequential per env and walked by a kernel of its own; with
 * epsilon = 0 the stream kind does not matter.  num_steps above 16 is cut into launches of at most 16 on the handle's
 * stream (an env's trajectory does not depend on the cut).  Handles whose short launches cannot use the step kernel
 * (ccx_get_step_shape: ok = 0, e.g. 100 x 100 grids) run the composition inside the library, step by step, through a
 * scratch action buffer allocated by the first such call.  The call only enqueues on the handle's stream: no host
 * synchronisation, no allocation after the first call, and it captures into a HIP graph (the unfused path after one
 * eager call).
 */
int ccx_rollout_mixed(ccx_handle* h, int32_t num_steps, int32_t policy, uint64_t scripted_slots,
                      const uint8_t* actions, const uint8_t* order, int32_t auto_reset,
                      const ccx_rollout_out* out, uint8_t* actions_out);
/*
 * CCX_ACTION_MASKS: which of its five actions would actually move an agent -- what a masked policy needs once per step,
 * on the device, next to the observations.  The reference answers it per agent and action through
 * GreedyPolicy._is_valid_action -> env._is_move_valid (baseline_policies/greedy_policy.py:238-264,
 * collectivecrossing.py:345-369); the policies' epsilon branch enumerates exactly that set (greedy_policy.py:51-57).
 *
 * `masks` is u8 [E][N], one byte per agent slot, and describes the state the handle holds when the call returns: behind
 * the launch's last step, and behind an auto-reset if one happened.
 *   - Agents the reference lists in env.agents (neither terminated nor truncated): bit a (a = 0..3: right, up, left,
 *     down, the action ids) is set iff _is_valid_action(id, a, env) is true on that state -- the target cell passes
 *     _is_valid_position (inclusive bounds, door row, tram walls) and no OTHER ACTIVE agent stands on it.  Bit 4 (wait)
 *     is always set.
 *   - Agents that are done: the byte is 0x10, wait only.  Done agents still block others according to their own `active`
 *     flag, as in _is_position_occupied: truncated agents block, arrived ones do not.
 *   - Bits 5-7 are zero.
 * Tied to the step itself: for a live agent i that is still ACTIVE, bit a is set <=> a step whose action tensor is
 * CCX_ACTION_ABSENT everywhere except actions[i] = a changes agent i's position, or a = 4.  (A live agent that has
 * arrived -- inactive, kept in env.agents by all_at_destination until everyone is there -- is answered as the reference
 * answers: _is_valid_action looks at the target cell only, while _move_agent, collectivecrossing.py:397-399, leaves an
 * inactive agent where it is.  Its bits follow _is_valid_action.)
 *
 * ccx_action_masks       the masks of the current state, by a kernel of its own (any legal grid; one pass over an env's
 *                        agents per thread).  Only enqueues on the handle's stream: it captures into a HIP graph.
 * ccx_bind_action_masks  while a pointer is bound (NULL unbinds), every call that advances the state also leaves the
 *                        masks of its final state there: ccx_step, ccx_rollout, ccx_rollout_policy, ccx_rollout_mixed and
 *                        ccx_step_finish.  One env-step without a move order on a handle whose short launches take the
 *                        step kernel (ccx_get_step_shape: ok = 1) writes them from that very launch (its sim wave does one
 *                        more round on the occupancy table behind the step); every other call is followed by the
 *                        stand-alone kernel on the same stream.  The bytes are the same either way.  The buffer is the
 *                        caller's and must stay valid while bound.
 * ccx_get_masks_fused    fused = 1 when such a call (num_steps, with / without a move order, mixed = through
 *                        ccx_rollout_mixed) is ONE kernel with the masks bound, 0 when the stand-alone kernel follows it.
 */
int ccx_action_masks(ccx_handle* h, uint8_t* masks);
int ccx_bind_action_masks(ccx_handle* h, uint8_t* masks_or_null);
int ccx_get_masks_fused(ccx_handle* h, int32_t num_steps, int32_t has_order, int32_t mixed, int32_t* fused);
/*
 * CCX_RESET_OBS: what the observation rows of a step that RESTARTED its env hold.  A learner on the device feeds the rows of
 * step t into its network to pick the actions of step t + 1; on the step where an env auto-resets, the rows it needs are
 * those of the NEW episode's first state (the reference's loop: `if done: obs, _ = env.reset(seed=...)`,
 * scripts/run_greedy_policy_demo.py:67-109; Gymnasium's SAME_STEP autoreset with `final_obs`).  Opt-in per handle.
 *
 *   CCX_RESET_OBS_TERMINAL (default)  obs[s][e] / obs_compact[s][e] are the rows of the step itself, also where the env
 *                                     restarted behind it: the bytes every earlier version wrote.
 *   CCX_RESET_OBS_NEXT                for every (step s, env e) whose env-flag byte carries CCX_EF_RESET:
 *     1. obs[s][e][a][:] for ALL N slots = the DefaultObservation rows of the restarted state: the placement of pool entry
 *        (global_env + episode * stride) mod P (the cursor of ccx_set_reset_pool) for the episode that restart opened,
 *        every agent active -- the bytes ccx_observe would write immediately after that restart;
 *     2. obs_compact[s][e][a] = (x, y, type, 1) of the same state;
 *     3. the rows TERMINAL mode writes at obs[s][e] / obs_compact[s][e] go to final_obs[s][e] / final_compact[s][e] where a
 *        side buffer is bound (ccx_bind_final_obs).  The side buffers have the shape and indexing of the call's own obs /
 *        obs_compact ([K][E][N][L] / [K][E][N][4] for a rollout of K steps) and the alignment asked of those.  Rows of
 *        (s, e) WITHOUT CCX_EF_RESET are not written at all: the caller's bytes stay.  A NULL side buffer drops the rows.
 *     4. nothing else changes: rewards, agent_flags (CCX_AF_OBS keeps describing the finished step), env_flags, the state,
 *        the counters, bound masks and episode statistics are bit for bit those of TERMINAL mode.
 *   Only steps with auto-reset and a reset pool raise CCX_EF_RESET: every other call is untouched by the mode.
 *
 * Serves ccx_rollout, ccx_rollout_policy, ccx_rollout_mixed and ccx_step_finish(auto_reset = 1) on every config ccx_create
 * accepts.  With auto-reset in NEXT mode, a call that asks for obs or obs_compact but passes no env_flags returns
 * CCX_EINVAL (the restarted envs are found there).  One env-step from an action tensor without a move order, on a handle
 * whose short launches take the step kernel, redirects the rows inside that very launch; every other call is followed, on
 * the same stream, by ONE fix-up kernel for the whole call that walks env_flags per env, works each restart's episode
 * ordinal out of the handle's episode counter (episode[e] after the call minus the restarts later in the call), moves the
 * terminal rows to the side buffers and writes the restarted rows in place -- it touches the rows of restarted envs only.
 * The bytes are the same either way.  Every call only enqueues on the handle's stream, allocates nothing and captures into
 * a HIP graph.
 *
 * ccx_set_reset_obs        CCX_RESET_OBS_TERMINAL or CCX_RESET_OBS_NEXT.
 * ccx_bind_final_obs       the side buffers, bound like ccx_bind_action_masks: the caller's, valid while bound, NULL unbinds
 *                          (either one on its own).
 * ccx_get_reset_obs_fused  fused = 1 when such a call (num_steps, with / without a move order, mixed = through
 *                          ccx_rollout_mixed) redirects the rows in the step's own launch, 0 when the fix-up kernel follows.
 */
#define CCX_RESET_OBS_TERMINAL 0
#define CCX_RESET_OBS_NEXT     1
int ccx_set_reset_obs(ccx_handle* h, int32_t mode);
int ccx_bind_final_obs(ccx_handle* h, float* final_obs_or_null, float* final_compact_or_null);
int ccx_get_reset_obs_fused(ccx_handle* h, int32_t num_steps, int32_t has_order, int32_t mixed, int32_t* fused);
/*
 * CCX_EPISODE_STATS: how the episodes went -- per-agent episode returns and episode lengths, accumulated on the device from
 * the reward / flag arrays a step or a rollout wrote, plus an optional log of finished episodes.  The reference's demos end
 * with exactly this: examples/waiting_policy_demo.py:52-85 (`total_reward += reward`, the step count) and
 * examples/training_script.py:95-97 (episode_return_min / mean / max).  Opt-in per handle; nothing else changes behaviour.
 *
 * Per env e the handle keeps
 *   running accumulators  ret f64 [E][N], live_steps i32 [E][N], steps i32 [E];
 *   a latch               closed u8 [E];
 *   finished i32 [E]      records this env has emitted since enable;
 *   the most recent finished episode: last_ret f64 [E][N], last_live_steps i32 [E][N], last_steps i32 [E], last_end u8 [E]
 *                         (all zero before the first finished episode).
 * ccx_episode_stats_update walks the steps s = 0 .. num_steps - 1 of its arrays in order, with af = agent_flags[s][e][a]
 * and ef = env_flags[s][e]:
 *   1. if not closed: steps += 1, and for every agent with af & CCX_AF_LIVE: ret = ret + reward[s][e][a], live_steps += 1.
 *      ONE f64 add per step, in step order: no reassociation, no compensation -- the bits of the reference's left-to-right
 *      `total += reward`.  Reward values of agents that are not live are never read into the sum.
 *   2. if ef & (CCX_EF_ALL_TERMINATED | CCX_EF_ALL_TRUNCATED) and not closed: emit a record (global env index
 *      env_offset + e, episode ordinal = finished, steps, end = ef & 3, ret[.], live_steps[.]), copy it into last_*,
 *      finished += 1, closed = 1.
 *   3. if ef & CCX_EF_RESET: ret, live_steps, steps = 0 and closed = 0.
 * The latch is what makes step-wise loops without auto-reset right: `__all__` stays raised step after step once an env is
 * done and not restarted, and only the first raise ends the episode.
 *
 * Log (optional, log_capacity = C records, struct of arrays): log_env i64 [C], log_episode i32 [C], log_steps i32 [C],
 * log_end u8 [C], log_ret f64 [C][N], log_live_steps i32 [C][N], and log_count u64 [2] = { stored, dropped }.  The records
 * of ONE update are appended behind those of earlier updates in env-major order (ascending e, then ascending s): counted per
 * env, placed by an exclusive scan, then written -- no atomic decides the order.  Records that would land at or beyond C
 * are dropped and counted exactly.  The log pointers are NULL when C = 0 (log_count stays { 0, 0 }).
 *
 * ccx_episode_stats_enable   synchronous; allocates the buffers and zeroes everything; log_capacity 0 = no log; calling it
 *                            again reallocates (and zeroes).
 * ccx_episode_stats_disable  turns tracking off and frees the buffers (synchronises the handle's stream).
 * ccx_episode_stats_view     the device pointers of the handle's own buffers (valid until disable / enable / destroy).
 * ccx_episode_stats_update   reward f64 [K][E][N], agent_flags u8 [K][E][N], env_flags u8 [K][E] (what ccx_rollout_out /
 *                            ccx_step_out hold).  Only enqueues on the handle's stream: no host synchronisation, no allocation,
 *                            and it captures into a HIP graph.  A pure function of its three arrays and the accumulators -- it
 *                            never reads the env state -- so the same bytes cut into any sequence of calls leave the same
 *                            accumulators and the same set of records.  A NULL array, num_steps < 1, or tracking that is
 *                            not enabled: CCX_EINVAL.  Offsets are 64-bit (K E N may exceed 2^31).
 * ccx_episode_stats_launches kernels one update enqueues: 1 without a log (accumulate + last_*), 3 with one (records per
 *                            env from env_flags and the latch; exclusive scan + log fill level; accumulate + write records).
 * ccx_episode_stats_reset    env_mask device u8 [E], NULL = all envs: zeroes ret, live_steps, steps and the latch of the
 *                            masked envs; writes no record; leaves finished and last_* alone.  Only enqueues.
 * ccx_episode_log_clear      stored = dropped = 0.  Only enqueues.
 * While tracking is enabled ccx_reset_from_pool and ccx_reset_seeded call ccx_episode_stats_reset with their own mask (a
 * restarted env starts a new episode); ccx_set_state_host does NOT (it overwrites any part of the state, an episode
 * boundary is the caller's to declare).
 */
typedef struct ccx_episode_stats {
    double*   ret;              /* [E][N] */
    int32_t*  live_steps;       /* [E][N] */
    int32_t*  steps;            /* [E]    */
    uint8_t*  closed;           /* [E]    */
    int32_t*  finished;         /* [E]    */
    double*   last_ret;         /* [E][N] */
    int32_t*  last_live_steps;  /* [E][N] */
    int32_t*  last_steps;       /* [E]    */
    uint8_t*  last_end;         /* [E]    */
    int64_t*  log_env;          /* [C]    */
    int32_t*  log_episode;      /* [C]    */
    int32_t*  log_steps;        /* [C]    */
    uint8_t*  log_end;          /* [C]    */
    double*   log_ret;          /* [C][N] */
    int32_t*  log_live_steps;   /* [C][N] */
    uint64_t* log_count;        /* [2] = { stored, dropped } */
    int64_t   log_capacity;     /* C */
} ccx_episode_stats;
int ccx_episode_stats_enable(ccx_handle* h, int64_t log_capacity);
int ccx_episode_stats_disable(ccx_handle* h);
int ccx_episode_stats_view(ccx_handle* h, ccx_episode_stats* out);
int ccx_episode_stats_launches(ccx_handle* h, int32_t* launches);
int ccx_episode_stats_update(ccx_handle* h, int32_t num_steps, const double* reward /* [K][E][N] */,
                             const uint8_t* agent_flags /* [K][E][N] */, const uint8_t* env_flags /* [K][E] */);
int ccx_episode_stats_reset(ccx_handle* h, const uint8_t* env_mask);
int ccx_episode_log_clear(ccx_handle* h);
/*
 * CCX_GAE: generalised advantage estimates and value targets from the arrays a rollout left on the device plus a critic's
 * values -- the step between ccx_rollout_out and a policy-gradient update (the reference trains with PPO,
 * examples/training_script.py).  ccx_episode_stats_update is the forward pass over reward / agent_flags / env_flags; this is
 * the backward pass over the same three arrays.
 *
 * A pure function of its arrays: it never reads the env state; E and N come from the handle.  All arithmetic is IEEE
 * binary32: every operation named below is ONE correctly rounded f32 operation, nothing is fused (no fma), nothing is
 * reassociated, subnormals are kept.
 *
 * Inputs (device pointers):
 *   reward        f64 [K][E][N]   what ccx_rollout_out / ccx_step_out hold
 *   agent_flags   u8  [K][E][N]   likewise
 *   env_flags     u8  [K][E]      likewise
 *   values        f32 [K][E][N]   values[s] = the critic's value of the observation the agent ACTED ON in step s (the state
 *                                 before step s)
 *   last_values   f32 [E][N]      value of the state behind step K - 1
 *   final_values  f32 [K][E][N] or NULL: value of the observation step s ENDED ON, read only at cut steps (below).  NULL: a
 *                                 cut bootstraps from +0.0, the usual "truncation = termination" shortcut
 *   gamma, lam    float, by value, each in [0, 1] and not NaN (else CCX_EINVAL); gl = gamma * lam is one f32 multiply on the
 *                                 host
 * Outputs: advantages f32 [K][E][N], returns f32 [K][E][N] (every element of both is written), valid u8 [K][E][N] or NULL.
 *
 * For every column (e, a) independently, the steps walked BACKWARDS:
 *     carry = +0.0f
 *     for s = K-1 .. 0:
 *         af = agent_flags[s][e][a];  ef = env_flags[s][e]
 *         if !(af & CCX_AF_LIVE):            (no reward entry exists for this agent-step)
 *             advantages = returns = +0.0f; valid = 0; carry = +0.0f; continue
 *         v = values[s][e][a];  r = (float)reward[s][e][a]                    (round to nearest even)
 *         cut = (af & CCX_AF_TRUNCATED) || (ef & (CCX_EF_ALL_TERMINATED | CCX_EF_ALL_TRUNCATED | CCX_EF_RESET))
 *         if   af & CCX_AF_TERMINATED:  nv = +0.0f;                                           c = +0.0f
 *         elif cut:                     nv = final_values ? final_values[s][e][a] : +0.0f;    c = +0.0f
 *         elif s == K-1:                nv = last_values[e][a];                               c = +0.0f
 *         else:                         nv = values[s+1][e][a];                               c = carry
 *         delta = (r + gamma * nv) - v        (mul, add, sub)
 *         adv   = delta + gl * c              (mul, add: the same two operations in every case)
 *         advantages[s][e][a] = adv;  returns[s][e][a] = adv + v;  valid = 1;  carry = adv
 * The pseudo-code is the contract, also for arrays no kernel of this library writes (a live step followed by a step that is
 * not live with no cut between them reads values[s+1] all the same).  Values at places the rule does not read never reach
 * a result: they are selected away, never multiplied by zero (a NaN there stays there).
 *
 * Termination does not bootstrap.  Truncation, the end of an episode of the whole env and an auto-reset do, from the value of
 * the rows the step ENDED ON: with CCX_RESET_OBS_NEXT those are the final_obs rows, not the next episode's rows that took
 * their place in obs -- the caller evaluates the critic on final_obs at the steps with CCX_EF_RESET and hands the result
 * in as final_values.  Agents of one env finish on different steps (CCX_AF_LIVE drops per agent while the env goes on),
 * several episodes of one env may start and end inside one array (CCX_EF_RESET), and without auto-reset the `__all__` flags
 * stay raised step after step: each such step is a cut of its own.
 * lam = 1 with values = 0 (and last_values = 0, final_values NULL) gives the discounted rewards-to-go of every episode:
 * adv[s] = r[s] + gamma * adv[s+1] inside an episode.  lam = 0 gives the one-step TD errors: adv[s] = (r + gamma * nv) - v,
 * plus gl * c = +0.0 * c.
 *
 * ccx_gae only enqueues ONE kernel on the handle's stream: no host synchronisation, no allocation, and it captures into a
 * HIP graph.  A NULL required pointer, num_steps < 1, or gamma / lam outside [0, 1] (NaN included): CCX_EINVAL with a
 * ccx_last_error message.  Offsets are 64-bit (K E N may exceed 2^31).
 */
int ccx_gae(ccx_handle* h, int32_t num_steps, const double* reward /* [K][E][N] */, const uint8_t* agent_flags /* [K][E][N] */,
            const uint8_t* env_flags /* [K][E] */, const float* values /* [K][E][N] */, const float* last_values /* [E][N] */,
            const float* final_values_or_null /* [K][E][N] */, float gamma, float lam, float* advantages /* [K][E][N] */,
            float* returns /* [K][E][N] */, uint8_t* valid_or_null /* [K][E][N] */);
/*
 * CCX_SAMPLE: from a network's logits to the action tensor ccx_step consumes -- masked categorical sampling on the device,
 * with the log-probability a policy-gradient update needs later and the entropy of the masked distribution.  The draw is
 * the library's own counter-based word (ccx_set_rng_seed below), keyed by (global env, episode, step of the episode, agent
 * slot): the same actions for any split of a run into calls, any world size, eager or captured.  Every output is
 * bit-defined.
 *
 * Inputs (device pointers): logits f32 [E][N][5] (index = action id; 16-byte aligned), masks u8 [E][N] or NULL (the bytes of
 * CCX_ACTION_MASKS; NULL = everything legal), deterministic (0 = sample, otherwise the masked argmax).  Outputs: actions u8
 * [E][N], logp f32 [E][N] or NULL, entropy f32 [E][N] or NULL; every element of every output given is written.  The call
 * reads the handle's terminated, truncated, step_count and episode arrays and the seed of ccx_set_rng_seed; it writes
 * nothing but its outputs.
 *
 * All arithmetic is IEEE binary32: every operation named below is ONE correctly rounded f32 operation (+ - * /), nothing is
 * fused (no fma), nothing is reassociated, subnormals are kept.  For every slot (e, a) on its own, with g = env_offset + e,
 * j = episode[e], t = step_count[e], l_k = logits[e][a][k]:
 *   1. dead slot (terminated[e][a] or truncated[e][a]): actions = CCX_ACTION_ABSENT, logp = +0.0f, entropy = +0.0f; its
 *      logits and its mask byte are not read into any result.
 *   2. m = ((masks ? masks[e][a] : 0x1F) & 0x1F) | 0x10: action k is legal iff bit k of m is set; wait always is.  A logit
 *      at an illegal k is selected away, never multiplied by zero (a NaN there stays there).
 *   3. mx = -inf; for legal k ascending: if (l_k > mx) mx = l_k.
 *   4. the slot is degenerate if a legal l_k is NaN or +inf, or mx == -inf.  Then d_k = +0.0f for every legal k (uniform
 *      over the legal set).  Otherwise d_k = l_k - mx (a legal -inf gives d_k = -inf and is fine).
 *   5. w_k = (d_k < D_MIN) ? +0.0f : exp_spec(d_k) for legal k, +0.0f for illegal k.  D_MIN = -80.0f: every nonzero weight
 *      is a normal number, and the weight of the maximum is exactly 1.
 *   6. c_0 = w_0, c_k = c_(k-1) + w_k, S = c_4 (1 <= S <= 5).
 *   7. u = word(seed_lo, seed_hi ^ 0x2545F491; g, j, t, a): the k of ccx_set_rng_seed's formula before "* 5", with g, j, t
 *      reduced to u32.  r = (float)(u >> 8) * 0x1p-24f (exact, in [0, 1)); thr = r * S.
 *   8. action = the lowest legal k with c_k > thr (none: k = 4; a k with w_k = 0 is never chosen).  deterministic: the
 *      lowest legal k with l_k == mx, in a degenerate slot the lowest legal k; no draw is made.
 *   9. logp = d_action - log_spec(S).
 *  10. entropy = log_spec(S) - T / S, T = (((t_0 + t_1) + t_2) + t_3) + t_4 with t_k = (w_k == 0) ? +0.0f : w_k * d_k.
 *
 * exp_spec(x), x in [-80, 0] here and in CCX_EVALUATE, in [-80, 80] in CCX_PPO_LOSS:
 *     n = rint(x * 0x1.715476p+0f)                              (round to nearest even)
 *     r = (x - n * 0x1.62e4p-1f) - n * 0x1.7f7d1cp-20f           (the first product is exact)
 *     p = 0x1.a01a02p-13f;  then p = p * r + C, one multiply and one add each, for C = 0x1.6c16c2p-10f, 0x1.111112p-7f,
 *         0x1.555556p-5f, 0x1.555556p-3f, 0x1p-1f, 0x1p+0f, 0x1p+0f                 (1/7! .. 1/2!, 1, 1)
 *     exp_spec = p * 2^n                                         (exact; |n| <= 116)
 * log_spec(s), s in [1, 5]:
 *     s = m * 2^e with m in [0.5, 1) (exact); if (m < 0x1.6a09e6p-1f) { m = m + m; e = e - 1; }
 *     t = m - 0x1p+0f;  q = t / (0x1p+1f + t);  z = q * q
 *     p = 0x1.c71c72p-4f;  then p = p * z + C for C = 0x1.24924ap-3f, 0x1.99999ap-3f, 0x1.555556p-2f        (1/9 .. 1/3)
 *     u = q + q;  lf = u + u * (z * p)
 *     log_spec = (float)e * 0x1.62e4p-1f + (lf + (float)e * 0x1.7f7d1cp-20f)
 * exp_spec(+0.0f) == 1.0f and log_spec(1.0f) == +0.0f exactly: a slot with one legal action has logp = entropy = +0.0f.
 * Against IEEE f64 (measured on the CPU, tests/test_sample_spec.py, maxima doubled): exp_spec within 2.0e-7 relative on
 * [-80, 0]; logp within 9.2e-7 and entropy within 4.3e-7 absolute of the f64 masked log-softmax and entropy of the same
 * f32 logits, over the adversarial generator's slots that are not degenerate.
 *
 * ccx_sample_actions only enqueues ONE kernel on the handle's stream: no host synchronisation, no allocation, and it
 * captures into a HIP graph next to ccx_step.  A NULL handle, NULL logits or NULL actions, or logits that are not 16-byte
 * aligned: CCX_EINVAL with a ccx_last_error message.  Not here: bf16 / f16 logits (cast first), a temperature (scale the
 * logits first).
 */
int ccx_sample_actions(ccx_handle* h, const float* logits /* [E][N][5] */, const uint8_t* masks_or_null /* [E][N] */,
                       int32_t deterministic, uint8_t* actions /* [E][N] */, float* logp_or_null /* [E][N] */,
                       float* entropy_or_null /* [E][N] */);
/*
 * CCX_EVALUATE: the learning side of CCX_SAMPLE -- log pi_new(a_stored | s) and the entropy of the masked distribution under
 * NEW logits for STORED actions, and the gradient of both with respect to those logits: what every epoch of a PPO update
 * needs after collection.  The distribution is CCX_SAMPLE's own (its steps 2-6 and 9-10, exp_spec and log_spec), so on the
 * logits an action was sampled from, logp and entropy equal ccx_sample_actions' outputs bit for bit: the ratio
 * exp(logp_new - logp_old) is exactly 1 before the first update.  Every output of both passes is bit-defined.
 *
 * A pure function of its arrays: it never reads the env state; the handle supplies only device and stream.  Rows are flat:
 * M >= 1 rows (any leading shape on the caller's side).  All arithmetic follows the discipline of CCX_SAMPLE: IEEE binary32,
 * every operation named below is ONE correctly rounded f32 operation (+ - * /), nothing is fused (no fma), nothing is
 * reassociated, subnormals are kept.
 *
 * Forward.  Inputs (device pointers): logits f32 [M][5] (index = action id; 16-byte aligned), actions u8 [M] (what
 * ccx_sample_actions wrote), masks u8 [M] or NULL (the bytes of CCX_ACTION_MASKS; NULL = everything legal).  Outputs: logp f32
 * [M], entropy f32 [M] or NULL; every element of every output given is written.  For every row i on its own, with
 * a = actions[i], l_k = logits[i][k]:
 *   - a == CCX_ACTION_ABSENT (255): logp = +0.0f, entropy = +0.0f; the row's logits and its mask byte are not read into any
 *     result (a NaN there stays there).
 *   - otherwise m, the legal set, mx, degenerate, d_k, w_k, c_k and S are exactly steps 2-6 of CCX_SAMPLE (a degenerate row
 *     is uniform over its legal set: d_k = +0.0f, w_k = 1 for every legal k), and
 *       entropy = log_spec(S) - T / S                      exactly step 10
 *       logp    = d_a - log_spec(S)                        if a <= 4 and a is legal under m: step 9.  A legal a with w_a = 0
 *                                                          gives a large negative or -inf logp; that follows from the rule
 *       logp    = -inf                                     if a is in 5..254, or a is illegal under m
 *
 * Backward.  Inputs: the forward's three inputs, grad_logp f32 [M] or NULL, grad_entropy f32 [M] or NULL (at least one of
 * the two is given).  Output: grad_logits f32 [M][5] (16-byte aligned), every element written.  The forward quantities are
 * recomputed from the logits; nothing is saved between the passes but the inputs.  For every row i on its own:
 *   - absent row (a == 255) or degenerate row: grad_logits[i][k] = +0.0f for all five k.
 *   - illegal k: grad_logits[i][k] = +0.0f, SELECTED, whatever the logit or the incoming gradients hold.
 *   - legal k of any other row, in this order of operations:
 *       p_k  = w_k / S                                     (one division)
 *       ls   = log_spec(S);  lp_k = d_k - ls
 *       H    = the forward's entropy, the same operation sequence
 *       t1_k = (k == a ? 1.0f : 0.0f) - p_k
 *       A_k  = grad_logp[i] * t1_k;  or +0.0f, selected, for every k when a is in 5..254 or illegal under m (logp = -inf
 *              has no gradient; a NaN in grad_logp[i] stays there)
 *       t2_k = (w_k == 0) ? +0.0f : p_k * (lp_k + H)       (one add, one multiply; lp_k may be -inf where w_k = 0: selected)
 *       B_k  = grad_entropy[i] * t2_k
 *       grad_logits[i][k] = A_k - B_k;   with grad_entropy NULL: A_k;   with grad_logp NULL: 0.0f - B_k
 *   These are d logp / d l_k = [k == a] - p_k and d entropy / d l_k = -p_k (log p_k + H) of the masked softmax.  A row with
 *   one legal action has logp = entropy = +0.0f and gradients +-0.  Incoming gradients at absent and degenerate rows are
 *   selected away, never multiplied by zero: the library's rule holds in the backward pass too.
 *
 * Against IEEE f64 (measured on the CPU, tests/test_evaluate_spec.py, maxima doubled), as max |err| / max(1, |f64 value|)
 * over the adversarial generator's rows that are not absent, not degenerate and whose stored action is legal with w_a > 0:
 * logp within 4.0e-7, entropy within 4.0e-7, the Jacobian of logp (grad_logp = 1 alone) within 4.1e-7 and the Jacobian of
 * the entropy (grad_entropy = 1 alone) within 3.7e-7 of the f64 masked log-softmax, its entropy and their f64 autograd
 * gradients on the same f32 logits.  logp carries its own bound, relative to its size: a sampled action sits near d = 0, a
 * stored one may sit at d near -80, where one rounding of l_a - mx is already 3.8e-6 absolute.
 *
 * Each entry point only enqueues ONE kernel on the handle's stream: no host synchronisation, no allocation, and it captures
 * into a HIP graph.  A NULL handle or a NULL required pointer (logits, actions, logp / grad_logits), rows < 1, rows so large
 * that the grid would pass 2^31 - 1 workgroups of 64 rows, logits or grad_logits that are not 16-byte aligned, or both
 * gradients NULL: CCX_EINVAL with a ccx_last_error message.  Offsets are 64-bit (5 M may exceed 2^31).  Not here: bf16 / f16
 * logits (cast first), a temperature (scale the logits first).  The PPO loss over these quantities: CCX_PPO_LOSS below.
 */
int ccx_evaluate_actions(ccx_handle* h, int64_t rows, const float* logits /* [M][5] */, const uint8_t* actions /* [M] */,
                         const uint8_t* masks_or_null /* [M] */, float* logp /* [M] */, float* entropy_or_null /* [M] */);
int ccx_evaluate_actions_backward(ccx_handle* h, int64_t rows, const float* logits /* [M][5] */, const uint8_t* actions /* [M] */,
                                  const uint8_t* masks_or_null /* [M] */, const float* grad_logp_or_null /* [M] */,
                                  const float* grad_entropy_or_null /* [M] */, float* grad_logits /* [M][5] */);
/*
 * CCX_PPO_LOSS: the clipped-surrogate PPO loss over the agent-steps that count, its statistics, and its gradient with respect
 * to the logits and the values -- the last link of an iteration (ccx_step / ccx_sample_actions / ccx_gae /
 * ccx_evaluate_actions being the others).  `valid` (ccx_gae's output) is a SELECTION inside the kernels: nothing is
 * compacted, shapes are static, there is no host synchronisation, and the whole update captures into a HIP graph.  Every
 * output is bit-defined, the reduction included.
 *
 * Pure functions of their arrays: the handle supplies device and stream only.  Rows are flat: M >= 1 rows.  The discipline
 * is CCX_SAMPLE's: every f32 operation named below is ONE correctly rounded f32 operation (+ - * /), nothing is fused (no
 * fma), nothing is reassociated, subnormals are kept; every f64 operation named below is likewise ONE correctly rounded f64
 * operation.  What a rule does not read is selected away, never multiplied by zero.
 *
 * Inputs (device pointers): logits f32 [M][5] (16-byte aligned), actions u8 [M], masks u8 [M] or NULL -- CCX_EVALUATE's
 * three; logp_old f32 [M] (ccx_sample_actions' logp), advantages f32 [M], returns f32 [M] (ccx_gae's), values f32 [M] (the
 * critic's, under the new weights), valid u8 [M] or NULL, norm f32 [2] = {mean, std} on the device or NULL (elements 1 and 2
 * of ccx_masked_moments' output), and by value clip in (0, 1), vf_coef >= 0, ent_coef >= 0, adv_eps >= 0 (all finite).
 *
 * Which rows count.  For the loss: row i counts iff (valid == NULL || valid[i] != 0) && actions[i] != 255.  For the
 * moments: iff valid == NULL || valid[i] != 0.  A row that does not count contributes to no sum and gets +0.0f in every
 * gradient, whatever its logits, values, advantages, logp_old or the incoming gradient hold (NaN included).  A NaN at a
 * row that counts propagates: that is the caller's data.
 *
 * Forward, per row that counts (f32, one operation each), with lo = 1.0f - clip, hi = 1.0f + clip and, where norm is given,
 * den = norm[1] + adv_eps computed once:
 *   1. logp, H = CCX_EVALUATE's forward for the row (the same operation sequence: its logp and entropy).
 *   2. x = logp - logp_old[i];  xc = x < -80.0f ? -80.0f : (x > 80.0f ? 80.0f : x);  ratio = exp_spec(xc)  (a NaN xc is
 *      passed through as the ratio and never enters exp_spec).  exp_spec is CCX_SAMPLE's, unchanged, on [-80, 80]: the first
 *      product of its reduction stays exact (|n| <= 115), the result is a normal number, exp_spec(+0.0f) == 1.0f.  On the
 *      logits an action was sampled from, x is +0.0f and ratio exactly 1.  An illegal stored action (logp = -inf) gives
 *      xc = -80, not a NaN.
 *   3. an = norm ? (advantages[i] - norm[0]) / den : advantages[i].
 *   4. s1 = ratio * an;  rc = ratio < lo ? lo : (ratio > hi ? hi : ratio);  s2 = rc * an;  surr = s2 < s1 ? s2 : s1.
 *   5. ve = values[i] - returns[i];  vl = ve * ve.
 *   6. kl = (ratio - 1.0f) - xc;  cf = (ratio < lo || ratio > hi) ? 1.0f : 0.0f.
 *
 * Reduction.  Six sums over the rows that count -- 1 (the count n), surr, vl, H, kl, cf -- in f64, each f32 term converted
 * exactly.  The tree is fixed by M alone (not by the CU count, a launch shape or a tunable); there is no floating-point
 * atomic:
 *   - rows are cut into B = ceil(M / 256) blocks of 256 consecutive rows, a block into four groups of 64 consecutive rows;
 *     rows that do not count and rows >= M enter as +0.0;
 *   - a group is reduced by halving: for o = 32, 16, 8, 4, 2, 1, at once for all 64 places j: s[j] = s[j] + s[j ^ o].  Every
 *     place ends with the same bits; G = s[0];
 *   - a block's partial is ((G0 + G1) + G2) + G3;
 *   - the final step takes the B partials P of a quantity: place j of 64 starts from +0.0 and adds P[j], P[j + 64], P[j + 128],
 *     ... in ascending order; the 64 places are then reduced by the same halving.
 * Final values, all in f64, each output rounded to f32 once (round to nearest even):
 *     policy = -(S_surr / n);  value = S_vl / n;  entropy = S_H / n
 *     loss   = (policy + (double)vf_coef * value) - (double)ent_coef * entropy
 *     stats  = {loss, policy, value, entropy, S_kl / n, S_cf / n, (float)n, +0.0f};   n == 0: all eight are +0.0f
 * ccx_masked_moments runs the same tree over 1, x and x * x (x converted to f64 exactly, the product exact) and gives, all
 * in f64 until the one rounding of each output:
 *     mean = S_x / n;  q = (S_xx - S_x * mean) / (n - 1);  var = q < 0 ? 0 : q;  std = sqrt(var)  (the correctly rounded f64
 *     square root, taken on the device: tests/test_gpu_ppo_loss.py compares its bits with IEEE sqrt on the host)
 *     out = {(float)n, (float)mean, (float)std, +0.0f};   n < 2: {(float)n, +0.0f, 1.0f, +0.0f} (no normalisation)
 * std is the unbiased (Bessel) standard deviation, torch.std's definition.
 *
 * Backward: one elementwise pass; nothing is saved but the inputs and stats.  g = grad_loss ? grad_loss[0] : 1.0f;
 * sc = g / stats[6];  gent = 0.0f - sc * ent_coef;  scv = sc * vf_coef, each computed once.  stats[6] == 0: every gradient is
 * +0.0f, selected.  For a row that counts, steps 1-5 are recomputed, then
 *     pass = !(ratio < lo || ratio > hi) || s1 < s2
 *     glp  = (pass && x == xc) ? 0.0f - sc * s1 : +0.0f       (d(-surr)/d logp = -an ratio = -s1 where the unclipped branch is
 *                                                              active and the clamp of x is not)
 *     grad_logits[i][.] = CCX_EVALUATE's backward for the row with grad_logp = glp, grad_entropy = gent: illegal places,
 *                         degenerate rows and an illegal stored action get exactly +0.0f by that rule
 *     grad_values[i]    = scv * (ve + ve)
 * At least one of grad_logits (16-byte aligned) and grad_values is given; a NULL one is not computed.  Every element of
 * every output given is written.
 *
 * Against IEEE f64 (measured on the CPU, tests/test_ppo_loss_spec.py, maxima doubled), as max |err| / max(1, |f64 value|)
 * against the textbook composition in f64 on the same f32 inputs (masked log-softmax, gather, guarded entropy, exp, clamp,
 * minimum, means over the rows that count, and their autograd gradients): exp_spec within 2.1e-7 relative on [-80, 80];
 * loss within 9.9e-8, policy 2.2e-8, value 6.7e-8, entropy 5.0e-8, approx_kl 2.4e-8; grad_values (times n) within 2.6e-7;
 * grad_logits (times n) within 2.2e-6 over rows with logp >= -10 and within 6.1e-5 over all rows (a stored action far down
 * the tail has a logp of size 80 and more, whose rounding -- 3.8e-6 absolute and up -- exp(logp - logp_old) turns into a
 * relative error of that row's gradient; the means average it away); the masked mean within 3.6e-8 and std within 8.3e-8.
 * The comparison leaves out rows where the two sides legitimately differ (ratio within one ulp of lo / hi, s1 == s2 outside
 * the range, |x| > 80, logp = -inf, and degenerate rows, which f64 softmax has no answer for): under 10 % of the generator's
 * counted rows, asserted.
 *
 * Launches: ccx_masked_moments and ccx_ppo_loss enqueue TWO kernels each on the handle's stream (block partials, then one
 * final wave), ccx_ppo_loss_backward ONE.  The final step is a launch of its own, not a last-block-done counter inside the
 * first: two plain launches cannot hang.  No host synchronisation, no allocation: the caller owns the workspace
 * (ccx_ppo_workspace_bytes(rows) bytes, 8-byte aligned, enough for either forward call; its contents mean nothing between
 * calls).  Everything captures into a HIP graph.  Offsets are 64-bit.  A NULL handle or a NULL required pointer, rows < 1 (or
 * so many that a grid would pass 2^31 - 1 workgroups), logits or grad_logits that are not 16-byte aligned, a workspace that
 * is not 8-byte aligned, a clip that is not finite or lies outside (0, 1), a negative or non-finite vf_coef, ent_coef or
 * adv_eps, or both gradient outputs NULL: CCX_EINVAL with a ccx_last_error message, before any launch.
 * ccx_ppo_workspace_bytes returns 0 for rows < 1.  Not here: value clipping, a KL penalty term, dual clipping, bf16 / f16
 * inputs, the optimiser, minibatch shuffling (a minibatch is whatever contiguous rows the caller hands in).
 */
int64_t ccx_ppo_workspace_bytes(int64_t rows);
int ccx_masked_moments(ccx_handle* h, int64_t rows, const float* x /* [M] */, const uint8_t* valid_or_null /* [M] */,
                       void* workspace, float* out /* [4] */);
int ccx_ppo_loss(ccx_handle* h, int64_t rows, const float* logits /* [M][5] */, const uint8_t* actions /* [M] */,
                 const uint8_t* masks_or_null /* [M] */, const float* logp_old /* [M] */, const float* advantages /* [M] */,
                 const float* returns /* [M] */, const float* values /* [M] */, const uint8_t* valid_or_null /* [M] */,
                 const float* norm_or_null /* [2] */, float clip, float vf_coef, float ent_coef, float adv_eps, void* workspace,
                 float* stats /* [8] */);
int ccx_ppo_loss_backward(ccx_handle* h, int64_t rows, const float* logits /* [M][5] */, const uint8_t* actions /* [M] */,
                          const uint8_t* masks_or_null /* [M] */, const float* logp_old /* [M] */,
                          const float* advantages /* [M] */, const float* returns /* [M] */, const float* values /* [M] */,
                          const uint8_t* valid_or_null /* [M] */, const float* norm_or_null /* [2] */, float clip, float vf_coef,
                          float ent_coef, float adv_eps, const float* stats /* [8] */, const float* grad_loss_or_null /* [1] */,
                          float* grad_logits_or_null /* [M][5] */, float* grad_values_or_null /* [M] */);
/*
 * CCX_MLP: the network between the observation rows and the logits -- a two-layer perceptron whose forward is a fixed
 * sequence of f32 operations per row.  The logits of a row depend on (L, H, O, activation), the row and the parameters only:
 * never on the number of rows, the row's index, the launch shape or the entry point.  So the logits an action was sampled
 * from are reproduced bit for bit by a later call on any batch that holds the row, and the ratio of CCX_EVALUATE on them is
 * exactly 1 for minibatches of any shape.  Every output is bit-defined.
 *
 * A pure function of its arrays (ccx_mlp_forward never reads the env state).  Inputs (device pointers), per row: x f32 [L];
 * shared: w1t f32 [L][H], the first layer INPUT-major (torch.nn.Linear(L, H).weight.t().contiguous(): for one k the H
 * weights are contiguous), b1 f32 [H], w2 f32 [O][H] (torch's layout), b2 f32 [O].  Limits: 1 <= L <= 512, H a multiple of
 * 16 with 16 <= H <= 256, 1 <= O <= 8, activation 0 = tanh, 1 = relu.  Outputs: y f32 [rows][O], hidden f32 [rows][H] or
 * NULL (the activations, for a backward pass); every element of every output given is written.
 *
 * All arithmetic follows the discipline of CCX_SAMPLE: IEEE binary32, every operation named below is ONE correctly rounded
 * f32 operation (+ - * /), nothing is fused (no fma), nothing is reassociated, subnormals are kept.  For every row on its own:
 *   1. layer 1, for every hidden unit j: a = b1[j]; for k = 0 .. L-1 in this order: a = a + x[k] * w1t[k][j]  (one multiply,
 *      one add).
 *   2. activation, h[j] = act(a):
 *        relu(a)      = (a < 0) ? +0.0f : a                       (NaN stays NaN, -0.0f stays -0.0f)
 *        tanh_spec(a) : m = (|a| < 40.0f) ? |a| : 40.0f
 *                       t = exp_spec(-(m + m))                     (CCX_SAMPLE's exp_spec, on its own domain [-80, 0])
 *                       r = (1.0f - t) / (1.0f + t)                (one subtraction, one addition, one division)
 *                       tanh_spec = (a != a) ? a : copysign(r, a)  (a select: a NaN pre-activation reaches the logits, where
 *                                                                  CCX_SAMPLE's degenerate-row rule takes over)
 *      tanh_spec(+-0.0f) = +-0.0f, and tanh_spec(a) = +-1.0f exactly from |a| = 8.67 on.  A NaN that an operation produces or
 *      passes on is a NaN in the outputs; its sign and payload are not defined (IEEE 754 leaves them to the implementation).
 *   3. layer 2.  The hidden units form G = H / 16 groups of 16 consecutive units.  For output o, the partial of group g is
 *      p_g = h[16g] * w2[o][16g]; then for i = 1 .. 15 in order p_g = p_g + h[16g + i] * w2[o][16g + i].  Then y[o] = b2[o];
 *      for g = 0 .. G-1 in order y[o] = y[o] + p_g.  (The groups exist so that an implementation may give the hidden units of
 *      one row to several lanes or waves and still have exactly one defined order.)
 * Against IEEE f64 (measured on the CPU, tests/test_mlp_spec.py, maxima doubled): tanh_spec within 1.9e-7 absolute of
 * tanh; the logits of L = 38, H = 64, O = 5 with torch.nn.Linear's initial weights on observation-like rows within
 * 1.5e-6 absolute of the f64 composition on the same f32 inputs.
 *
 * ccx_mlp_forward only enqueues ONE kernel on the handle's stream: no host synchronisation, no allocation, and it captures
 * into a HIP graph.  ccx_mlp_sample_actions is by definition ccx_sample_actions applied to what ccx_mlp_forward with
 * L = ccx_obs_len(N), O = 5 writes for the same obs [E][N][L] -- the same key, the same stream constant, the same rule for
 * terminated or truncated slots (255 / +0.0f / +0.0f), the same bits -- in ONE kernel; logits_or_null receives those logits
 * for every slot, dead ones included.  A NULL handle or a NULL required pointer (everything but hidden, masks, logp, entropy,
 * logits_or_null), rows < 1, rows beyond 2^31 - 1 workgroups of 64 rows, a size outside the limits, x / obs or hidden not
 * 16-byte aligned, or any other f32 array not 4-byte aligned: CCX_EINVAL with a ccx_last_error message, before any launch.
 * Offsets are 64-bit.
 *
 * Backward (ccx_mlp_backward): the gradients of the four parameter arrays, bit-defined.  Inputs (device pointers), M >= 1
 * rows: x f32 [M][L], hidden f32 [M][H] (what ccx_mlp_forward wrote), grad_y f32 [M][O], w2 f32 [O][H], activation; the
 * limits on L, H, O and activation are the forward's.  The discipline is the forward's and CCX_PPO_LOSS's: every f32
 * operation named is ONE correctly rounded f32 operation, every f64 operation named ONE correctly rounded f64 operation,
 * nothing is fused, nothing is reassociated, subnormals are kept.
 * Per row r, in f32 (a row's values depend on that row and w2 only):
 *   1. for every hidden unit j: gh = grad_y[r][0] * w2[0][j]; then for o = 1 .. O-1 in order gh = gh + grad_y[r][o] * w2[o][j].
 *   2. ga[r][j], with h = hidden[r][j]:
 *        tanh: hh = h * h;  d = 1.0f - hh;  ga = gh * d
 *        relu: ga = (h > 0.0f) ? gh : +0.0f                        (a select: a NaN h gives +0.0f)
 *      A NaN that an operation produces propagates; its sign and payload are not defined, as in the forward.
 * Terms.  Every term is the product of two f32 values converted to f64, which is exact in f64 (so acc + a * b as one f64 fma
 * and as an exact multiply followed by one add give the same bits; an implementation may use either):
 *     grad_w1t[k][j] sums (double)x[r][k] * (double)ga[r][j] over r        grad_b1[j] sums (double)ga[r][j]
 *     grad_w2[o][j]  sums (double)grad_y[r][o] * (double)hidden[r][j]      grad_b2[o] sums (double)grad_y[r][o]
 * Reduction over rows.  The tree is fixed by M alone (not by the CU count, a launch shape or a tunable); there is no
 * floating-point atomic:
 *   - rows are cut into B = ceil(M / 256) blocks of 256 consecutive rows;
 *   - a block's partial of an output element is a chain: it starts from +0.0 and adds the block's terms in ascending row
 *     order; rows >= M add nothing.  (A chain, not CCX_PPO_LOSS's halving, because the natural mapping differs: a thread
 *     owns output elements and walks the rows, a lane does not own a row, so no element needs a reduction across lanes.)
 *   - the final step over the B partials P of an element is CCX_PPO_LOSS's, unchanged: place j of 64 starts from +0.0 and adds
 *     P[j], P[j + 64], ... in ascending order; the 64 places are then halved, for o = 32, 16, 8, 4, 2, 1.
 * Each output is rounded to f32 once; every element of every output is written.  grad_a_or_null f32 [M][H] receives ga of
 * every row (bit-defined, per row).
 * Against IEEE f64 (measured on the CPU, tests/test_mlp_backward_spec.py, maxima doubled), as max |err| / max(1, |f64 value|)
 * against the textbook composition in f64 on the same f32 x, hidden, grad_y and w2 (gh = grad_y w2, ga = gh (1 - h^2) or
 * gh (h > 0), then matrix products), L = 38, H = 64, O = 5, torch.nn.Linear's initial weights, observation-like rows,
 * M = 20 000: grad_w1t within 2.9e-5, grad_b1 3.7e-6, grad_w2 1.2e-7, grad_b2 9.2e-8 (both sides read the same hidden, so no
 * row is left out).
 * ccx_mlp_backward only enqueues TWO plain launches on the handle's stream (block partials, then the final step; no
 * last-block-done counter, for the reason CCX_PPO_LOSS gives): no host synchronisation, no allocation, and it captures into
 * a HIP graph.  The caller owns the workspace: ccx_mlp_backward_workspace_bytes(rows, L, H, O) =
 * B * (L * H + H + O * H + O) * 8 bytes (46 MB at 524 288 rows of L = 38, H = 64, O = 5; 0 for rows < 1 or a shape outside the
 * limits), 8-byte aligned; its layout is private and its contents mean nothing between calls.  Offsets are 64-bit.  A NULL
 * handle or a NULL required pointer (everything but grad_a), rows < 1, B beyond 2^31 - 1, a shape outside the limits, x,
 * hidden or grad_a not 16-byte aligned, a workspace not 8-byte aligned, or any other f32 array not 4-byte aligned: CCX_EINVAL
 * with a ccx_last_error message, before any launch.
 *
 * Not here: wider networks (CCX_MLP_WIDE) or a second hidden layer (CCX_MLP_DEEP) in these entry points, bf16 / f16, the gradient with respect to x (observation rows are inputs and nothing
 * here learns upstream of them; the Python layer forms ga w1t^T in ordinary f32 torch when x requires a gradient: correct
 * to rounding, not bit-defined), the optimiser.
 */
int ccx_mlp_forward(ccx_handle* h, int64_t rows, int32_t L, int32_t H, int32_t O, int32_t activation, const float* x /* [rows][L] */,
                    const float* w1t /* [L][H] */, const float* b1 /* [H] */, const float* w2 /* [O][H] */, const float* b2 /* [O] */,
                    float* y /* [rows][O] */, float* hidden_or_null /* [rows][H] */);
int ccx_mlp_sample_actions(ccx_handle* h, int32_t H, int32_t activation, const float* obs /* [E][N][ccx_obs_len(N)] */,
                           const float* w1t /* [L][H] */, const float* b1 /* [H] */, const float* w2 /* [5][H] */,
                           const float* b2 /* [5] */, const uint8_t* masks_or_null /* [E][N] */, int32_t deterministic,
                           uint8_t* actions /* [E][N] */, float* logp_or_null /* [E][N] */, float* entropy_or_null /* [E][N] */,
                           float* logits_or_null /* [E][N][5] */);
int64_t ccx_mlp_backward_workspace_bytes(int64_t rows, int32_t L, int32_t H, int32_t O);
int ccx_mlp_backward(ccx_handle* h, int64_t rows, int32_t L, int32_t H, int32_t O, int32_t activation, const float* x /* [rows][L] */,
                     const float* hidden /* [rows][H] */, const float* grad_y /* [rows][O] */, const float* w2 /* [O][H] */,
                     void* workspace, float* grad_w1t /* [L][H] */, float* grad_b1 /* [H] */, float* grad_w2 /* [O][H] */,
                     float* grad_b2 /* [O] */, float* grad_a_or_null /* [rows][H] */);
/*
 * CCX_ADAM: one optimiser step over a set of f32 parameter tensors -- the global gradient norm, the clip scale, and Adam
 * with decoupled weight decay (AdamW; the only kind) -- the link between ccx_mlp_backward's gradients and the next forward.
 * The step counter and the bias corrections live on the device, so a captured graph advances them on replay.  Every output
 * is bit-defined, the norm's reduction included.  A pure function of its arrays: the handle supplies device and stream only.
 *
 * The discipline is CCX_SAMPLE's and CCX_PPO_LOSS's: every f32 operation named below is ONE correctly rounded f32 operation
 * (+ - * / sqrt), every f64 operation ONE correctly rounded f64 operation, nothing is fused (no fma), nothing is
 * reassociated, subnormals are kept, and a choice is a select.
 *
 * Inputs: T tensors, 1 <= T <= CCX_ADAM_MAX_TENSORS, as a HOST array of ccx_adam_tensor (it is copied into the kernel
 * arguments: no host-to-device copy is enqueued).  Each row: param, grad, m, v (device pointers, contiguous f32, 16-byte
 * aligned, numel >= 1 elements each, no two overlapping).  param, m and v are updated in place; grad is read only -- the
 * clipped gradient is never stored.  By value: lr >= 0, 0 <= beta1 < 1, 0 <= beta2 < 1, eps > 0, weight_decay >= 0,
 * max_grad_norm >= 0 (0 = no clipping), all finite.  lr_dev_or_null: when given, the rate is lr_dev[0] (a device scalar: a
 * schedule works under a captured graph) and the by-value lr is not used.
 *
 * 1. Sum of squares, by the tree of CCX_PPO_LOSS.  The elements form a virtual sequence: the tensors in table order, each
 *    padded to a multiple of 256 places, so a block of 256 places never straddles two tensors and B = sum ceil(numel_t / 256).
 *    A place that exists contributes the exact f64 product (double)g * (double)g, a padding place +0.0.  Groups of 64 places
 *    are reduced by halving, four groups to a block as ((G0 + G1) + G2) + G3, and the B block partials by the final step
 *    (place j of 64 adds P[j], P[j + 64], ... in ascending order onto +0.0; the 64 places are halved).  The result is S.
 *    The tree depends on the list of numel alone.
 * 2. Norm and skip.  nd = sqrt(S) in f64;  gn = (float)nd;  skip = gn is NaN or +inf (any NaN or +-inf among the gradients,
 *    or a norm beyond f32).  When skip holds, every param, m, v, pow1, pow2 and step keep their bits, state.skipped increases
 *    by one and stats[2] = 1.0f.
 * 3. Scale.  max_grad_norm > 0:  den = gn + 1e-6f;  c = max_grad_norm / den;  scale = c < 1.0f ? c : 1.0f  (computed from gn
 *    whether or not skip holds).  max_grad_norm == 0: the gradient is used as it is and scale = 1.0f.
 * 4. Bias corrections, without pow (whose bits no libm promises).  state keeps the f64 running products pow1 and pow2, both
 *    1.0 at the start.  A step that is not skipped:  pow1 = pow1 * (double)beta1;  pow2 = pow2 * (double)beta2;  step += 1.
 *    Then  bc1 = (float)(1.0 - pow1);  bc2 = (float)(1.0 - pow2);  once per call in f64, rounded to f32 once each,
 *    omb1 = (float)(1.0 - (double)beta1);  omb2 = (float)(1.0 - (double)beta2);  once per call in f32,  lrwd = lr * weight_decay.
 * 5. Per element of a step that is not skipped (f32, one rounding each):
 *      gs = max_grad_norm > 0 ? g * scale : g
 *      pd = weight_decay != 0 ? p - p * lrwd : p                         (two operations)
 *      m' = beta1 * m + omb1 * gs                                        (three operations)
 *      gg = gs * gs;   v' = beta2 * v + omb2 * gg                        (three operations)
 *      mh = m' / bc1;  vh = v' / bc2;  dn = sqrt(vh) + eps;  u = mh / dn
 *      p' = pd - lr * u                                                  (two operations)
 * Outputs: stats f32 [4] = {gn, scale, skip ? 1.0f : 0.0f, the lr used}.  state: 64 bytes on the device, 8-byte aligned --
 * f64 pow1, f64 pow2, i64 step, i64 skipped, 32 reserved bytes (zero; never written).  A fresh state is {1.0, 1.0, 0, 0, 0...}.
 *
 * Against IEEE f64 (measured on the CPU, tests/test_adam_spec.py, maxima doubled), as max |err| / max(1, |f64 value|) against
 * torch.optim.AdamW / Adam with clip_grad_norm_ in f64 on the same f32 gradients, 50 steps of the two-head set (5 382
 * parameters, lr = 3e-4, max_grad_norm = 0.5, 17 steps clipped): parameters within 7.8e-7 without weight decay and within
 * 4.8e-6 with weight_decay = 0.01 (where a parameter hardly moves, p - p * lrwd rounds the same way step after step), m
 * within 2.8e-9, v within 6.7e-11 (absolute: |m| and |v| are far below 1 there); gn within one f32 ulp of the f64 norm.
 *
 * ccx_adam_step only enqueues THREE plain launches on the handle's stream: block partials; one final wave (norm, skip, scale,
 * bias corrections, the state advance, stats); the element update, which on a skip returns without a store.  No workgroup
 * reads a word that another workgroup of the same launch writes; there is no floating-point atomic, no last-block-done
 * counter, no grid synchronisation, no host synchronisation and no allocation, and everything captures into a HIP graph.
 * The caller owns the workspace: ccx_adam_workspace_bytes(T, numel) = 64 + 8 * B bytes (0 for a T or a numel outside the
 * limits), 8-byte aligned; its contents mean nothing between calls.  Offsets are 64-bit.  A NULL handle or a NULL required
 * pointer, T outside 1..32, a numel < 1 (or beyond 2^40, or B beyond 2^31 - 1), a tensor pointer that is not 16-byte aligned,
 * a state or workspace that is not 8-byte aligned, or a hyper-parameter outside its range: CCX_EINVAL with a ccx_last_error
 * message, before any launch.  Not here: other optimisers, L2-coupled weight decay, amsgrad, per-tensor norms, per-group
 * hyper-parameters, bf16 / f16 state, writing the clipped gradients back.
 */
#define CCX_ADAM_MAX_TENSORS 32
typedef struct ccx_adam_tensor {
    float*       param;
    const float* grad;
    float*       m;
    float*       v;
    int64_t      numel;
} ccx_adam_tensor;
int64_t ccx_adam_workspace_bytes(int32_t num_tensors, const int64_t* numel /* host [T] */);
int ccx_adam_step(ccx_handle* h, int32_t num_tensors, const ccx_adam_tensor* tensors /* host [T] */, float lr,
                  const float* lr_dev_or_null /* [1] */, float beta1, float beta2, float eps, float weight_decay,
                  float max_grad_norm, void* state /* 64 bytes */, void* workspace, float* stats /* [4] */);
/*
 * CCX_SIDES: several heads of CCX_MLP, each owning a set of agent slots, run directly on the [..][N][L] arrays a rollout
 * wrote -- the two policies ("boarding", "exiting") the reference trains, a learner beside scripted agents, or a head per
 * agent -- without a gathered copy.  Nothing about the arithmetic is new: every output is, bit for bit, what an existing
 * call gives on the gathered rows, and no tolerance enters anywhere.
 *
 * A group is a 64-bit slot mask and one head (w1t, b1, w2, b2: device pointers, CCX_MLP's layouts).  Bit a of the mask
 * stands for agent slot a, boarding slots first (ccx_rollout_mixed's convention).  A call takes 1 to
 * CCX_SIDES_MAX_GROUPS groups as a HOST array of ccx_slot_group (it is copied into the kernel arguments: no host-to-device
 * copy is enqueued); the masks are non-empty, pairwise disjoint and have no bit at or above N (1 <= N <= 64); all groups of
 * a call share (L, H, O, activation), within CCX_MLP's limits.
 *
 * An array x is [M][N][L], M >= 1 the product of the leading dimensions.  The SELECTED rows of a group are the flat rows
 * m * N + a with bit a set, in ascending flat index: m-major, then a ascending.  S = popcount(mask); a group has M * S
 * selected rows, and selection index j = m * S + i names the i-th set bit of m.
 *
 * Forward (ccx_sides_forward).  For every selected row of every group, y[row][0 .. O-1] (and hidden[row][0 .. H-1] when
 * given) are exactly CCX_MLP's outputs for x[row] under the group's parameters: the per-row sequence of CCX_MLP, which does
 * not depend on the row's place or on how many rows there are.  Rows of slots that no group owns are not read, and their y
 * and hidden bytes are not written.
 *
 * Fused sampling (ccx_sides_sample_actions): by definition ccx_sample_actions on the logits the forward with M = E,
 * L = ccx_obs_len(N), O = 5 assembles from obs [E][N][L] -- the same key (global env, episode, step, slot), the same rule
 * for terminated or truncated slots, the same bits in actions, logp and entropy -- in ONE kernel.  A slot that no group
 * owns gets action 255 (CCX_ACTION_ABSENT), logp = +0.0f and entropy = +0.0f, and its logits_or_null bytes are untouched;
 * every element of actions, logp and entropy is written.
 *
 * Backward (ccx_sides_backward; one group per call): grad_w1t, grad_b1, grad_w2, grad_b2 and grad_a are exactly what
 * ccx_mlp_backward gives on the gathered arrays -- the group's selected rows of x, hidden and grad_y, contiguous, in
 * selection order.  In detail: blocks of 256 SELECTED rows, chains in ascending selection order, B = ceil(M * S / 256)
 * block partials per element, then CCX_PPO_LOSS's final step.  The workspace is
 * ccx_mlp_backward_workspace_bytes(M * S, L, H, O) bytes.  grad_a_or_null is [M][N][H] and is written at the selected
 * rows only.
 *
 * ccx_sides_forward and ccx_sides_sample_actions enqueue ONE kernel on the handle's stream, ccx_sides_backward TWO plain
 * launches: no host synchronisation, no atomic, no allocation, and everything captures into a HIP graph.  Offsets are
 * 64-bit.  A NULL handle or a NULL required pointer (everything but hidden, masks, logp, entropy, logits and grad_a), M < 1
 * or beyond 2^40, N outside 1..64, more than CCX_SIDES_MAX_GROUPS groups or none, an empty mask, a mask with a bit at or
 * above N, overlapping masks, a grid beyond 2^31 - 1 workgroups (of 64 selected rows; of 256 in the backward), a shape
 * outside CCX_MLP's limits, x / obs, hidden or grad_a not 16-byte aligned, a workspace not 8-byte aligned, or any other
 * f32 array not 4-byte aligned: CCX_EINVAL with a ccx_last_error message, before any launch.
 *
 * Not here: groups of different (H, O, activation) in one launch, per-env slot assignments (the mask holds for every env,
 * as in ccx_rollout_mixed), the gradient with respect to x, critics inside the actor launch, bf16 / f16.
 */
#define CCX_SIDES_MAX_GROUPS 8
typedef struct ccx_slot_group {
    uint64_t     slots;
    const float* w1t;
    const float* b1;
    const float* w2;
    const float* b2;
} ccx_slot_group;
int ccx_sides_forward(ccx_handle* h, int64_t M, int32_t N, int32_t L, int32_t H, int32_t O, int32_t activation,
                      const float* x /* [M][N][L] */, int32_t num_groups, const ccx_slot_group* groups /* host [num_groups] */,
                      float* y /* [M][N][O] */, float* hidden_or_null /* [M][N][H] */);
int ccx_sides_sample_actions(ccx_handle* h, int32_t H, int32_t activation, const float* obs /* [E][N][ccx_obs_len(N)] */,
                             int32_t num_groups, const ccx_slot_group* groups /* host [num_groups] */,
                             const uint8_t* masks_or_null /* [E][N] */, int32_t deterministic, uint8_t* actions /* [E][N] */,
                             float* logp_or_null /* [E][N] */, float* entropy_or_null /* [E][N] */,
                             float* logits_or_null /* [E][N][5] */);
int ccx_sides_backward(ccx_handle* h, int64_t M, int32_t N, uint64_t slots, int32_t L, int32_t H, int32_t O, int32_t activation,
                       const float* x /* [M][N][L] */, const float* hidden /* [M][N][H] */, const float* grad_y /* [M][N][O] */,
                       const float* w2 /* [O][H] */, void* workspace, float* grad_w1t /* [L][H] */, float* grad_b1 /* [H] */,
                       float* grad_w2 /* [O][H] */, float* grad_b2 /* [O] */, float* grad_a_or_null /* [M][N][H] */);
/*
 * CCX_QLEARN: the two links a Q-learning iteration needs beside the heads, the optimiser and the rollout -- epsilon-greedy
 * actions over the legal set from a network's Q-values (the actor loop), and the double-DQN TD error with its Huber loss, its
 * means over the rows that count and its gradient with respect to the Q-values (the update).  Q-values are the [..][5]
 * outputs of CCX_MLP / CCX_SIDES (index = action id), the online and the target network being two sets of parameters.  Every
 * output is bit-defined, the reduction included.  The discipline is CCX_SAMPLE's and CCX_PPO_LOSS's: every f32 operation
 * named below is ONE correctly rounded f32 operation (+ - * /), nothing is fused (no fma), nothing is reassociated,
 * subnormals are kept; every f64 operation likewise.  What a rule does not read is SELECTED away, never multiplied by zero.
 *
 * greedy(v, m), the ONE argmax of this section, over five values v_k and a legal set m (bit k set = legal, bit 4 always):
 *     kg = the lowest legal k;  mx = -inf;  for legal k ascending: if (v_k > mx) { mx = v_k; kg = k; }
 * A NaN never wins (the comparison is false); a row of NaNs (or of -inf) gives the lowest legal k; ties go to the lowest
 * index; a value at an illegal k reaches no result.
 *
 * ccx_q_actions.  Inputs (device pointers): q f32 [E][N][5] (16-byte aligned), masks u8 [E][N] or NULL (the bytes of
 * CCX_ACTION_MASKS; NULL = everything legal), epsilon f32 [1] ON THE DEVICE or NULL (NULL = greedy: nothing is drawn and
 * neither step_count nor episode is read).  Outputs: actions u8 [E][N], explored u8 [E][N] or NULL; every element of every
 * output given is written.  The rate is a device scalar so that an annealed rate changes between the replays of a captured
 * actor loop without a re-capture.  For every slot (e, a) on its own, with the key (g, j, t, a) of CCX_SAMPLE step 7
 * (g = env_offset + e, j = episode[e], t = step_count[e]) and eps = epsilon[0]:
 *   1. dead slot (terminated[e][a] or truncated[e][a]): actions = CCX_ACTION_ABSENT, explored = 0; its Q-values and its mask
 *      byte reach no result.
 *   2. m = the legal set of CCX_SAMPLE step 2: ((masks ? masks[e][a] : 0x1F) & 0x1F) | 0x10.  Wait is always legal.
 *   3. kg = greedy(q[e][a], m).
 *   4. only with epsilon given: u1 = word(seed_lo, seed_hi ^ 0x68E31DA4; g, j, t, a);  r = (float)(u1 >> 8) * 0x1p-24f
 *      (exact, in [0, 1));  the slot explores iff r < eps.  By the comparison alone: a NaN eps never explores, eps <= 0 never
 *      does, eps >= 1 always does.
 *   5. u2 = word(seed_lo, seed_hi ^ 0xB5297A4D; g, j, t, a);  n = popcount(m);  idx = (u32)(((u64)u2 * n) >> 32);  choice =
 *      the idx-th legal k, ascending from idx = 0: uniform over the legal set, with a bias of at most n / 2^32.
 *   6. actions = explores ? choice : kg;  explored = explores ? 1 : 0 (0 in every slot when epsilon is NULL).
 * The two stream constants differ from each other, from 0 (CCX_POLICY_RANDOM), from 0x5BD1E995 (the scripted policies'
 * epsilon) and from 0x2545F491 (CCX_SAMPLE): the four draws of a slot are four words.  As in CCX_SAMPLE the actions are the
 * same for any split of a run into calls, any world size, eager or captured.
 *
 * ccx_td_loss / ccx_td_loss_backward.  Pure functions of their arrays: the handle supplies device and stream only.  Rows are
 * flat: M >= 1.  Inputs (device pointers): q f32 [M][5] (the online network at the state), actions u8 [M], reward f64 [M] (the
 * rollout's own), done u8 [M] (not zero: the step ended the agent's episode by termination, nothing is bootstrapped),
 * q_next_target f32 [M][5] (the target network at the next state), q_next_online f32 [M][5] or NULL (the online network at
 * the next state: double-Q; NULL: the target network chooses its own action), masks_next u8 [M] or NULL (the legal set of
 * the next state), valid u8 [M] or NULL, weights f32 [M] or NULL (importance weights of a prioritised replay), and by value
 * gamma in [0, 1] and huber_delta > 0 (+inf allowed: the squared error).  The three Q arrays are 16-byte aligned.
 * Per row i, with a = actions[i] and c = 0.5f * huber_delta computed once:
 *   1. the row counts iff (valid == NULL || valid[i] != 0) && a <= 4.  A row with (valid == NULL || valid[i] != 0) and a in
 *      5..254 does not count and is tallied in stats[7] (bad): a corrupt action is visible and poisons no mean.  a == 255
 *      (an absent agent) and valid[i] == 0 are the ordinary ways not to count.  A row that does not count contributes to no
 *      sum and gets +0.0f in td_error and in every gradient, whatever its inputs hold (NaN included).
 *   2. qa = q[i][a], selected.
 *   3. m' = CCX_SAMPLE step 2 on masks_next;  k* = greedy(q_next_online ? q_next_online[i] : q_next_target[i], m');
 *      boot = q_next_target[i][k*], selected.
 *   4. r = (float)reward[i] (one rounding, as CCX_GAE does it);  nb = (done[i] || gamma == 0.0f) ? +0.0f : gamma * boot
 *      (selected: a NaN in a terminal row's next-Q stays there, and gamma = 0 reads no next-state array into a result);
 *      y = r + nb.
 *   5. d = qa - y;  ad = |d|;  h = (ad <= huber_delta) ? 0.5f * (d * d) : huber_delta * (ad - c)  (two operations in either
 *      branch);  term = weights ? weights[i] * h : h.
 * Reduction: six sums over the rows -- 1 (the count n), term, ad, qa, y over the rows that count, and 1 over the bad rows --
 * in f64, each f32 term converted exactly, by the tree of CCX_PPO_LOSS, unchanged (blocks of 256 rows, groups of 64 by
 * halving, ((G0 + G1) + G2) + G3, the final wave).  Final values, in f64, each output rounded to f32 once:
 *     stats = {S_term / n, S_ad / n, S_qa / n, S_y / n, +0.0f, +0.0f, (float)n, (float)bad};  n == 0: the first six are +0.0f
 *     td_error[i] = counts ? d : +0.0f                           (written where td_error is given)
 * Backward: one elementwise pass that recomputes steps 1-5 from the same inputs; nothing is saved but the inputs and stats.
 * g = grad_loss ? grad_loss[0] : 1.0f;  sc = g / stats[6], computed once;  gw = weights ? sc * weights[i] : sc;
 *     dd = (ad <= huber_delta || d is NaN) ? d : (d < 0 ? -huber_delta : huber_delta)        (a NaN goes through loudly)
 *     grad_q[i][k] = (counts && k == a) ? gw * dd : +0.0f
 * Every element of grad_q (16-byte aligned) is written; rows that do not count, and stats[6] == 0, give exactly +0.0f
 * whatever the inputs hold.  No gradient reaches the next-state arrays: the target is a constant.
 *
 * Against IEEE f64 (measured on the CPU, tests/test_qlearn_spec.py, maxima doubled), as max |err| / max(1, |f64 value|)
 * against the textbook composition in torch f64 on the same f32 inputs (masked argmax, gather, where(done), Huber, mean
 * over the rows that count, autograd): loss within 1.1e-7, mean |td| within 9.9e-8, grad_q (times n) within 1.1e-6 (rows whose |d| lies within 1e-6 of
 * huber_delta, where the two sides may sit on different branches of the derivative, are left out: under 10 %, asserted).
 *
 * Launches: ccx_q_actions enqueues ONE kernel on the handle's stream, ccx_td_loss TWO (block partials, then one final
 * wave; no atomic, no last-block-done counter), ccx_td_loss_backward ONE.  No host synchronisation, no allocation: the
 * caller owns the workspace (ccx_td_workspace_bytes(rows) bytes, 8-byte aligned; 0 for rows < 1).  Everything captures into
 * a HIP graph.  Offsets are 64-bit.  A NULL handle or a NULL required pointer, rows < 1 (or so many that a grid would pass
 * 2^31 - 1 workgroups), a Q array or grad_q that is not 16-byte aligned, a workspace that is not 8-byte aligned, a gamma that
 * is not finite or lies outside [0, 1], a huber_delta that is not > 0: CCX_EINVAL with a ccx_last_error message, before any
 * launch.  n-step targets are CCX_NSTEP (a discount per row: ccx_td_loss_discounted).  The dueling combine and the head's forward fused with the action choice are CCX_DUELING.  Distributional (categorical, C51) heads are CCX_C51.  Not here: prioritised sampling (weights and td_error
 * are its two hooks; the replay buffer itself is CCX_REPLAY), bf16 / f16.
 */
int ccx_q_actions(ccx_handle* h, const float* q /* [E][N][5] */, const uint8_t* masks_or_null /* [E][N] */,
                  const float* epsilon_or_null /* device f32 [1]; NULL = greedy */, uint8_t* actions /* [E][N] */,
                  uint8_t* explored_or_null /* [E][N] */);
int64_t ccx_td_workspace_bytes(int64_t rows);
int ccx_td_loss(ccx_handle* h, int64_t rows, const float* q /* [M][5] */, const uint8_t* actions /* [M] */,
                const double* reward /* [M] */, const uint8_t* done /* [M] */, const float* q_next_target /* [M][5] */,
                const float* q_next_online_or_null /* [M][5] */, const uint8_t* masks_next_or_null /* [M] */,
                const uint8_t* valid_or_null /* [M] */, const float* weights_or_null /* [M] */, float gamma, float huber_delta,
                void* workspace, float* stats /* [8] */, float* td_error_or_null /* [M] */);
int ccx_td_loss_backward(ccx_handle* h, int64_t rows, const float* q /* [M][5] */, const uint8_t* actions /* [M] */,
                         const double* reward /* [M] */, const uint8_t* done /* [M] */, const float* q_next_target /* [M][5] */,
                         const float* q_next_online_or_null /* [M][5] */, const uint8_t* masks_next_or_null /* [M] */,
                         const uint8_t* valid_or_null /* [M] */, const float* weights_or_null /* [M] */, float gamma,
                         float huber_delta, const float* stats /* [8] */, const float* grad_loss_or_null /* [1] */,
                         float* grad_q /* [M][5] */);
/*
 * CCX_REPLAY: the replay memory of an off-policy loop on the device -- a ring of COMPACT env-step records whose cursor lives
 * on the device, filled from a rollout's own arrays (ccx_replay_push), and ONE kernel that draws B records with the
 * library's counter-based word and writes the minibatch as DefaultObservation rows plus the small arrays ccx_td_loss takes
 * (ccx_replay_sample; ccx_replay_fetch is the same kernel on the caller's record indices).  Everything is integer work and
 * copies: every output is bit-defined.
 *
 * The ring belongs to the caller and travels as arguments: ring_steps = S >= 1 steps of the handle's E envs, R = S E < 2^31
 * records, struct of arrays -- obs_c and next_c f32 [R][N][4] (CCX_OBS_COMPACT records, 16-byte aligned), actions u8, reward
 * f64, done u8, valid u8, masks_next u8, each [R][N], and state i64 [4] = {head, draws, 0, 0}.  One record is 44 N bytes; the
 * same env-step as two DefaultObservation rows per agent and the small fields is N (2 (24 + 16 N) + 12) bytes (N = 8: 352
 * against 2 528; N = 32: 1 408 against 34 688).  The EMPTY record, which the caller initialises the ring to (with head =
 * draws = 0): actions = CCX_ACTION_ABSENT, done = valid = 0, reward = +0.0, masks_next = 0x10, both compact records +0.0.
 *
 * ccx_replay_push.  A block of K steps, 1 <= K <= S: obs0_compact f32 [E][N][4] (the compact observation step 0 acted on),
 * actions u8 [K][E][N], and a rollout's reward f64 [K][E][N], agent_flags u8 [K][E][N], env_flags u8 [K][E], obs_compact f32
 * [K][E][N][4], final_compact (the same shape) or NULL, and masks_next u8 [K][E][N] or NULL (the legal set behind each step).
 * With head = state[0] READ ON THE DEVICE when the kernel runs, the record of step s and env e goes to slot
 *     ((head + s) mod S) * E + e
 * with, per agent slot,
 *     obs_c      = s == 0 ? obs0_compact[e] : obs_compact[s - 1][e]
 *     reset      = final_compact != NULL && (env_flags[s][e] & CCX_EF_RESET)
 *     next_c     = reset ? final_compact[s][e] : obs_compact[s][e]
 *     actions, reward: copied bit for bit
 *     done       = agent_flags & CCX_AF_TERMINATED          (0 / 1)
 *     valid      = agent_flags & CCX_AF_LIVE                (0 / 4)
 *     masks_next = (reset || masks_next == NULL) ? 0x1F : masks_next[s][e]
 * and then head += K.  K <= S makes the K slots distinct: a block may wrap inside itself, and K == S rewrites the whole
 * ring.  The records mean what they say only for a rollout made with CCX_RESET_OBS_NEXT (obs_compact[s][e] of a restarted env
 * is then the new episode's first observation, and final_compact[s][e] the one the step ended on): the caller's contract,
 * the library cannot see it.
 *
 * ccx_replay_sample.  With F = min(head, S) * E and d = draws = state[1], both read on the device when the kernel runs, and
 * the seed of ccx_set_rng_seed, for b = 0 .. B - 1 (1 <= B <= 2^31 / N):
 *     w0 = word(seed_lo, seed_hi ^ 0x3C6EF372; (u32)b, (u32)d, (u32)(d >> 32), 0)     (the k of ccx_set_rng_seed's formula)
 *     w1 = the same with 1 as the last key
 *     index[b] = F == 0 ? -1 : (i64)((((u64)w0 << 32) | w1) * F >> 64)               (the high half of the 128-bit product)
 * and then draws += 1.  The key holds neither env nor shard; draws are with replacement; the bias is below F / 2^64.  The
 * stream constant differs from 0, 0x5BD1E995, 0x2545F491, 0x68E31DA4 and 0xB5297A4D.  The minibatch is the same for any split
 * of the pushes into calls, eager or captured, and needs nothing from any other generator.  ccx_replay_fetch takes index
 * i64 [B] from the caller instead (and writes it to the index output, which may be the same array) and leaves draws alone.
 *
 * Gather (both).  Row b of every output is a copy of the fields of record index[b], bit for bit, and every element of every
 * output given is written: actions u8, reward f64, done u8, valid u8, masks_next u8, each [B][N], index i64 [B], and obs /
 * next_obs f32 [B][N][ccx_obs_len(N)] (each may be NULL; 16-byte aligned), the N DefaultObservation rows of the record's
 * obs_c / next_c: the very gather of ccx_observe and ccx_expand_observations with the handle's row constants, hence the bits
 * of ccx_expand_observations on those compact records.  An index outside [0, R) -- the -1 of an empty ring included -- gives
 * the EMPTY record and reads nothing; its rows are the rows of compact records of +0.0, like those of an empty slot.  An
 * index in [F, R) reads what is there: the empty record until the ring is full.
 *
 * Launches: ccx_replay_push and ccx_replay_sample enqueue TWO kernels on the handle's stream -- the main one, and one plain
 * lane behind it that adds to head / draws, so the update cannot race with the lanes that read the old value (no atomic, no
 * last-block-done counter); ccx_replay_fetch ONE.  No host synchronisation, no allocation; everything captures into a HIP
 * graph, and a captured push / sample advances with every replay.  Offsets are 64-bit.  A NULL handle or required pointer, S
 * < 1 or S E >= 2^31, K outside 1..S, B outside 1..2^31 / N, a compact or row array that is not 16-byte aligned, an f64 / i64
 * array that is not 8-byte aligned: CCX_EINVAL with a ccx_last_error message, before any launch.  Not here: prioritised or
 * recency-weighted sampling (index, ccx_replay_fetch and ccx_td_loss's weights / td_error are the hooks), sampling without
 * replacement from the ring (CCX_MINIBATCH shuffles a rollout's own records without replacement), frames shared between obs_c and next_c, records of single agents or of sequences, a ring over
 * several GPUs (each shard has its own), rows-form storage, bf16 / f16.
 */
int ccx_replay_push(ccx_handle* h, int64_t ring_steps, float* ring_obs_c /* [R][N][4] */, float* ring_next_c /* [R][N][4] */,
                    uint8_t* ring_actions /* [R][N] */, double* ring_reward /* [R][N] */, uint8_t* ring_done /* [R][N] */,
                    uint8_t* ring_valid /* [R][N] */, uint8_t* ring_masks_next /* [R][N] */, int64_t* ring_state /* [4] */,
                    int64_t K, const float* obs0_compact /* [E][N][4] */, const uint8_t* actions /* [K][E][N] */,
                    const double* reward /* [K][E][N] */, const uint8_t* agent_flags /* [K][E][N] */,
                    const uint8_t* env_flags /* [K][E] */, const float* obs_compact /* [K][E][N][4] */,
                    const float* final_compact_or_null /* [K][E][N][4] */, const uint8_t* masks_next_or_null /* [K][E][N] */);
int ccx_replay_sample(ccx_handle* h, int64_t ring_steps, float* ring_obs_c, float* ring_next_c, uint8_t* ring_actions,
                      double* ring_reward, uint8_t* ring_done, uint8_t* ring_valid, uint8_t* ring_masks_next, int64_t* ring_state,
                      int64_t batch, float* obs_or_null /* [B][N][L] */, float* next_obs_or_null /* [B][N][L] */,
                      uint8_t* actions /* [B][N] */, double* reward /* [B][N] */, uint8_t* done /* [B][N] */,
                      uint8_t* valid /* [B][N] */, uint8_t* masks_next /* [B][N] */, int64_t* index /* [B] */);
int ccx_replay_fetch(ccx_handle* h, int64_t ring_steps, float* ring_obs_c, float* ring_next_c, uint8_t* ring_actions,
                     double* ring_reward, uint8_t* ring_done, uint8_t* ring_valid, uint8_t* ring_masks_next, int64_t* ring_state,
                     int64_t batch, const int64_t* index_in /* [B] */, float* obs_or_null, float* next_obs_or_null,
                     uint8_t* actions, double* reward, uint8_t* done, uint8_t* valid, uint8_t* masks_next, int64_t* index);
/*
 * CCX_PRIO: proportional prioritised replay (Schaul et al.; the scheme of RLlib's prioritised buffers) over the ring of
 * CCX_REPLAY.  The priorities are FIXED-POINT INTEGERS, so every sum over them is exact: the total, and every partial sum
 * the draw walks through, have the same bits for any reduction order and any tree shape, a parent is exactly the sum of its
 * children (a descent cannot run off the end), and the whole rule is stated below in integers -- the tree is never named.
 * The two f32 rules (update, weights) follow the discipline of CCX_SAMPLE: every line is ONE correctly rounded f32
 * operation, nothing is fused, what a rule does not read is selected away.  exp_spec and log_spec are CCX_SAMPLE's,
 * unchanged; this section uses log_spec on [2^-31, 2^15] (its code takes any positive normal float) and exp_spec on
 * [-22, 11].
 *
 * Storage (the caller's, travelling as arguments; R = S E records of the ring): leaf i32 [R], the priority p^alpha of each
 * record with 16 fractional bits, 1 <= leaf <= 2^31 - 1, and 0 = never pushed / not drawable (the initial value); pstate
 * i64 [4] = {max_leaf, draws, T, min_leaf}: max_leaf the running maximum of every leaf ever written (initially 65536 =
 * 1.0), draws this section's own launch counter (not the ring's state[1]), T the sum of all leaves and min_leaf the
 * smallest non-zero leaf (0: none) as of the latest ccx_prio_sample; beta f32 [1] ON THE DEVICE (a rate annealed between
 * the replays of a captured graph needs no re-capture); and tree i64 [ccx_prio_tree_words(R)], work space that every
 * ccx_prio_sample rewrites in full before it reads it: nothing observable depends on its contents or its shape.  With R <
 * 2^31 and leaf < 2^31, T < 2^62.  Alignment: 8 bytes for the i64 arrays, 4 for i32 and f32.
 *
 * ccx_prio_push(ring_steps, ring_state, K, leaf, pstate).  Enqueued directly BEHIND a ccx_replay_push of K steps into the
 * same ring: with head' = ring_state[0] (which that push advanced by K) and max_leaf = pstate[0], both read on the device,
 *     leaf[((head' - K + s) mod S) * E + e] = max_leaf            for s = 0 .. K - 1, e = 0 .. E - 1
 * the K E slots that push wrote: a new record is drawn at least as often as any other until its TD error is known.  (head' -
 * K < 0, a caller that pushed nothing, counts as 0: the stores stay inside leaf.)
 *
 * ccx_prio_update(index i64 [B], num_td, td_error: HOST array of num_td <= 8 device pointers f32 [B][N], alpha, eps).  The
 * arrays are the per-side td_error outputs of ccx_td_loss (+0.0 where a row did not count).  Per b:
 *     m = +0.0;  for every array and agent: a = |td|;  m = a > m ? a : m        (a NaN never wins; +inf does)
 *     s = m + eps;  x = s < 2^-16 ? 2^-16 : (s > 2^15 ? 2^15 : s)
 *     p = alpha == 0 ? 1.0f : exp_spec(alpha * log_spec(x))
 *     f = floor(p * 65536.0f);  c = f > 0x1.fffffep+30f ? 0x1.fffffep+30f : f;  new = max((i32)c, 1)
 * (the cast is made after the clamp: it is always in range).  Per slot: the leaf becomes the MAXIMUM of the new values of
 * all b that name it -- duplicates are normal, the draw is with replacement; a b whose index lies outside [0, R), or names a
 * slot whose leaf is 0, changes nothing.  Then max_leaf = max(max_leaf, every new value written).  The result does not
 * depend on the order in which lanes run: a first launch stores -|leaf| at the named slots (every writer stores the same
 * value), a second does a signed integer atomic max of the new values; no floating-point atomic, no last writer.
 * 0 <= alpha <= 1 and 0 < eps < inf, by value.
 * Against f64 pow on the same x (measured on the CPU, tests/test_prio_spec.py, the maximum doubled): p is within a relative
 * 2.2e-6 for x in [2^-31, 2^15] and alpha in {0.3, 0.6, 1}.
 *
 * ccx_prio_sample(leaf, pstate, beta, tree, B, stratified) -> index i64 [B], weights f32 [B][N], leaf_drawn i32 [B].
 *   1. T = the sum of all leaves, min_leaf = the smallest non-zero leaf (0: none); both are written to pstate.
 *   2. per b, with d = pstate.draws read on the device and the seed of ccx_set_rng_seed:
 *        w0 = word(seed_lo, seed_hi ^ 0x7F4A7C15; (u32)b, (u32)d, (u32)(d >> 32), 0),  w1 = the same with 1 as the last key
 *        x  = ((u64)w0 << 32) | w1
 *        stratified:  x' = floor((b 2^64 + x) / B)  -- t1 = ((u64)b << 32) | w0;  q1 = t1 / B;  r1 = t1 % B;
 *                     t2 = (r1 << 32) | w1;  q2 = t2 / B;  x' = (q1 << 32) | q2  (b < B < 2^31: two 64-bit divisions);
 *                     draw b lies in the b-th of B equal strata.   Not stratified: x' = x.
 *        u  = (x' * T) >> 64                                           (the high half of the 128-bit product: 0 <= u < T)
 *        index[b] = the smallest i with leaf[0] + ... + leaf[i] > u;   T == 0: index[b] = -1
 *      With all non-zero leaves equal and in front (F of them), the unstratified index is CCX_REPLAY's (x F) >> 64 for the same words.
 *   3. leaf_drawn[b] = leaf[index[b]] (0 for -1);  r = (f32)((f64)min_leaf / (f64)leaf_drawn[b]);  bt = beta[0] clamped to
 *      [0, 1] (bt = beta < 0 ? 0 : (beta > 1 ? 1 : beta));  weights[b][n] = exp_spec(bt * log_spec(r)) for every n -- (p_min /
 *      p_i)^beta, the normalisation by the largest weight in the buffer; r == 1 gives exactly 1.0; index -1 gives +0.0.
 *   4. draws += 1.
 * The minibatch itself is ccx_replay_fetch on index.  The stream constant differs from those of every other section.
 *
 * Launches: ccx_prio_push ONE kernel; ccx_prio_update TWO; ccx_prio_sample the refresh (one workgroup per 256 leaves, once
 * more per 65 536 and per 16 777 216 where R exceeds them, then ONE final workgroup that writes T and min_leaf; no atomic, no
 * last-block-done counter), the draw, and one plain lane behind it that advances draws.  No host synchronisation, no
 * allocation; everything captures into a HIP graph and advances with every replay.  A NULL handle or pointer, S < 1 or S E >=
 * 2^31, K outside 1..S, B outside 1..2^31 / N (and B < 2^31), num_td outside 1..8, alpha or eps out of range, a misaligned
 * array: CCX_EINVAL with a ccx_last_error message, before any launch.  ccx_prio_tree_words(R) is 0 for R outside 1..2^31 - 1.
 * Not here: rank-based prioritisation, sampling without replacement, per-agent priorities, an incrementally updated tree,
 * priorities shared across shards or GPUs, bf16 / f16.
 */
int64_t ccx_prio_tree_words(int64_t records);
int ccx_prio_push(ccx_handle* h, int64_t ring_steps, const int64_t* ring_state /* [4] */, int64_t K, int32_t* leaf /* [R] */,
                  const int64_t* pstate /* [4] */);
int ccx_prio_update(ccx_handle* h, int64_t ring_steps, int32_t* leaf /* [R] */, int64_t* pstate /* [4] */, int64_t batch,
                    const int64_t* index /* [B] */, int32_t num_td, const float* const* td_error /* host [num_td] of device [B][N] */,
                    float alpha, float eps);
int ccx_prio_sample(ccx_handle* h, int64_t ring_steps, const int32_t* leaf /* [R] */, int64_t* pstate /* [4] */,
                    const float* beta /* device f32 [1] */, int64_t* tree /* [ccx_prio_tree_words(R)] */, int64_t batch,
                    int32_t stratified, int64_t* index /* [B] */, float* weights /* [B][N] */, int32_t* leaf_drawn /* [B] */);
/*
 * CCX_NSTEP: n-step targets over the ring of CCX_REPLAY.  The ring is step-major, so the successor of a record is the same
 * env one ring step on; one byte per record says whether the env's episode ended with it; and ONE kernel walks every drawn
 * record forward through up to n - 1 successors and writes the minibatch of ccx_replay_fetch with the discounted n-step
 * reward in the place of the reward, the state the window ends on in the place of the next state, and per row the discount
 * gamma^m its bootstrap takes (ccx_td_loss_discounted reads it where ccx_td_loss reads gamma).  The integer part is exact;
 * the f64 chain follows the discipline of CCX_QLEARN: every line is ONE correctly rounded operation, nothing is fused, what
 * a rule does not read is SELECTED away, never multiplied by zero.
 *
 * Storage (the caller's, travelling as arguments): cut u8 [R], one byte per record (env-step) of the ring, initially 0.  Not
 * zero: the episode of env e ended with this step, the record in the next ring step is not its continuation.
 *
 * ccx_nstep_push(ring_steps, ring_state, K, env_flags u8 [K][E], cut).  Enqueued directly BEHIND a ccx_replay_push of the same
 * K steps into the same ring: with head' = ring_state[0] (which that push advanced by K) read on the device,
 *     cut[((head' - K + s) mod S) * E + e] = (env_flags[s][e] & (CCX_EF_ALL_TERMINATED | CCX_EF_ALL_TRUNCATED | CCX_EF_RESET)) ? 1 : 0
 * for s = 0 .. K - 1, e = 0 .. E - 1.  (head' - K < 0, a caller that pushed nothing, counts as 0, as in ccx_prio_push: the
 * stores stay inside cut.)
 *
 * ccx_nstep_mark_cut(ring_steps, ring_state, env_mask u8 [E] or NULL, cut).  cut = 1 at the newest ring step, (head - 1) mod S,
 * for the envs whose mask byte is not zero (NULL: all envs); nothing while head == 0.  For a caller that restarts envs between
 * two pushes by hand (ccx_reset and its kin): the library cannot see that.
 *
 * ccx_nstep_fetch.  The ring of ccx_replay_fetch, cut, n with 1 <= n <= min(S, CCX_NSTEP_MAX), gamma finite in [0, 1], and
 * index i64 [B].  Outputs: those of ccx_replay_fetch, and discount f32 [B][N] and span u8 [B][N]; every element of every
 * output given is written.  For b with i = index[b] in [0, R): p = i / E, e = i % E, slot_k = ((p + k) mod S) * E + e, and
 * head = ring_state[0] read on the device:
 *     avail = head == 0 ? 0 : (head < S && p >= head) ? 0 : (head - 1 - p) mod S        (non-negative: successors that exist)
 *     m_env = 1;  while (m_env < n && m_env <= avail && cut[slot_{m_env-1}] == 0) ++m_env;                    (per record)
 *   per agent a:
 *     m_a = 1;  while (m_a < m_env && done[slot_{m_a-1}][a] == 0 && valid[slot_{m_a}][a] != 0) ++m_a;
 *     g = 1.0 (f64);  G = reward[slot_0][a];
 *     for k = 1 .. m_a - 1:  g = g * (double)gamma;  t = g * reward[slot_k][a];  G = G + t;   (three f64 operations, k ascending)
 *     g = g * (double)gamma;  discount = (float)g;  span = m_a;
 *     done_out  = done[slot_{m_a-1}][a];
 *     dropped   = m_a < m_env && done_out == 0;
 *     valid_out = dropped ? 0 : valid[slot_0][a];
 *     reward_out = G;   actions, index and the obs rows: record slot_0, as ccx_replay_fetch
 *     next_obs rows and masks_next: record slot_{m_env-1}
 * A dropped row is an agent that stopped being live inside the env's window without terminating and without an env cut --
 * only a user truncation class can do that; the env's next state is then not this agent's bootstrap state, so the row is
 * left out (valid 0), not given a wrong target.  next_obs and masks_next are env-level: the state every bootstrapping agent
 * of the record continues from.  A reward beyond m_a reaches no result; a NaN inside the window goes through loudly.  An
 * index outside [0, R) gives the EMPTY record of CCX_REPLAY with discount = (float)(double)gamma = gamma and span = 1, and
 * reads nothing.  Every slot_k is reduced mod S (p < S and k < n <= S: one conditional subtraction), so NO access can leave
 * the arrays, whatever head, cut or index hold.  With n == 1 every output shared with ccx_replay_fetch has its bits,
 * discount is gamma everywhere and span is 1.
 *
 * ccx_nstep_sample is the same kernel drawing its own indices by exactly ccx_replay_sample's draw: the same stream constant,
 * the same key (b, draws), F = min(head, S) * E, draws = ring_state[1], and then draws += 1 -- for equal state it names the
 * records ccx_replay_sample names.
 *
 * ccx_td_loss_discounted / ccx_td_loss_discounted_backward: ccx_td_loss / ccx_td_loss_backward with discount f32 [M] (device,
 * 4-byte aligned) in the place of gamma.  The per-row rule is CCX_QLEARN's, unchanged, with discount[i] where it says gamma:
 * step 4 is nb = (done[i] || discount[i] == 0.0f) ? +0.0f : discount[i] * boot.  The tree, stats, td_error, the backward and
 * the NULL combinations are the same; a discount array filled with one value gives the bits of ccx_td_loss at that gamma.
 * The values are the caller's: they are not range-checked.
 *
 * Launches: ccx_nstep_push ONE kernel, ccx_nstep_mark_cut ONE, ccx_nstep_fetch ONE, ccx_nstep_sample TWO (the fetch and one
 * plain lane behind it that advances draws); ccx_td_loss_discounted TWO, its backward ONE.  No host synchronisation, no
 * allocation; everything captures into a HIP graph and advances with every replay.  In the fetch no successor address depends
 * on loaded data: the loads of cut, done, valid and reward of all n records are in flight together, and the one dependent
 * load is next_c / masks_next of record m_env - 1.  A NULL handle or required pointer, S < 1 or S E >= 2^31, K outside 1..S,
 * n outside 1..min(S, 16), gamma not finite or outside [0, 1], B outside 1..2^31 / N, a misaligned array: CCX_EINVAL with a
 * ccx_last_error message, before any launch.  Not here: n above 16, a per-agent next state for dropped rows,
 * lambda-returns or Retrace, n-step inside the actor, sequences, rings across GPUs, bf16 / f16.
 */
#define CCX_NSTEP_MAX 16
int ccx_nstep_push(ccx_handle* h, int64_t ring_steps, const int64_t* ring_state /* [4] */, int64_t K,
                   const uint8_t* env_flags /* [K][E] */, uint8_t* cut /* [R] */);
int ccx_nstep_mark_cut(ccx_handle* h, int64_t ring_steps, const int64_t* ring_state /* [4] */,
                       const uint8_t* env_mask_or_null /* [E] */, uint8_t* cut /* [R] */);
int ccx_nstep_sample(ccx_handle* h, int64_t ring_steps, float* ring_obs_c, float* ring_next_c, uint8_t* ring_actions,
                     double* ring_reward, uint8_t* ring_done, uint8_t* ring_valid, uint8_t* ring_masks_next, int64_t* ring_state,
                     const uint8_t* cut /* [R] */, int32_t n, float gamma, int64_t batch, float* obs_or_null /* [B][N][L] */,
                     float* next_obs_or_null /* [B][N][L] */, uint8_t* actions /* [B][N] */, double* reward /* [B][N] */,
                     uint8_t* done /* [B][N] */, uint8_t* valid /* [B][N] */, uint8_t* masks_next /* [B][N] */,
                     int64_t* index /* [B] */, float* discount /* [B][N] */, uint8_t* span /* [B][N] */);
int ccx_nstep_fetch(ccx_handle* h, int64_t ring_steps, float* ring_obs_c, float* ring_next_c, uint8_t* ring_actions,
                    double* ring_reward, uint8_t* ring_done, uint8_t* ring_valid, uint8_t* ring_masks_next, int64_t* ring_state,
                    const uint8_t* cut /* [R] */, int32_t n, float gamma, int64_t batch, const int64_t* index_in /* [B] */,
                    float* obs_or_null, float* next_obs_or_null, uint8_t* actions, double* reward, uint8_t* done, uint8_t* valid,
                    uint8_t* masks_next, int64_t* index, float* discount, uint8_t* span);
int ccx_td_loss_discounted(ccx_handle* h, int64_t rows, const float* q /* [M][5] */, const uint8_t* actions /* [M] */,
                           const double* reward /* [M] */, const uint8_t* done /* [M] */, const float* q_next_target /* [M][5] */,
                           const float* q_next_online_or_null /* [M][5] */, const uint8_t* masks_next_or_null /* [M] */,
                           const uint8_t* valid_or_null /* [M] */, const float* weights_or_null /* [M] */,
                           const float* discount /* [M] */, float huber_delta, void* workspace, float* stats /* [8] */,
                           float* td_error_or_null /* [M] */);
int ccx_td_loss_discounted_backward(ccx_handle* h, int64_t rows, const float* q /* [M][5] */, const uint8_t* actions /* [M] */,
                                    const double* reward /* [M] */, const uint8_t* done /* [M] */,
                                    const float* q_next_target /* [M][5] */, const float* q_next_online_or_null /* [M][5] */,
                                    const uint8_t* masks_next_or_null /* [M] */, const uint8_t* valid_or_null /* [M] */,
                                    const float* weights_or_null /* [M] */, const float* discount /* [M] */, float huber_delta,
                                    const float* stats /* [8] */, const float* grad_loss_or_null /* [1] */,
                                    float* grad_q /* [M][5] */);
/*
 * CCX_DUELING: the dueling combine of a Q-head, forward and backward, and the head's forward fused with ccx_q_actions' choice
 * (the DQN actor step in ONE launch, as ccx_mlp_sample_actions is PPO's).  A dueling head is an ordinary CCX_MLP / CCX_SIDES
 * head with O = 6: a row of its output is va f32 [6], va[k] for k = 0..4 the advantage of action k (index = action id, as
 * everywhere), va[5] the state value.  The discipline is CCX_QLEARN's: every line below is ONE correctly rounded f32
 * operation, nothing is fused, `/` is the correctly rounded division.
 *     forward:   s = (((va0 + va1) + va2) + va3) + va4;   mean = s / 5.0f;
 *                c_k = va_k - mean;   q_k = va5 + c_k                      (k = 0..4)
 *     backward:  t = (((g0 + g1) + g2) + g3) + g4;   gm = t / 5.0f;
 *                grad_va_k = g_k - gm   (k = 0..4);   grad_va_5 = t
 * The mean runs over ALL five actions whatever the state's mask says: the combine is a property of the network, the mask a
 * property of the state (it enters where an action is chosen).  The backward is a pure function of grad_q: it reads neither
 * va nor q.  A row whose grad_q is five +0.0 gets six +0.0 -- what ccx_td_loss_backward writes at rows that do not count
 * stays exactly +0.0 through the combine, whatever va holds there.  A NaN in a row's advantages reaches all five of its
 * Q-values; nothing crosses rows.
 *
 * ccx_dueling_forward: num in 1..4 arrays of equal row count in ONE launch -- va and q are HOST arrays of num device
 * pointers, f32 [rows][6] and f32 [rows][5]; the table travels by value in the kernel arguments, so the call captures (an
 * update combines q, q_next_target and q_next_online in one node).  ccx_dueling_backward: grad_q f32 [rows][5] to grad_va f32
 * [rows][6], ONE launch.  Pure functions of their arrays: the handle supplies device and stream only.  Every element of
 * every output is written; all arrays are 16-byte aligned (rows travel in whole 16-byte pieces).
 *
 * ccx_mlp_q_actions / ccx_sides_q_actions: ccx_mlp_sample_actions / ccx_sides_sample_actions with the Q choice in the place
 * of the softmax draw, ONE launch.  O = 5: a plain head; O = 6: a dueling head.  By definition
 *     ccx_mlp_q_actions(head, obs, ..) == ccx_q_actions(O == 6 ? dueling(head(obs)) : head(obs), ..)
 * -- the same key, the same two streams, the same rule for dead slots, the same bits in actions, explored and q;
 * ccx_sides_q_actions likewise, per group.  q f32 [E][N][5] or NULL receives the COMBINED values of every slot, dead ones
 * included.  masks, epsilon (device f32 [1], NULL = greedy), actions and explored are ccx_q_actions'.  In
 * ccx_sides_q_actions a slot that no group owns gets action CCX_ACTION_ABSENT and explored 0; its q elements are not
 * written and it runs no layer.  obs is 16-byte aligned, the other float arrays 4-byte aligned.
 *
 * Against IEEE f64 (measured on the CPU, tests/test_dueling_spec.py, maxima doubled), as max |err| / max(1, |f64 value|)
 * against the textbook composition in torch f64 on the same f32 inputs (v + a - a.mean(-1), autograd of a random cotangent),
 * advantages ~ N(0, 1) * 10^U(-3, 3), a third of the rows with a common offset of ten times their scale: q within 9.6e-04,
 * grad_va within 1.3e-04.  Both figures are the cancellation in va_k - mean and in the sums where a row's entries are large
 * against the result: the error of f32 inputs this large, not of the order of the operations.
 *
 * No host synchronisation, no allocation; everything captures into a HIP graph.  Offsets are 64-bit.  A NULL handle or
 * required pointer, rows < 1, num outside 1..4, a misaligned pointer, a grid beyond 2^31 - 1 workgroups, O other than 5 or 6,
 * a shape CCX_MLP refuses: CCX_EINVAL with a ccx_last_error message, before any launch.  Not here: dueling inside
 * ccx_td_loss or inside the tile's epilogue for the learner, a masked mean or a max-combine, noisy heads (distributional
 * heads are CCX_C51; dueling combined with them is not here),
 * different (H, activation, O) per group, bf16 / f16.
 */
int ccx_dueling_forward(ccx_handle* h, int64_t rows, int32_t num /* 1..4 */,
                        const float* const* va /* host [num] of device [rows][6] */,
                        float* const* q /* host [num] of device [rows][5] */);
int ccx_dueling_backward(ccx_handle* h, int64_t rows, const float* grad_q /* [rows][5] */, float* grad_va /* [rows][6] */);
int ccx_mlp_q_actions(ccx_handle* h, int32_t H, int32_t activation, int32_t O /* 5: plain, 6: dueling */,
                      const float* obs /* [E][N][ccx_obs_len(N)] */, const float* w1t, const float* b1, const float* w2,
                      const float* b2, const uint8_t* masks_or_null /* [E][N] */,
                      const float* epsilon_or_null /* device f32 [1]; NULL = greedy */, uint8_t* actions /* [E][N] */,
                      uint8_t* explored_or_null /* [E][N] */, float* q_or_null /* [E][N][5], the COMBINED values */);
int ccx_sides_q_actions(ccx_handle* h, int32_t H, int32_t activation, int32_t O, const float* obs /* [E][N][ccx_obs_len(N)] */,
                        int32_t num_groups, const ccx_slot_group* groups, const uint8_t* masks_or_null /* [E][N] */,
                        const float* epsilon_or_null, uint8_t* actions /* [E][N] */, uint8_t* explored_or_null /* [E][N] */,
                        float* q_or_null /* [E][N][5] */);
/*
 * CCX_MINIBATCH: shuffled on-policy minibatches out of a rollout's own arrays -- sampling WITHOUT replacement.  ONE kernel
 * draws B positions of a keyed permutation of the rollout's records, gathers the records they name and writes the minibatch
 * ccx_ppo_loss takes (ccx_minibatch_next; ccx_minibatch_fetch is the same kernel on the caller's record indices).  The
 * permutation is never materialised: any lane computes pi_c(p) from p alone.  Everything is integer work and copies: every
 * output is bit-defined.
 *
 * Records.  A rollout of K steps of the handle's E envs gives M = K E records, 1 <= M < 2^31; record j = s E + e, step-major
 * like the ring of CCX_REPLAY.
 *
 * The permutation pi_c of [0, M) of epoch c (u64): a keyed, unbalanced Feistel network with cycle walking.  w = the smallest
 * integer >= 2 with 2^w >= M, a = floor(w / 2), b = w - a; x = L 2^b + R with R of b bits.  Six rounds r = 0 .. 5, with wl the
 * current width of L (a at the start):
 *     (L, R) <- (R, L ^ (word(seed_lo, seed_hi ^ 0x1B873593; R, (u32)c, (u32)(c >> 32), r) & (2^wl - 1)));   wl <- w - wl
 * (the k of ccx_set_rng_seed's formula, its four key slots in that order); after six rounds the widths are (a, b) again and
 * x' = L 2^b + R.  Cycle walk: the six rounds are repeated while x' >= M; then pi_c(p) = x'.  Every round is invertible, so
 * the walk ends for every key and every M; 2^w < 2 M, so a step of it succeeds with probability above 1 / 2.  The key holds
 * neither env nor shard.  The stream constant differs from 0, 0x5BD1E995, 0x2545F491, 0x68E31DA4, 0xB5297A4D, 0x3C6EF372 and
 * 0x7F4A7C15.  ccx_minibatch_permutation writes pi_epoch(0 .. M - 1) to out i64 [M].
 *
 * ccx_minibatch_next.  state i64 [4] = {epoch, cursor, 0, 0} lives on the device and is READ THERE when the kernel runs.  For
 * b = 0 .. B - 1 (1 <= B <= 2^31 / N), with p = cursor + b:
 *     index[b] = (cursor >= 0 && p < M) ? pi_epoch(p) : -1
 * and then
 *     if (cursor < 0 || cursor + B >= M) { epoch += 1; cursor = 0; } else cursor += B;
 * An epoch is ceil(M / B) draws; the last one is padded with EMPTY rows when B does not divide M; every record of [0, M)
 * appears exactly once per epoch.  Whatever state holds, no address outside the source arrays is formed: a stale or junk
 * state yields EMPTY rows or records in range.  ccx_minibatch_fetch takes index_in i64 [B] from the caller instead (and writes
 * it to the index output, which may be the same array) and leaves state alone.
 *
 * Gather (both).  Row b of every output is a copy of the fields of record index[b], bit for bit, and every element of every
 * output given is written.  With (s, e) = (j / E, j mod E):
 *   out_obs f32 [B][N][ccx_obs_len(N)] (may be NULL) from obs_steps and obs0, in one of two forms chosen by `compact`:
 *     compact == 0: obs_steps f32 [K][E][N][L], obs0 f32 [E][N][L] or NULL -- DefaultObservation rows, copied;
 *     compact != 0: obs_steps f32 [K][E][N][4], obs0 f32 [E][N][4] or NULL -- CCX_OBS_COMPACT records, expanded with the
 *                   handle's row constants: the very gather of ccx_observe, hence the bits of ccx_expand_observations.
 *   With obs0 given the row is the one the step ACTED ON, s == 0 ? obs0[e] : obs_steps[s - 1][e] (CCX_REPLAY's obs_c rule; the
 *   caller's contract is again a rollout made with CCX_RESET_OBS_NEXT).  With obs0 NULL it is obs_steps[s][e]: the caller's
 *   array already holds the rows acted on.
 *   actions u8, logp f32, advantages f32, returns f32, each [K][E][N] -> [B][N]; masks u8 and valid u8 likewise, where either
 *   SOURCE may be NULL: the output is then 0x1F, respectively CCX_AF_LIVE (4), for every record in range.  index i64 [B].
 *   The EMPTY row, where index[b] is outside [0, M): action CCX_ACTION_ABSENT, logp = advantages = returns = +0.0, masks 0x10,
 *   valid 0, and the observation rows of compact records of +0.0 (as CCX_REPLAY defines them).  valid = 0 takes the padding
 *   out of ccx_ppo_loss without a change of shape.
 *
 * Launches: ccx_minibatch_next enqueues TWO kernels on the handle's stream -- the gather, and one plain lane behind it that
 * advances the state, so the update cannot race with the lanes that read the old value (no atomic, no host synchronisation);
 * ccx_minibatch_fetch and ccx_minibatch_permutation ONE.  No allocation; everything captures into a HIP graph, and a captured
 * ccx_minibatch_next advances with every replay.  Offsets are 64-bit.  A NULL handle or required pointer, K E outside
 * 1 .. 2^31 - 1, B outside 1 .. 2^31 / N, out_obs given without obs_steps, an observation-row array that is not 16-byte aligned
 * (8-byte for an odd number of agents, as for ccx_step), a compact array that is not 16-byte aligned, an i64 array that is not
 * 8-byte aligned, an f32 array that is not 4-byte aligned: CCX_EINVAL with a ccx_last_error message, before any launch.
 * Not here: old values for a clipped value loss, sequences for recurrent policies, a shuffle across GPUs (each shard shuffles
 * its own records), stratification by env, bf16 / f16.
 */
int ccx_minibatch_next(ccx_handle* h, int64_t K, int32_t compact, const float* obs0_or_null, const float* obs_steps_or_null,
                       const uint8_t* actions /* [K][E][N] */, const float* logp /* [K][E][N] */,
                       const float* advantages /* [K][E][N] */, const float* returns /* [K][E][N] */,
                       const uint8_t* masks_or_null /* [K][E][N] */, const uint8_t* valid_or_null /* [K][E][N] */,
                       int64_t* state /* [4] */, int64_t batch, float* out_obs_or_null /* [B][N][L] */,
                       uint8_t* out_actions /* [B][N] */, float* out_logp /* [B][N] */, float* out_advantages /* [B][N] */,
                       float* out_returns /* [B][N] */, uint8_t* out_masks /* [B][N] */, uint8_t* out_valid /* [B][N] */,
                       int64_t* out_index /* [B] */);
int ccx_minibatch_fetch(ccx_handle* h, int64_t K, int32_t compact, const float* obs0_or_null, const float* obs_steps_or_null,
                        const uint8_t* actions, const float* logp, const float* advantages, const float* returns,
                        const uint8_t* masks_or_null, const uint8_t* valid_or_null, int64_t batch,
                        const int64_t* index_in /* [B] */, float* out_obs_or_null, uint8_t* out_actions, float* out_logp,
                        float* out_advantages, float* out_returns, uint8_t* out_masks, uint8_t* out_valid, int64_t* out_index);
int ccx_minibatch_permutation(ccx_handle* h, int64_t M, int64_t epoch, int64_t* out /* [M] */);
/*
 * CCX_C51: categorical (C51) Q-heads -- the expected values of a network's atom logits (what ccx_q_actions chooses from), the
 * projection of the bootstrapped target distribution onto the support, the cross-entropy loss with its means over the rows
 * that count, and its gradient with respect to the logits.  The textbook projection is floor / ceil and two scatter-adds,
 * which on a GPU are floating-point atomics in no fixed order; here it is a gather with a written order of additions, so
 * every output is bit-defined, the reduction included.  The discipline is CCX_QLEARN's, unchanged: every f32 operation named
 * below is ONE correctly rounded f32 operation (+ - * /), nothing is fused, nothing is reassociated, subnormals are kept;
 * what a rule does not read is SELECTED away, never multiplied by zero.
 *
 * A = atoms, 2 <= A <= 64;  vmin < vmax finite f32;  dz = (vmax - vmin) / (float)(A - 1);  z_j = vmin + (float)j * dz;
 * top = (float)(A - 1).  Logits are f32 [M][5][A] (action id, then atom), contiguous, and need only the alignment of an f32,
 * 4 bytes: A = 51 gives rows of 204 bytes, so nothing wider is assumed anywhere.  butterfly(v) is the halving of
 * CCX_PPO_LOSS's groups over 64 places in f32: for o = 32, 16, .. 1 every place j takes v_j + v_(j ^ o); places j >= A hold
 * +0.0f.  exp_spec and log_spec are CCX_SAMPLE's (log_spec over [1, 64]: within 2.6e-7 absolute of f64 log, measured on the
 * CPU over 2e6 points).
 *   1. The distribution of one (row, action) with logits l_0 .. l_(A-1).  mx = their maximum by the same butterfly with
 *      max2(a, b) = fmax(a, b) with a zero of either sign made +0.0f (a NaN beside a number gives the number; exact and the
 *      same bits in any order).  d_j = l_j - mx;  u_j = d_j - d_j (+0.0f for a finite d_j, NaN otherwise);
 *      e_j = d_j >= -80 ? exp_spec(d_j) : u_j;  S = butterfly(e).  So a logit far below the maximum weighs exactly +0.0f, and
 *      a NaN, a +inf or a -inf logit makes S a NaN: every logit that is read must be finite, and one that is not is loud.
 *      log S is log_spec(S), or S itself where S is a NaN.
 *   2. The expected value Q = butterfly(e_j * z_j) / S: the products are summed, ONE division.  ccx_c51_q_values and the
 *      bootstrap choice of step 3 run the same function.
 *   3. Bootstrap (only where step 4 does not cut the target): Q_sel,k = the expected values of next_online[i][k] if given
 *      (double-Q), else of next_target[i][k];  k* = greedy(Q_sel, m') of CCX_QLEARN with m' = CCX_SAMPLE step 2 on
 *      masks_next;  p_j = e_j / S of next_target[i][k*].  A NaN expected value never wins.
 *   4. Projection.  r = (float)reward[i] (one rounding);  disc = discount ? discount[i] : gamma;  cut = done[i] ||
 *      disc == 0.0f.  A cut target reads no next-state array: p_0 = 1.0f, p_j = +0.0f (j > 0), the point mass at r.
 *      t_j = cut ? r : r + disc * z_j;  u = t_j - t_j;  b0 = (t_j - vmin) / dz;  b1 = b0 < 0 ? u : b0;
 *      b_j = b1 > top ? top + u : b1      (two selects; u is +0.0f for a finite t_j, so a finite target is limited to
 *      [0, top], while an infinite or NaN reward or discount gives a NaN, not an edge atom);
 *      w_ij = (1.0f - |b_j - (float)i|) < 0 ? +0.0f : that value      (max(+0.0f, .) as a select a NaN passes);
 *      m_i = sum over j = 0 .. A - 1 ascending of p_j * w_ij, onto +0.0f.
 *      Adding the exact zeros of the far atoms changes no bit: this is the floor / ceil scatter with its additions in
 *      ascending j.
 *   5. Loss of the row, on the distribution of logits[i][a] (step 1):  logp_i = d_i - log S;
 *      ce = 0.0f - butterfly(m_i != 0 ? m_i * logp_i : +0.0f);  term = weights ? weights[i] * ce : ce;
 *      qa = its expected value (step 2);  y = butterfly(m_i * z_i).
 *   6. Which rows count and which are tallied as bad is CCX_QLEARN step 1, verbatim.  A row that does not count contributes
 *      to no sum, reads no logits, and gets +0.0f in row_loss, in its A elements of proj and in every gradient, whatever its
 *      inputs hold.  Six sums -- 1, term, ce, qa, y over the rows that count, 1 over the bad rows -- in f64 by the tree of
 *      CCX_PPO_LOSS, unchanged.  stats = {S_term / n, S_ce / n, S_qa / n, S_y / n, +0.0f, +0.0f, (float)n, (float)bad};
 *      n == 0: the first six are +0.0f.  row_loss[i] = counts ? ce : +0.0f (unweighted, >= 0: what CCX_PRIO takes as
 *      td_error);  proj[i][.] = counts ? m : +0.0f.
 *   7. Backward: a pure function of logits, actions, proj (the target is a constant), valid, weights, stats, grad_loss.
 *      g = grad_loss ? grad_loss[0] : 1.0f;  sc = g / stats[6], made once;  gw = weights ? sc * weights[i] : sc;
 *      Msum = butterfly(m);  grad_logits[i][a][j] = gw * ((e_j / S) * Msum - m_j), e and S of logits[i][a].
 *      The other four actions of the row, rows that do not count, and stats[6] == 0 give exactly +0.0f.  Every element is
 *      written.
 * A non-finite logit (of logits[i][a], of next_target[i][k*]), reward or discount of a row that counts reaches row_loss and
 * the loss as a NaN or an infinity.  A non-finite logit of an action the bootstrap does not choose is CCX_QLEARN's case: its
 * NaN expected value never wins and reaches no result.
 *
 * Against IEEE f64 (measured on the CPU, tests/test_c51_spec.py, maxima doubled), as max |err| / max(1, |f64 value|) against
 * the textbook composition in torch f64 on the same f32 inputs (softmax, expected values, masked argmax, floor / ceil
 * projection with index_add_, cross-entropy averaged over the rows that count, autograd), logits ~ N(0, 2^2), support
 * [-10, 10], A in {2, 3, 33, 51, 64}: proj within 1.3e-05, loss within 1.1e-07, row_loss within 1.6e-05, q within 2.1e-06,
 * grad_logits (times n) within 1.6e-05 (rows whose two best legal expected next-values lie within 1e-4 of each other may
 * choose another k* than f64 and are left out: under 0.5 %, asserted).  The projection's figure is ulp(b) at b near A - 1, a
 * property of f32 positions on the support; row_loss and the gradient inherit it times |log p|.
 *
 * Launches: ccx_c51_q_values ONE kernel on the handle's stream, ccx_c51_loss TWO (block partials, then one final wave; no
 * atomic, no last-block-done counter), ccx_c51_loss_backward ONE.  No host synchronisation, no allocation: the caller owns
 * the workspace (ccx_c51_workspace_bytes(rows) bytes, 8-byte aligned; 0 for rows < 1).  Everything captures into a HIP
 * graph.  Offsets are 64-bit.  q is f32 [M][5], 16-byte aligned (what ccx_q_actions takes); reward f64 and the workspace
 * are 8-byte aligned; every other f32 array 4-byte aligned.  A NULL handle or a NULL required pointer, rows < 1 (or so many
 * that a grid would pass 2^31 - 1 workgroups), atoms outside 2 .. 64, a vmin or vmax that is not finite, vmin >= vmax, a
 * spacing that is not finite or not above zero, a gamma that is not finite or lies outside [0, 1] when discount is NULL
 * (with discount given gamma is not read), a misaligned pointer: CCX_EINVAL with a ccx_last_error message, before any launch.
 * The feature draws nothing: actions come from ccx_q_actions on the expected values.  (A device network with 5 A outputs
 * is CCX_MLP_WIDE.)  Not here: the obs -> action fusion for categorical heads, quantile (QR-DQN / IQN) heads, noisy layers, dueling combined
 * with categorical heads, more than 64 atoms, bf16 / f16, the vector and RLlib adapters.
 */
int64_t ccx_c51_workspace_bytes(int64_t rows);
int ccx_c51_q_values(ccx_handle* h, int64_t rows, int32_t atoms, float vmin, float vmax, const float* logits /* [M][5][A] */,
                     float* q /* [M][5] */);
int ccx_c51_loss(ccx_handle* h, int64_t rows, int32_t atoms, float vmin, float vmax, const float* logits /* [M][5][A] */,
                 const uint8_t* actions /* [M] */, const double* reward /* [M] */, const uint8_t* done /* [M] */,
                 const float* next_target /* [M][5][A] */, const float* next_online_or_null /* [M][5][A] */,
                 const uint8_t* masks_next_or_null /* [M] */, const uint8_t* valid_or_null /* [M] */,
                 const float* weights_or_null /* [M] */, const float* discount_or_null /* [M] */, float gamma, void* workspace,
                 float* stats /* [8] */, float* row_loss_or_null /* [M]: ce, unweighted */, float* proj /* [M][A] */);
int ccx_c51_loss_backward(ccx_handle* h, int64_t rows, int32_t atoms, const float* logits /* [M][5][A] */,
                          const uint8_t* actions /* [M] */, const float* proj /* [M][A] */, const uint8_t* valid_or_null /* [M] */,
                          const float* weights_or_null /* [M] */, const float* stats /* [8] */,
                          const float* grad_loss_or_null /* [1] */, float* grad_logits /* [M][5][A] */);
/*
 * CCX_MLP_WIDE: CCX_MLP with up to 320 outputs -- the [5][A] atom logits of a categorical head (CCX_C51: 255 at A = 51, 320
 * at A = 64) from the observation rows, and the parameter gradients from the gradient of those logits.  The rule is
 * CCX_MLP's, forward and backward, word for word, with 1 <= O <= 320 in the place of 1 <= O <= 8: the layer-1 chain over k,
 * the activations, the layer-2 partials over groups of 16 hidden units added in group order onto b2[o]; the gh chain over
 * o = 0 .. O-1 ascending, ga, the f64 terms, the chains over blocks of 256 rows and CCX_PPO_LOSS's final step.  The limits
 * on L, H and activation, the layouts (y f32 [rows][O], grad_y f32 [rows][O], w2 and grad_w2 f32 [O][H], b2 and grad_b2
 * f32 [O]), the alignment demands (x, hidden and grad_a 16 bytes, the workspace 8, every other f32 array 4: a row of y or
 * grad_y is 4 O bytes, 1020 at A = 51, and may start at any multiple of 4), the 64-bit offsets, the written-every-element
 * rule and the refusals are CCX_MLP's as well.  So for O <= 8 the entry points below give the bits of ccx_mlp_forward and
 * ccx_mlp_backward on the same arrays, and a row's outputs depend on nothing but the row and the parameters.
 *
 * What differs is inside: ccx_mlp_wide_forward is ONE kernel that runs layer 2 over chunks of consecutive outputs,
 * ccx_mlp_wide_backward TWO plain launches (block partials with w2 streamed in slabs of consecutive o -- the order of the
 * gh chain is the slabs' order --, then CCX_MLP's final step; no floating-point atomic, no last-block-done counter).  Both
 * enqueue on the handle's stream only, neither allocates nor synchronises, both capture into a HIP graph.
 * ccx_mlp_wide_backward_workspace_bytes(rows, L, H, O) = B * (L * H + H + O * H + O) * 8 bytes with B = ceil(rows / 256)
 * (0 for rows < 1 or a shape outside the limits).  A shape outside the limits is CCX_EINVAL with a ccx_last_error message
 * that names L, H, O and activation, before any launch; ccx_mlp_forward / ccx_mlp_backward / CCX_SIDES / ccx_mlp_q_actions
 * keep their own limit of 8.
 * Against IEEE f64 (measured on the CPU, tests/test_mlp_wide_spec.py, maxima doubled; the compositions and the measure
 * are CCX_MLP's), L = 38, H = 64, O = 255, torch.nn.Linear's initial weights, observation-like rows, tanh and relu, M = 20 000: the logits
 * within 4.8e-6 absolute; grad_w1t within 5.3e-4, grad_b1 1.1e-4, grad_w2 1.2e-7, grad_b2 1.14e-7 (gh sums 255 terms of a
 * standard-normal grad_y here, 5 there: the first two figures grow with it).
 *
 * Not here: the fusion of obs -> head -> expected values -> epsilon-greedy action into one launch, wide heads in CCX_SIDES
 * or CCX_DUELING, more than 320 outputs, a second hidden layer under a wide output (CCX_MLP_DEEP has two hidden layers and O <= 8), a
 * bit-defined gradient with respect to x, matrix-core (MFMA)
 * arithmetic -- the rule is a chain of f32 operations --, bf16 / f16.
 */
int ccx_mlp_wide_forward(ccx_handle* h, int64_t rows, int32_t L, int32_t H, int32_t O, int32_t activation,
                         const float* x /* [rows][L] */, const float* w1t /* [L][H] */, const float* b1 /* [H] */,
                         const float* w2 /* [O][H] */, const float* b2 /* [O] */, float* y /* [rows][O] */,
                         float* hidden_or_null /* [rows][H] */);
int64_t ccx_mlp_wide_backward_workspace_bytes(int64_t rows, int32_t L, int32_t H, int32_t O);
int ccx_mlp_wide_backward(ccx_handle* h, int64_t rows, int32_t L, int32_t H, int32_t O, int32_t activation,
                          const float* x /* [rows][L] */, const float* hidden /* [rows][H] */, const float* grad_y /* [rows][O] */,
                          const float* w2 /* [O][H] */, void* workspace, float* grad_w1t /* [L][H] */, float* grad_b1 /* [H] */,
                          float* grad_w2 /* [O][H] */, float* grad_b2 /* [O] */, float* grad_a_or_null /* [rows][H] */);
/*
 * CCX_MLP_DEEP: CCX_MLP with a second hidden layer -- Linear(L, H1) -> act -> Linear(H1, H2) -> act -> Linear(H2, O), one
 * activation for both hidden layers: the fully connected net of two hidden layers that RLlib trains by default and the
 * usual 64-64 tanh PPO baseline -- forward in ONE kernel, fused with CCX_SAMPLE and with ccx_q_actions' choice in ONE kernel
 * each, and the six parameter gradients bit-defined.  What CCX_MLP promises holds word for word: the outputs of a row depend
 * on (L, H1, H2, O, activation), the row and the parameters only, never on the number of rows, the row's index, the launch
 * shape or the entry point.
 *
 * Parameters (device pointers): w1t f32 [L][H1] (input-major, as CCX_MLP's), b1 f32 [H1], w2t f32 [H1][H2] (input-major:
 * torch.nn.Linear(H1, H2).weight.t().contiguous()), b2 f32 [H2], w3 f32 [O][H2] (torch's layout), b3 f32 [O].  Limits:
 * 1 <= L <= 512; H1 and H2 each a multiple of 16 in 16..256 (they need not be equal); 1 <= O <= 8; activation 0 = tanh,
 * 1 = relu.  The discipline is CCX_MLP's: IEEE binary32, every operation named ONE correctly rounded operation, no fma, no
 * reassociation, subnormals kept, the sign and payload of a NaN left open.
 *
 * Forward, for every row on its own:
 *   1. h1[0 .. H1-1]: CCX_MLP's steps 1 and 2 on x with (w1t, b1).
 *   2. layer 2, for every unit j of H2: a = b2[j]; for k = 0 .. H1-1 in this order a = a + h1[k] * w2t[k][j]; h2[j] = act(a)
 *      (CCX_MLP's layer-1 chain with h1 in the place of x).
 *   3. the output layer: CCX_MLP's step 3 on h2 with (w3, b3) -- the partials over groups of 16 units of H2, added in group
 *      order onto b3[o].
 * So by definition
 *     deep(x) == ccx_mlp_forward(L := H1, H := H2, O; x := h1, w1t := w2t, b1 := b2, w2 := w3, b2 := b3)
 * where h1 is the `hidden` that ccx_mlp_forward writes for (x, w1t, b1) (with any w2, b2): hidden1 is that h1, hidden2 the
 * `hidden` of the second call, y its y, bit for bit.
 *
 * Backward (ccx_mlp_deep_backward).  Inputs: x f32 [M][L], hidden1 f32 [M][H1], hidden2 f32 [M][H2] (what the forward wrote),
 * grad_y f32 [M][O], w2t, w3, activation.  Per row r, in f32:
 *   - gh2 and ga2[r][0 .. H2-1]: CCX_MLP's backward steps 1 and 2 with (grad_y, w3, hidden2).
 *   - for every unit i of H1: gh1 = ga2[r][0] * w2t[i][0]; then for j = 1 .. H2-1 in order gh1 = gh1 + ga2[r][j] * w2t[i][j].
 *   - ga1[r][i] from gh1 and hidden1[r][i] by step 2's activation rule.
 * Terms, each the f64 product of two f32 values (exact):
 *     grad_w1t[k][i] sums x[r][k] * ga1[r][i]             grad_b1[i] sums ga1[r][i]
 *     grad_w2t[i][j] sums hidden1[r][i] * ga2[r][j]       grad_b2[j] sums ga2[r][j]
 *     grad_w3[o][j]  sums grad_y[r][o] * hidden2[r][j]    grad_b3[o] sums grad_y[r][o]
 * The reduction over rows is CCX_MLP's, unchanged: blocks of 256 consecutive rows, ascending chains from +0.0, CCX_PPO_LOSS's
 * final step over the B = ceil(M / 256) partials, one rounding to f32; no floating-point atomic, no last-block-done counter.
 * grad_a1_or_null f32 [M][H1] and grad_a2_or_null f32 [M][H2] receive ga1 and ga2 of every row.  Two identities follow, and
 * the tests hold the kernels to them:
 *   - (grad_w2t, grad_b2, grad_w3, grad_b3, grad_a2) == ccx_mlp_backward(L := H1, H := H2, O; x := hidden1,
 *     hidden := hidden2, grad_y, w2 := w3): its grad_w1t is grad_w2t, its grad_b1 is grad_b2.
 *   - (grad_w1t, grad_b1, grad_a1) == ccx_mlp_wide_backward(L, H := H1, O := H2; x, hidden := hidden1, grad_y := grad_a2,
 *     w2 := w2t transposed to [H2][H1]).
 * Against IEEE f64 (measured on the CPU, tests/test_mlp_deep_spec.py, maxima doubled; the textbook composition in f64 on
 * the same f32 inputs, autograd for the gradients, the measure of CCX_MLP's backward), torch.nn.Linear's initial weights,
 * observation-like rows, the worse of tanh and relu, M = 20 000, L = 38, O = 5.  At 64-64: the logits within 1.74e-6
 * absolute; grad_w1t within 1.86e-4, grad_b1 6.0e-6, grad_w2t 4.1e-5, grad_b2 1.4e-6, grad_w3 1.0e-4, grad_b3 9.7e-8.  At
 * 256-256: the logits within 2.6e-6; grad_w1t 6.5e-3, grad_b1 5.0e-4, grad_w2t 1.43e-1, grad_b2 8.1e-3, grad_w3 1.57e-4,
 * grad_b3 9.7e-8 -- the first four of these are ONE relu unit of ONE row whose layer-2 pre-activation lies within f32
 * rounding of zero: the f64 side forms its own masks, takes the other branch there, and that row's whole term moves the
 * element (with tanh alone the same shape measures 3.11e-5, 2.03e-6, 8.82e-6, 3.75e-6).
 *
 * Entry points.  Each only enqueues on the handle's stream: no host synchronisation, no allocation, and it captures into a
 * HIP graph.  ccx_mlp_deep_forward is ONE kernel (hidden1 / hidden2 may be NULL).  ccx_mlp_deep_sample_actions is by
 * definition ccx_sample_actions applied to the deep head's logits (L = ccx_obs_len(N), O = 5) on obs [E][N][L], in ONE
 * kernel: ccx_mlp_sample_actions' key, dead-slot rule and optional logits output.  ccx_mlp_deep_q_actions is
 * ccx_mlp_q_actions with the deep head, in ONE kernel: O = 5 (plain) or 6 (dueling), the same epsilon, explored and draw.
 * ccx_mlp_deep_backward is THREE plain launches for every shape and every input (block partials, then CCX_MLP's final
 * kernel on each of two stretches of the workspace; a kernel boundary orders the partials).  The caller owns the workspace,
 * 8-byte aligned: ccx_mlp_deep_backward_workspace_bytes(rows, L, H1, H2, O) =
 * ceil(rows / 256) * (L * H1 + H1 + H1 * H2 + H2 + O * H2 + O) * 8 bytes (0 for rows < 1 or a shape outside the limits):
 * 1.3 GB at 524 288 rows of L = 38, H1 = H2 = 256, O = 5 (77 061 elements per block; 1.26 GB exactly; 114 MB at 64-64) -- it grows with
 * H1 * H2, so update in chunks of rows where that is too much.  A NULL handle or a NULL required pointer, rows < 1, a shape
 * outside the limits, x / obs, hidden1, hidden2, grad_a1 or grad_a2 not 16-byte aligned, a workspace not 8-byte aligned, or
 * any other f32 array not 4-byte aligned: CCX_EINVAL with a ccx_last_error message, before any launch.  Offsets are 64-bit.
 *
 * Not here: more than two hidden layers, deep heads in CCX_SIDES, wide outputs (O > 8) on deep heads, a bit-defined
 * gradient with respect to x, matrix-core (MFMA) arithmetic, bf16 / f16.
 */
int ccx_mlp_deep_forward(ccx_handle* h, int64_t rows, int32_t L, int32_t H1, int32_t H2, int32_t O, int32_t activation,
                         const float* x /* [rows][L] */, const float* w1t /* [L][H1] */, const float* b1 /* [H1] */,
                         const float* w2t /* [H1][H2] */, const float* b2 /* [H2] */, const float* w3 /* [O][H2] */,
                         const float* b3 /* [O] */, float* y /* [rows][O] */, float* hidden1_or_null /* [rows][H1] */,
                         float* hidden2_or_null /* [rows][H2] */);
int ccx_mlp_deep_sample_actions(ccx_handle* h, int32_t H1, int32_t H2, int32_t activation,
                                const float* obs /* [E][N][ccx_obs_len(N)] */, const float* w1t /* [L][H1] */,
                                const float* b1 /* [H1] */, const float* w2t /* [H1][H2] */, const float* b2 /* [H2] */,
                                const float* w3 /* [5][H2] */, const float* b3 /* [5] */, const uint8_t* masks_or_null /* [E][N] */,
                                int32_t deterministic, uint8_t* actions /* [E][N] */, float* logp_or_null /* [E][N] */,
                                float* entropy_or_null /* [E][N] */, float* logits_or_null /* [E][N][5] */);
int ccx_mlp_deep_q_actions(ccx_handle* h, int32_t H1, int32_t H2, int32_t activation, int32_t O /* 5: plain, 6: dueling */,
                           const float* obs /* [E][N][ccx_obs_len(N)] */, const float* w1t /* [L][H1] */, const float* b1 /* [H1] */,
                           const float* w2t /* [H1][H2] */, const float* b2 /* [H2] */, const float* w3 /* [O][H2] */,
                           const float* b3 /* [O] */, const uint8_t* masks_or_null /* [E][N] */,
                           const float* epsilon_or_null /* [1] */, uint8_t* actions /* [E][N] */,
                           uint8_t* explored_or_null /* [E][N] */, float* q_or_null /* [E][N][5] */);
int64_t ccx_mlp_deep_backward_workspace_bytes(int64_t rows, int32_t L, int32_t H1, int32_t H2, int32_t O);
int ccx_mlp_deep_backward(ccx_handle* h, int64_t rows, int32_t L, int32_t H1, int32_t H2, int32_t O, int32_t activation,
                          const float* x /* [rows][L] */, const float* hidden1 /* [rows][H1] */,
                          const float* hidden2 /* [rows][H2] */, const float* grad_y /* [rows][O] */,
                          const float* w2t /* [H1][H2] */, const float* w3 /* [O][H2] */, void* workspace,
                          float* grad_w1t /* [L][H1] */, float* grad_b1 /* [H1] */, float* grad_w2t /* [H1][H2] */,
                          float* grad_b2 /* [H2] */, float* grad_w3 /* [O][H2] */, float* grad_b3 /* [O] */,
                          float* grad_a1_or_null /* [rows][H1] */, float* grad_a2_or_null /* [rows][H2] */);
/*
 * CCX_POLICY_RANDOM: uniform random actions drawn on the device -- the random-action rollouts of the
 * reference's tests and demos (e.g. tests/.../test_trajectory_vcr.py) without an action tensor (SURVEY 8b:
 * `rng_seed` of ccx_rollout).  The action of agent slot a of global env g at step t (0-based) of its episode j is
 *     k = g*0x9E3779B1 + j*0x85EBCA77 + t*0xC2B2AE3D + a*0x27D4EB2F + seed_lo        (u32 arithmetic)
 *     k = mix(k);  k ^= seed_hi;  k = mix(k);       mix: k^=k>>16; k*=0x7FEB352D; k^=k>>15; k*=0x846CA68B; k^=k>>16
 *     action = (k * 5) >> 32
 * for every agent of env.agents (others: CCX_ACTION_ABSENT in actions_out).  It depends on the env's own
 * counters only, so the stream of an env is the same for any split into launches and any world size.  This is
 * NOT numpy's stream: trajectories driven by it are pinned by the oracle's restatement of the same function.
 */
int ccx_set_rng_seed(ccx_handle* h, uint64_t seed);
/*
 * Epsilon-greedy for ccx_rollout_policy's CCX_POLICY_GREEDY / CCX_POLICY_WAITING: the `randomness_factor` of the
 * reference's policies (greedy_policy.py:25-59, waiting_policy.py:25-59; create_greedy_policy's default is 0.1).
 * With probability epsilon an agent takes one of its VALID actions uniformly -- the directions the pre-step state
 * lets it enter (env._is_move_valid) plus wait -- instead of the policy's choice.  The reference draws from one
 * numpy RandomState shared by all agents of an env (a sequential stream); the device draws are counter-based
 * like CCX_POLICY_RANDOM's ("replace with a documented counter-based RNG"):
 *     u = word(seed_lo, seed_hi ^ 0x5BD1E995; g, j, t, a)     (the k of ccx_set_rng_seed's formula, before "* 5")
 *     explore  iff  u < floor(epsilon * 2^32)                (epsilon = 1: 2^32 - 1)
 *     action   =  the ((mix(u + 0x9E3779B9) * count) >> 32)-th valid action in ascending order, count = #valid
 * pinned by the oracle's restatement (ccxo_set_policy_epsilon).  0 (the default) = the deterministic policies.
 * The host classes of collectivecrossing_amd/baseline_policies.py keep the reference's own RandomState stream, and so does
 * the device with ccx_set_policy_stream(CCX_EPS_STREAM_MT19937) (below).
 * ccx_policy_actions honours it as well (same draws: a loop of ccx_policy_actions + ccx_step takes the actions
 * ccx_rollout_policy takes); ccx_greedy_actions is always epsilon = 0.
 */
int ccx_set_policy_epsilon(ccx_handle* h, double epsilon);
/*
 * Where the exploration draws of the scripted policies come from.
 *   CCX_EPS_STREAM_COUNTER (default): the counter-based draws documented above.
 *   CCX_EPS_STREAM_MT19937: the REFERENCE's own stream.  The reference's policies hold one
 *     `np.random.RandomState(seed)` (greedy_policy.py:31, waiting_policy.py:31; create_greedy_policy /
 *     create_waiting_policy seed it with 42, :452-465) and every get_action call draws from it in turn --
 *     `random_state.random() < randomness_factor` (:49), then `random_state.choice(valid_actions)` (:57) -- for the
 *     agents of env.agents in index order (scripts/run_greedy_policy_demo.py:67-109).  With this stream every env owns
 *     one such generator (numpy's legacy MT19937: init_genrand seeding, 53-bit doubles from two outputs, choice =
 *     masked rejection on 32-bit outputs, a one-entry list draws nothing), seeded here with seeds[e] (HOST array u32 [E])
 *     or, seeds NULL, with `seed` for every env (= one policy object per env, as the reference's callers have), and
 *     walked on the device by one wave per env: an epsilon episode of the reference replays ACTION FOR ACTION
 *     (tests: the reference-recorded g11_epsilon_policy_* episodes).  epsilon is compared as the double given to
 *     ccx_set_policy_epsilon.  The stream is sequential per env, so
 *       - ccx_policy_actions draws from it (every call advances the generators; epsilon 0 draws nothing);
 *       - ccx_rollout_policy (greedy / waiting, epsilon > 0) runs policy -> step -> policy ... as separate launches
 *         on the handle's stream instead of the fused kernel: the mode for replaying / validating against the
 *         reference, not for throughput (any batch size works; the fused kernel keeps the counter-based draws);
 *       - the generators run on across episodes (auto_reset), as a policy object of the reference does;
 *       - ccx_greedy_actions and CCX_POLICY_RANDOM never touch them.
 *     Calling it again re-seeds.  Synchronous.
 * ccx_get_policy_stream: the kind in effect and (state != NULL, host u32 [E][625]) every env's generator as numpy's
 * RandomState.get_state() has it: key[624] then pos.  Synchronises the handle's stream.
 */
#define CCX_EPS_STREAM_COUNTER 0
#define CCX_EPS_STREAM_MT19937 1
int ccx_set_policy_stream(ccx_handle* h, int32_t kind, const uint32_t* seeds, uint32_t seed);
int ccx_get_policy_stream(ccx_handle* h, int32_t* kind, uint32_t* state);

/*
 * Opt-in input validation for the array API (the dict API validates on the host).  The reference raises
 * ValueError for an action outside 0..4 and for an agent id the env does not have
 * (_check_action_and_agent_validity, collectivecrossing.py:685-711); ccx_step / ccx_rollout by default
 * treat any action byte other than 0..3 as "no move" and trust `order` to be a permutation.  With
 * checking enabled every launch that takes an action tensor is preceded by an elementwise kernel that
 * counts action bytes outside {0..4, CCX_ACTION_ABSENT} and move-order rows that are not a permutation
 * of 0..N-1; the next synchronising call (ccx_synchronize, ccx_read_counters, ccx_check_inputs) then
 * fails ONCE with CCX_EINVAL and a message naming both counts ("Invalid action", "Unknown agent ID").
 * The offending entries have been stepped as "no move" / an undefined order by then: a caller that
 * gets the error must discard those envs.  Costs one extra read of the action tensor (1 of 16N+34
 * bytes per agent-step).
 */
int ccx_set_check_inputs(ccx_handle* h, int32_t enabled);
int ccx_check_inputs(ccx_handle* h);     /* synchronises; CCX_EINVAL if anything was counted */

int ccx_zero_counters(ccx_handle* h);
int ccx_read_counters(ccx_handle* h, ccx_counters* out_host);   /* synchronous */
/* device pointer to the 6 u64 counters (for an RCCL all-reduce by the caller).  The rollout kernel
 * accumulates per-tile partial counters; this call enqueues their reduction on the handle's stream, so
 * the totals cover every launch enqueued BEFORE it (call it again after later launches). */
int ccx_counters_device_ptr(ccx_handle* h, uint64_t** out);

/*
 * The one collective of the multi-GPU layout, on RCCL directly: contiguous env shards never
 * exchange data; once per measurement window the six u64 counters are summed over the ranks.
 * ccx_rccl_allreduce_counters enqueues, on the handle's stream, the reduction of the per-tile partial
 * counters and ONE ncclAllReduce(ncclSum, 6 x u64) over `rccl_comm` (an ncclComm_t passed as void*)
 * into out_device (device memory, 6 x u64); *num_ranks (may be NULL) receives the communicator size.
 * The handle's own counters keep the per-rank values.  The communicator is the caller's: either one it
 * already has, or one made with the helpers below (rank 0 draws the 128-byte unique id, ships it to the
 * other ranks by any means -- bench.py uses the torch.distributed store -- and every rank calls
 * ccx_rccl_comm_create with the device its handle lives on).  librccl.so.1 is bound at run time; without
 * it these calls fail with CCX_ENODEVICE and everything else keeps working.
 * No reference counterpart: its parallelism is one env per RLlib EnvRunner process
 * (examples/training_script.py:84).
 */
#define CCX_RCCL_UNIQUE_ID_BYTES 128
int ccx_rccl_unique_id(void* id_out_128 /* host */);
int ccx_rccl_comm_create(int32_t num_ranks, const void* id_128 /* host */, int32_t rank, int32_t device,
                         void** comm_out);
int ccx_rccl_comm_destroy(void* comm);
int ccx_rccl_allreduce_counters(ccx_handle* h, void* rccl_comm, uint64_t* out_device, int32_t* num_ranks);

/* Launch timing, off by default (two event records per launch cost a step-wise loop several
 * microseconds per step): when enabled, HIP events are recorded on the handle's stream around every
 * ccx_step / ccx_rollout kernel and ccx_last_launch_ms returns the duration of the most recent one
 * (it synchronises on the stop event). */
int ccx_set_timing(ccx_handle* h, int32_t enabled);
int ccx_last_launch_ms(ccx_handle* h, float* ms);

/* launch-shape tuning (0 = library default): lanes of each 64-wide wavefront that carry agents
 * (a multiple of the per-env lane group), and wavefronts per workgroup. */
int ccx_set_launch_shape(ccx_handle* h, int32_t lanes_per_wave, int32_t waves_per_block);
/* writer wavefronts per env tile (0 = library default, 1..7): the wavefronts that turn a step into
 * reward / flag bytes / observation rows next to the wavefront that simulates it */
int ccx_set_writers(ccx_handle* h, int32_t writers_per_tile);
/* store throttle: stores a writer wavefront may still have in flight when it starts the next step
 * (0 = library default, -1 = unlimited, 1..63).  Many small env tiles oversubscribe the HBM write
 * queues; bounding the in-flight stores raises the sustained write rate. */
int ccx_set_store_throttle(ccx_handle* h, int32_t max_stores_in_flight);
/* Step pacing of rollouts that write observations: every env tile starts env-step s no earlier than
 * t0 + s * pace on the GPU's 100 MHz clock, which turns the output into a smooth stream at (just under)
 * the HBM drain rate instead of bursts that oversubscribe the write queues.
 *   0  = adaptive (default): starts from the write rate measured in-process at the first long rollout
 *        (ccx_set_pace_calibration; an assumed 6.8 TB/s without it) and is retuned by the kernel after every
 *        launch that lasts ~50 us or more (64 steps of the 4096 x 8 shape, 5 of a 4096 x 32 one; a launch
 *        shorter than ~12 us is not paced at all: late => slower, on time => 0.4 % faster, a collapse of the drain
 *        rate => +3 % and a decaying floor); batches too small to fill the drain rate are not paced at all
 *   -1 = off;   > 0 = fixed pace in nanoseconds per env-step.
 * ccx_get_step_pace returns the pace in effect (synchronises).  Results never depend on it. */
int ccx_set_step_pace(ccx_handle* h, int32_t ns_per_env_step);
int ccx_get_step_pace(ccx_handle* h, float* ns_per_env_step);
/* The controller's state for diagnostics and tests (synchronises): out6 = { the pace the next launch starts
 * from (ns), the floor just above the last collapse (ns), launches since that collapse, 1 if rollouts of this
 * shape are paced at all, the pace of the last collapse = the cliff (ns), how often that cliff was confirmed } */
int ccx_get_pace_state(ccx_handle* h, float* out6);
/* Where the ADAPTIVE controller starts (ns per env-step; 0 = the library's assumption of 6.8 TB/s): a
 * caller that remembers the pace a previous handle of the same shape converged to (ccx_get_step_pace)
 * skips the descent of the first launches; the value is also the controller's first floor (it decays like any
 * floor), so that the start of a process is not spent probing below a pace that is already known.  Restarts the
 * controller. */
int ccx_set_step_pace_start(ccx_handle* h, float ns_per_env_step);
/* Start-up calibration (default on; CCX_PACE_CALIBRATION=0 in the environment turns it off for new handles).  The first
 * adaptive paced rollout of a handle / launch shape -- one that writes observations for ~50 us or more -- first streams
 * filler into the caller's own observation buffer (which that rollout overwrites anyway) for ~2.5 ms with the writer
 * wavefronts' store type, takes the best pass as a lower bound of the drain rate of this box and starts the controller
 * 5 % above it (it descends further by itself until a launch comes in late).  One stream synchronisation; never inside a stream capture (a rollout that would have to restart
 * the controller while capturing fails with CCX_EINVAL: run one eager rollout of the shape first).  Without it -- or
 * before the first such rollout -- the start value is an assumed 6.8 TB/s. */
int ccx_set_pace_calibration(ccx_handle* h, int32_t enabled);
/* where the pace controller started: the value (ns per env-step; 0 if rollouts of this shape are not paced), its
 * source (CCX_PACE_START_*) and the write rate the calibration probe measured (GB/s, 0 = it did not run).  Any pointer
 * may be NULL. */
#define CCX_PACE_START_UNPACED    0  /* rollouts of this shape are not paced (too small to be memory-bound, or pacing off) */
#define CCX_PACE_START_ASSUMED    1  /* the library's assumption (6.8 TB/s): no calibration has run (yet)                  */
#define CCX_PACE_START_CALLER     2  /* ccx_set_step_pace_start                                                           */
#define CCX_PACE_START_CALIBRATED 3  /* measured in-process at the first adaptive rollout                                 */
#define CCX_PACE_START_FIXED      4  /* ccx_set_step_pace(h, ns > 0): no controller                                       */
int ccx_get_pace_start(ccx_handle* h, float* ns_per_env_step, int32_t* source, float* probe_gbs);
/* Performance experiments without an ABI change; results never depend on a tunable.  -1 = the library's
 * choice for the launch shape (pace_phase, tile_map).
 *   "pace_phase"   0 = every tile starts env-step s at t0 + s * pace, 1 = tiles are phased over the step
 *                  period in tile order (one write window sweeps through the slab), 2 = hashed phases,
 *                  3 = in tile order within each XCD's share (with tile_map 0)
 *   "tile_map"     0 = workgroups of one XCD take adjacent tiles, v >= 1 = groups of 2^(v-1) adjacent tiles
 *                  per XCD dealt round-robin (1 = tile = workgroup index)
 *   "writer_roles" 1 = writer wave 0 of a tile writes the small outputs only and the others share the observation
 *                  rows, 0 = every writer takes a share of the rows (writer 0 the small outputs on top), -1 = by
 *                  launch shape (split wherever a tile of at most 12 store iterations per step has two or more writers)
 *   "hand2"        how the simulating wavefront of a tile hands an env-step to its writer wavefronts: 1 (default) = launches
 *                  that are not paced use a ring of hand-off words with a sequence word and per-writer progress words in
 *                  LDS (no barrier; paced launches keep one workgroup barrier per step, which regularises their store
 *                  stream), 0 = a barrier per step always, 2 = the ring always
 *   "stats_naive"  1 = ccx_episode_stats_update runs its accumulate kernel with one dependent load per step (what the
 *                  pipelined loads are measured against, profiles/episode_stats_timing.py); 0 (default) = pipelined
 *   "max_launch_steps"  > 0: ccx_rollout cuts a rollout into kernel launches of at most this many env-steps (the library
 *                  does so by itself where one launch would exceed 4 GiB per small output stream); 0 = automatic
 *   "pair_rows"    in small batches (role-split writers, launches that are not paced) every writer can get a second
 *                  staging slot in LDS and a row writer then takes TWO env-steps per iteration whenever the simulating
 *                  wavefront is that far ahead: -1 (default) = where it pays (half-tile shapes: up to 128 full tiles),
 *                  1 = in every small batch, 0 = never
 *   "reset_obs_fused"  0 = CCX_RESET_OBS_NEXT single steps take the fix-up kernel too (what the fused rows are measured
 *                  against, profiles/reset_obs_timing.py); 1 (default) = inside the step launch where it applies */
int ccx_set_tunable(ccx_handle* h, const char* name, int32_t value);
/* workgroups of a rollout launch with outputs, and how many of them the device holds at once (a grid
 * larger than that runs in rounds; the pace of a partial last round is scaled accordingly) */
int ccx_get_residency(ccx_handle* h, int32_t* resident_workgroups, int32_t* workgroups);
/* the writers per tile and the store throttle in effect (0 = unlimited) */
int ccx_get_writer_shape(ccx_handle* h, int32_t* writers_per_tile, int32_t* max_stores_in_flight);
int ccx_get_launch_shape(ccx_handle* h, int32_t* lanes_per_wave, int32_t* waves_per_block,
                         int32_t* group_lanes, int32_t* num_blocks);
/* Plugin point for position-only user strategies on the batch path.  The reference accepts ANY registered RewardFunction /
 * TerminatedFunction class (rewards.py:16-38, 186-216; terminateds.py:16-36, 86-114); a class whose value depends on nothing
 * but the agent's own type and cell is lowered to a table by the host (collectivecrossing_amd/params.py: position_only_tables)
 * and evaluated inside the kernels like the built-in strategies, at the same speed:
 *   ccx_set_reward_table      rewards[id] of an agent that was live before the step and stands on cell (x, y) after it =
 *                             table[type][y][x]: f64 [height + 1][width + 1] per agent type (boarding, exiting), host memory.
 *                             Staged in LDS next to the cell table (16 bytes per cell of the padded grid): grids whose tables do
 *                             not fit are refused with CCX_EINVAL.
 *   ccx_set_terminated_table  terminateds[id] = table[type][y][x] != 0 (u8), for individual_at_destination handles;
 *                             terminateds["__all__"] stays all(values) (collectivecrossing.py:256).  Deactivation on the destination
 *                             row (:210-212) is env logic, not strategy, and does not change.
 * NULL for both types restores the built-in strategy of the handle's params.  Both synchronise the handle's stream. */
int ccx_set_reward_table(ccx_handle* h, const double* boarding_per_cell, const double* exiting_per_cell);
int ccx_set_terminated_table(ccx_handle* h, const uint8_t* boarding_per_cell, const uint8_t* exiting_per_cell);

/* Launch shape of the SHORT-LAUNCH kernel (csrc/ccx_step.hip): ccx_step and ccx_rollout calls of at most 16 steps with an
 * action tensor (with or without a move order) are CollectiveCrossingEnv.step itself (collectivecrossing.py:161-261) with one workgroup
 * per env tile -- a sim wave plus *row_waves waves that gather the observation rows, one LDS barrier per step, no ring, no
 * pacing.  *ok = 0: this handle's short launches take the rollout kernel (grid too large for the LDS tables).  Tunables:
 * "step_kernel" (0 = always the rollout kernel), "step_rows" (row waves per tile), "step_lanes" (lanes per wave carrying
 * agents). */
int ccx_get_step_shape(ccx_handle* h, int32_t* ok, int32_t* lanes_per_wave, int32_t* row_waves,
                       int32_t* num_blocks, int32_t* lds_bytes);

/* Zero-copy I/O for single-env stepping (the dict API of collectivecrossing.py:161-261 needs every
 * output on the host after each step): the device address of page-locked host memory (hipHostMalloc /
 * hipHostRegister, e.g. a torch pinned tensor).  Pass it to ccx_step as actions / outputs and the
 * kernel reads and writes the host buffer over the host link -- one launch + one sync per step,
 * no memcpy.  Fails with CCX_EINVAL for pageable or unregistered memory. */
int ccx_host_device_pointer(ccx_handle* h, void* pinned_host, void** device_ptr);
/* rebind the handle to another HIP stream of its device (synchronises the old one first) */
int ccx_set_stream(ccx_handle* h, void* stream);
int ccx_synchronize(ccx_handle* h);

#ifdef __cplusplus
}
#endif
#endif /* CCX_H */
