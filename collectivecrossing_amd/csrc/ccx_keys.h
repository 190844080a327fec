// ccx_keys.h -- which INSTANTIATION of the three stepping kernels a launch takes, as pure functions of integers and
// booleans: rollout_kernel / rollout_kernel_v128 <GLOG, PAIR, OUT, OCC, PLAIN> (ccx_rollout_dev.h), step_kernel <GLOG, PAIR,
// K1, ORD, POL, MSK, RSO> (ccx_step.hip) and observe_kernel <GLOG, PAIR> (ccx_kernels.hip).  The launch functions call
// these and switch on the result; the tests call them through the internal entry points below (ccx_plan.hip, ccx_api.hip)
// on a machine without a GPU.  Plain host C++: no HIP header, nothing of the device.  Not installed, not part of the ABI.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>

extern "C" {

// a kernel and its template arguments, one int32 each in the order of the template's parameter list (the rest zero)
enum { CCXI_KEY_NONE = -1, CCXI_KEY_STEP = 0, CCXI_KEY_ROLLOUT = 1, CCXI_KEY_OBSERVE = 2 };   // (0 / 1: ccxp::KERNEL_*)
typedef struct ccxi_key {
    int32_t kernel;
    int32_t v[7];
} ccxi_key;

// what the key of a stepping call reads besides the planner's inputs and the call (ccx_plan.h: ccxi_plan_in, ccxi_call_in)
typedef struct ccxi_key_facts {
    int32_t obs, reward, agent_flags, env_flags, obs_compact;   // 1: the call passes this output array
    int32_t obs_residue;                                        // address of the obs array mod 128
} ccxi_key_facts;

}  // extern "C"

namespace ccx {

constexpr int kFastObsIters = 10;  // observation store iterations whose LDS addresses live in VGPRs

struct RolloutKey { int glog; bool pair; int out; bool occ, plain; };
struct StepKey { int glog; bool pair, k1, ord, pol, msk, rso; };
struct ObserveKey { int glog; bool pair; };

// what launch_rollout_g reads of its arguments: the launch shape (glog, writers, occ), the kernel parameters (N, E, EW,
// units_per_wave, writer0_small, user_tables), which outputs are asked for and where the obs array lies, how the call is driven
struct RolloutFacts {
    int glog, N, E, EW, units_per_wave, writers;
    bool writer0_small, occ;
    bool want_out;          // any of obs / reward / agent_flags / env_flags / obs_compact / actions_out
    bool has_obs;
    uint32_t obs_residue;   // address of the obs array mod 128
    bool has_order, has_policy, user_tables;
};

inline RolloutKey rollout_key(const RolloutFacts& f) {
    const bool pair = (f.N % 2) == 0;
    // edge iterations: the tile regions of the observation output share 128-byte lines with their neighbours
    const size_t tile_region = (size_t)f.EW * f.N * (6 + 4 * f.N) * 4u, slab = (size_t)f.E * f.N * (6 + 4 * f.N) * 4u;
    const bool edges = f.has_obs && (((tile_region | slab) & 127u) != 0 || (f.obs_residue & 127u) != 0);
    // (3: the slab stride itself is not a multiple of 128 bytes -- `lead` per step, ccx_rollout_body.inc: VARLEAD -- and a row
    //  writer has more store iterations than it caches source addresses for: 50 agents x 532 envs 0.50 -> 0.88 of the peak.  Narrow
    //  rows, all of whose iterations are register-cached, are faster with the launch-wide layout: 3 agents 0.28 vs 0.19.)
    const int row_writers = std::max(1, f.writers - ((f.writer0_small && f.writers > 1) ? 1 : 0));
    const int its = ((f.units_per_wave >> (pair ? 1 : 0)) + 63) / 64;
    const bool long_rows = (its + row_writers - 1) / row_writers > kFastObsIters;
    const int outm = f.want_out ? (edges ? ((slab & 127u) != 0 && long_rows ? 3 : 2) : 1) : 0;
    const bool plain = !f.has_order && !f.has_policy && !f.user_tables;   // (user reward / terminated tables: the general instantiations)
    return RolloutKey{f.glog, pair, outm, f.occ, plain};
}

// launch_step_g: `masks` / `rso` are what the launch was GIVEN (the plan's masks_fused / reset_obs_fused: ccx_plan.hip); the
// MSK instantiations exist for one env-step without a move order, the RSO ones also without a policy (ccx_kernels.h:
// step_masks_fused, step_reset_obs_fused -- the launch refuses anything else), and both come as K1, not ORD
inline StepKey step_key(int glog, int N, int K, bool has_order, bool has_policy, bool masks, bool rso) {
    const bool pair = (N % 2) == 0;
    if (rso) return StepKey{glog, pair, true, false, false, masks, true};
    if (masks) return StepKey{glog, pair, true, false, has_policy, true, false};
    return StepKey{glog, pair, K == 1, has_order, has_policy, false, false};
}

inline ObserveKey observe_key(int glog, int N) { return ObserveKey{glog, (N % 2) == 0}; }

inline ccxi_key pack_key(const RolloutKey& k) { return ccxi_key{CCXI_KEY_ROLLOUT, {k.glog, k.pair, k.out, k.occ, k.plain, 0, 0}}; }
inline ccxi_key pack_key(const StepKey& k) { return ccxi_key{CCXI_KEY_STEP, {k.glog, k.pair, k.k1, k.ord, k.pol, k.msk, k.rso}}; }
inline ccxi_key pack_key(const ObserveKey& k) { return ccxi_key{CCXI_KEY_OBSERVE, {k.glog, k.pair, 0, 0, 0, 0, 0}}; }

}  // namespace ccx

extern "C" {

// the key of launch number `launch` (0 .. launches - 1, or -1: the last) of one stepping call: both shapes of `in` planned as in ccxi_plan_call, the call cut and
// its launch planned (plan_call, plan_launch), then rollout_key / step_key of what that launch is given.  A call that the
// mixed entry point steps one env-step per launch (ccxi_call_out: stepwise) launches the one-step call of an action tensor.
// kernel = CCXI_KEY_NONE for a refused call.  Works without a GPU.
int ccxi_call_key(const struct ccxi_plan_in* in, const int* blocks_per_cu, const struct ccxi_call_in* call, const ccxi_key_facts* facts,
                  int launch, ccxi_key* out);
// the same for n calls of one handle, planned once: out[2 i] the key of call i's first launch, out[2 i + 1] of its last
int ccxi_call_keys(const struct ccxi_plan_in* in, const int* blocks_per_cu, const struct ccxi_call_in* calls, const ccxi_key_facts* facts,
                   int n, ccxi_key* out);
// the key of ccx_observe / ccx_expand_observations on a handle planned from `in`
int ccxi_observe_key(const struct ccxi_plan_in* in, ccxi_key* out);
// what a live handle launched last: which = 0 the last launch of a stepping call (ccx_step, ccx_rollout, ccx_rollout_policy,
// ccx_rollout_mixed), 1 the last ccx_observe / ccx_expand_observations; CCXI_KEY_NONE before the first
int ccxi_handle_last_key(const struct ccx_handle* h, int which, ccxi_key* out);

}  // extern "C"
