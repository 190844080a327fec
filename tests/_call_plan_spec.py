"""An independent restatement of what libccx decides per stepping call: how the call is cut into launches, which kernel
takes a launch and how that launch is driven.

Written from the C ABI layer as it stood before these decisions moved into the pure planner (csrc/ccx_plan.hip:
``plan_call`` / ``plan_launch``), entry point by entry point, with Python integers -- no width can overflow here.
tests/test_call_plan.py holds ``ccxi_plan_call`` against it field for field; it is the reference, not a copy of the C++.

A *shape* is a dict of the fields of one planned launch shape that these rules read (the names of ``ccxi_plan``'s fields):
num_blocks, resident_blocks, step_bytes, paced, pace_adapt, pace_min_k, adapt_min_k, ring_when_paced, step_ok.  A *call* is a
dict of the fields of ``ccxi_call_in``.  Every two-way decision goes through ``_if`` so that the test can tell which sides
its sweep reached (``reached``).
"""

from collections import Counter

STEP_MAX_K = 16            # env-steps per launch of the short-launch kernel
KERNEL_STEP, KERNEL_ROLLOUT = 0, 1

FIELDS = ["steps_per_launch", "launches", "refused", "stepwise", "k", "kernel", "shape", "paced", "adaptive", "pace_adapt",
          "flip_slot", "hand_flags", "by_rounds", "per_round", "rounds", "masks_fused", "reset_obs_fused"]

DECISIONS = ["mixed", "mixed_fused", "cap_by_max_launch_steps", "odd_slab", "odd_slab_even_steps", "one_launch", "refused",
             "step_kernel", "masks_fused", "reset_obs_fused", "no_rows_shape", "paced", "adaptive", "captured_adaptive",
             "flags_always", "flags_unpaced", "ring_when_paced", "several_rounds", "thin_second_round", "rounds_forced",
             "rounds_by_size", "rounds_balanced"]
reached = Counter()


def _if(name, cond):
    assert name in DECISIONS
    reached[name, bool(cond)] += 1
    return bool(cond)


def obs_step_bytes(E, N):
    return E * N * (6 + 4 * N) * 4


# ---- the launch modes: one definition for the host and the kernel (ccx_kernels.h) ---------------------------------------
def launch_is_paced(handle_paces, writes_obs, K, pace_min_k):
    return bool(handle_paces and writes_obs and K >= pace_min_k)


def launch_is_adaptive(handle_paces, handle_adapts, writes_obs, K, pace_min_k, adapt_min_k):
    return bool(launch_is_paced(handle_paces, writes_obs, K, pace_min_k) and handle_adapts and K >= adapt_min_k)


# ---- one launch ------------------------------------------------------------------------------------------------------
def _step_launch(call, k, masks, rso, mixed):
    """The short-launch kernel: it writes the masks / the restarted rows itself where it has an instantiation for that."""
    has_order = bool(call["order"])
    return dict(k=k, kernel=KERNEL_STEP, shape=0, paced=0, adaptive=0, pace_adapt=0, flip_slot=0, hand_flags=0, by_rounds=0,
                per_round=0, rounds=0,
                masks_fused=int(_if("masks_fused", masks and k == 1 and not has_order)),
                reset_obs_fused=int(_if("reset_obs_fused", rso and call["reset_obs_fused"] != 0 and k == 1 and not has_order
                                        and not mixed)))


def _rollout_launch(E, N, shapes, call, k):
    """The rollout kernel, round by round where the grid exceeds the device."""
    writes_obs = bool(call["writes_obs"])
    small = _if("no_rows_shape", not writes_obs and call["small_shape"] != 0)
    s = shapes[1] if small else shapes[0]
    paced = _if("paced", launch_is_paced(s["paced"], writes_obs, k, s["pace_min_k"]))
    adaptive = _if("adaptive", launch_is_adaptive(s["paced"], s["pace_adapt"], writes_obs, k, s["pace_min_k"], s["adapt_min_k"]))
    pace_adapt = 0 if _if("captured_adaptive", adaptive and call["capturing"]) else s["pace_adapt"]
    # sequence words instead of a barrier per step: tunable hand2 = 0 never, 1 in launches that are not paced, 2 always ...
    if _if("flags_always", call["hand2"] >= 2):
        hand_flags = 1
    else:
        hand_flags = int(_if("flags_unpaced", call["hand2"] == 1 and not paced))
    # ... and the paced launches of a rows shape whose step period is close to the sim chain keep the ring too
    if _if("ring_when_paced", call["hand2"] == 1 and writes_obs and not small and shapes[0]["ring_when_paced"]):
        hand_flags = 1
    nb, res = s["num_blocks"], s["resident_blocks"]
    rows_bytes = k * obs_step_bytes(E, N) if writes_obs else 0
    n_rounds = -(-nb // res) if res > 0 else 1
    by_rounds, per_round = False, nb
    if _if("several_rounds", res > 0 and nb > res):
        thin = _if("thin_second_round", n_rounds == 2 and (nb - res) < 0.3 * res
                   and float(s["step_bytes"]) / 7000.0 * (0.5 * nb / res) >= 1200.0)
        if _if("rounds_forced", call["round_launches"] >= 2):
            by_rounds = True
        elif call["round_launches"] == 1:
            if _if("rounds_by_size", rows_bytes > 3_500_000_000):
                by_rounds = True
            elif _if("rounds_balanced", paced and thin):
                by_rounds = True
    if by_rounds:
        per_round = -(-nb // n_rounds)            # equal rounds
    return dict(k=k, kernel=KERNEL_ROLLOUT, shape=int(small), paced=int(paced), adaptive=int(adaptive), pace_adapt=pace_adapt,
                flip_slot=int(adaptive and not call["capturing"]), hand_flags=hand_flags, by_rounds=int(by_rounds),
                per_round=per_round, rounds=len(range(0, nb, per_round)), masks_fused=0, reset_obs_fused=0)


def _launch_one(E, N, shapes, call, k, masks, rso):
    """One launch of a call from ccx_step / ccx_rollout / ccx_rollout_policy."""
    short = (k <= STEP_MAX_K and call["actions"] and call["policy"] == 0 and not call["actions_out"]
             and shapes[0]["step_ok"] and call["step_kernel"] != 0)
    if _if("step_kernel", short):
        return _step_launch(call, k, masks, rso, mixed=False)
    return _rollout_launch(E, N, shapes, call, k)


# ---- a call ----------------------------------------------------------------------------------------------------------
def _cut(steps_per_launch, K, launch):
    launches = -(-K // steps_per_launch)
    assert 0 <= launch < launches
    return launches, min(steps_per_launch, K - launch * steps_per_launch)


def plan(E, N, shapes, call, launch=0):
    """Every field of FIELDS for launch number ``launch`` of ``call`` on a handle of E x N with the two ``shapes``
    (rows, no rows)."""
    K = call["K"]
    masks, rso = bool(call["masks_bound"]), bool(call["reset_obs_on"])
    nothing = dict.fromkeys(FIELDS[4:], 0)
    if _if("mixed", call["mixed"]):
        if _if("mixed_fused", shapes[0]["step_ok"] and call["step_kernel"] != 0):
            # policy + merge + step in one launch of the step kernel per <= 16 steps; the masks only in a call of one step,
            # the restarted rows never
            launches, k = _cut(STEP_MAX_K, K, launch)
            one = _step_launch(call, k, masks and K == 1, False, mixed=True)
            return dict(steps_per_launch=STEP_MAX_K, launches=launches, refused=0, stepwise=0, **one)
        # the composition itself, step by step: policy kernel, merge kernel, then the step as a one-step call from a tensor
        # (no actions_out of its own, nothing fused); without the step kernel that is the rollout kernel
        launches, k = _cut(1, K, launch)
        step = dict(call, K=1, actions=1, actions_out=0, policy=0, mixed=0)
        one = _launch_one(E, N, shapes, step, 1, False, False)
        return dict(steps_per_launch=1, launches=launches, refused=0, stepwise=1, **one)
    # the small output streams are addressed with 32-bit byte offsets: below 4 GiB per launch and stream (the widest: 16
    # bytes per agent slot and step)
    fit = 0xFFFFFFFF // (E * N * 16)
    max_k = min(fit - 1 if fit > 1 else 1, 0x7FFFFFFF)
    if _if("cap_by_max_launch_steps", call["max_launch_steps"] > 0):
        max_k = min(max_k, call["max_launch_steps"])
    # a slab of an odd number of agent slots is not a multiple of 16 bytes: sub-launches start on even steps
    odd = _if("odd_slab", call["writes_obs"] and obs_step_bytes(E, N) % 16 != 0)
    if _if("odd_slab_even_steps", odd and max_k > 1):
        max_k -= max_k % 2
    if _if("one_launch", K <= max_k):
        assert launch == 0
        return dict(steps_per_launch=max_k, launches=1, refused=0, stepwise=0, **_launch_one(E, N, shapes, call, K, masks, rso))
    if _if("refused", odd and max_k == 1):
        return dict(steps_per_launch=1, launches=0, refused=1, stepwise=0, **nothing)
    launches, k = _cut(max_k, K, launch)
    # (the sub-launches of a cut fuse nothing)
    return dict(steps_per_launch=max_k, launches=launches, refused=0, stepwise=0, **_launch_one(E, N, shapes, call, k, False, False))
