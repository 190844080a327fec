"""ctypes mirror of ``include/ccx.h`` (the C-ABI of libccx).

Only declarations live here: structures, constants and the prototype table used by
``_lib.load()`` to type-check every exported symbol.  No compute, no fallbacks.
"""

from __future__ import annotations

import ctypes as C

ABI_VERSION = 5

# ccx_status
OK, EINVAL, ENOMEM, EHIP, ENODEVICE = 0, -1, -2, -3, -4

# reward / terminated / truncated modes (include/ccx.h enums)
REWARD_MODES = {"default": 0, "simple_distance": 1, "binary": 2, "constant_negative": 3}
TERMINATED_MODES = {"individual_at_destination": 0, "all_at_destination": 1}
TRUNCATED_MODES = {"max_steps": 0, "custom": 0}  # truncateds.py:64-95: same arithmetic

ACTION_ABSENT = 255
POLICY_GREEDY = 1
POLICY_WAITING = 2
POLICY_RANDOM = 3
POLICIES = {"greedy": POLICY_GREEDY, "waiting": POLICY_WAITING, "random": POLICY_RANDOM}

# agent_flags bits
AF_TERMINATED, AF_TRUNCATED, AF_LIVE, AF_OBS = 0x01, 0x02, 0x04, 0x08
AF_IN_TRAM_AREA, AF_AT_DOOR, AF_ACTIVE, AF_AT_DEST = 0x10, 0x20, 0x40, 0x80
# env_flags bits
EF_ALL_TERMINATED, EF_ALL_TRUNCATED, EF_RESET = 0x01, 0x02, 0x04


class CcxParams(C.Structure):
    _fields_ = [
        ("width", C.c_int32), ("height", C.c_int32), ("division_y", C.c_int32),
        ("tram_left", C.c_int32), ("tram_right", C.c_int32),
        ("door_left", C.c_int32), ("door_right", C.c_int32),
        ("num_boarding", C.c_int32), ("num_exiting", C.c_int32),
        ("boarding_dest_y", C.c_int32), ("exiting_dest_y", C.c_int32),
        ("reward_mode", C.c_int32), ("terminated_mode", C.c_int32), ("truncated_mode", C.c_int32),
        ("max_steps", C.c_int32), ("_pad0", C.c_int32),
        ("boarding_destination_reward", C.c_double), ("tram_door_reward", C.c_double),
        ("tram_area_reward", C.c_double), ("distance_penalty_factor", C.c_double),
        ("goal_reward", C.c_double), ("no_goal_reward", C.c_double), ("step_penalty", C.c_double),
    ]

    @property
    def num_agents(self) -> int:
        return self.num_boarding + self.num_exiting


class CcxState(C.Structure):
    _fields_ = [
        ("x", C.c_void_p), ("y", C.c_void_p), ("active", C.c_void_p), ("terminated", C.c_void_p),
        ("truncated", C.c_void_p), ("step_count", C.c_void_p), ("episode", C.c_void_p),
    ]


class CcxStepOut(C.Structure):
    _fields_ = [("obs", C.c_void_p), ("reward", C.c_void_p), ("agent_flags", C.c_void_p),
                ("env_flags", C.c_void_p), ("obs_compact", C.c_void_p)]


class CcxRolloutOut(C.Structure):
    _fields_ = [("obs", C.c_void_p), ("reward", C.c_void_p), ("agent_flags", C.c_void_p),
                ("env_flags", C.c_void_p), ("obs_compact", C.c_void_p)]


class CcxCounters(C.Structure):
    _fields_ = [("env_steps", C.c_uint64), ("agent_steps", C.c_uint64),
                ("live_agent_steps", C.c_uint64), ("episodes", C.c_uint64),
                ("moves", C.c_uint64), ("arrivals", C.c_uint64)]

    def as_dict(self) -> dict[str, int]:
        return {name: int(getattr(self, name)) for name, _ in self._fields_}


class CcxEpisodeStats(C.Structure):
    """``ccx_episode_stats``: device pointers of a handle's episode statistics (CCX_EPISODE_STATS)."""

    _fields_ = [(name, C.c_void_p) for name in (
        "ret", "live_steps", "steps", "closed", "finished", "last_ret", "last_live_steps", "last_steps", "last_end",
        "log_env", "log_episode", "log_steps", "log_end", "log_ret", "log_live_steps", "log_count")] + [
        ("log_capacity", C.c_int64)]


ADAM_MAX_TENSORS = 32


class CcxAdamTensor(C.Structure):
    """``ccx_adam_tensor``: one row of ``ccx_adam_step``'s table (CCX_ADAM), device pointers and the element count."""

    _fields_ = [("param", C.c_void_p), ("grad", C.c_void_p), ("m", C.c_void_p), ("v", C.c_void_p), ("numel", C.c_int64)]


SIDES_MAX_GROUPS = 8


class CcxSlotGroup(C.Structure):
    """``ccx_slot_group``: one row of the group table of CCX_SIDES, the slot mask and the head's four device pointers."""

    _fields_ = [("slots", C.c_uint64), ("w1t", C.c_void_p), ("b1", C.c_void_p), ("w2", C.c_void_p), ("b2", C.c_void_p)]


PRIO_MAX_TD = 8
NSTEP_MAX = 16
DUELING_MAX_ARRAYS = 4

COUNTER_FIELDS =tuple(name for name, _ in CcxCounters._fields_)

_H = C.c_void_p  # ccx_handle*

# symbol -> (restype, argtypes): every function include/ccx.h declares
PROTOTYPES: dict[str, tuple] = {
    "ccx_abi_version": (C.c_int, []),
    "ccx_build_info": (C.c_char_p, []),
    "ccx_last_error": (C.c_char_p, []),
    "ccx_obs_len": (C.c_int32, [C.c_int32]),
    "ccx_create": (C.c_int, [C.POINTER(CcxParams), C.c_int32, C.c_int64, C.c_int64, C.c_int,
                             C.c_void_p, C.POINTER(_H)]),
    "ccx_destroy": (None, [_H]),
    "ccx_num_envs": (C.c_int32, [_H]),
    "ccx_num_agents": (C.c_int32, [_H]),
    "ccx_state_view": (C.c_int, [_H, C.POINTER(CcxState)]),
    "ccx_set_state_host": (C.c_int, [_H, C.POINTER(CcxState)]),
    "ccx_get_state_host": (C.c_int, [_H, C.POINTER(CcxState)]),
    "ccx_set_reset_pool": (C.c_int, [_H, C.c_void_p, C.c_int64]),
    "ccx_reset_from_pool": (C.c_int, [_H, C.c_void_p]),
    "ccx_fill_reset_pool_seeded": (C.c_int, [_H, C.c_void_p, C.c_int64, C.c_uint64]),
    "ccx_reset_seeded": (C.c_int, [_H, C.c_void_p, C.c_void_p]),
    "ccx_greedy_actions": (C.c_int, [_H, C.c_void_p]),
    "ccx_policy_actions": (C.c_int, [_H, C.c_int32, C.c_void_p]),
    "ccx_observe": (C.c_int, [_H, C.c_void_p]),
    "ccx_expand_observations": (C.c_int, [_H, C.c_void_p, C.c_int64, C.c_void_p]),
    "ccx_render": (C.c_int, [_H, C.c_void_p, C.c_int64, C.c_int, C.c_void_p]),
    "ccx_render_compact": (C.c_int, [_H, C.c_void_p, C.c_int64, C.c_int, C.c_void_p]),
    "ccx_step": (C.c_int, [_H, C.c_void_p, C.c_void_p, C.POINTER(CcxStepOut)]),
    "ccx_step_begin": (C.c_int, [_H, C.c_void_p, C.c_void_p]),
    "ccx_step_finish": (C.c_int, [_H, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(CcxStepOut), C.c_void_p, C.c_int32]),
    "ccx_rollout": (C.c_int, [_H, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32,
                              C.POINTER(CcxRolloutOut)]),
    "ccx_rollout_policy": (C.c_int, [_H, C.c_int32, C.c_int32, C.c_int32, C.POINTER(CcxRolloutOut),
                                     C.c_void_p]),
    "ccx_rollout_mixed": (C.c_int, [_H, C.c_int32, C.c_int32, C.c_uint64, C.c_void_p, C.c_void_p, C.c_int32,
                                    C.POINTER(CcxRolloutOut), C.c_void_p]),
    "ccx_action_masks": (C.c_int, [_H, C.c_void_p]),
    "ccx_bind_action_masks": (C.c_int, [_H, C.c_void_p]),
    "ccx_get_masks_fused": (C.c_int, [_H, C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_int32)]),
    "ccx_set_reset_obs": (C.c_int, [_H, C.c_int32]),
    "ccx_bind_final_obs": (C.c_int, [_H, C.c_void_p, C.c_void_p]),
    "ccx_get_reset_obs_fused": (C.c_int, [_H, C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_int32)]),
    "ccx_episode_stats_enable": (C.c_int, [_H, C.c_int64]),
    "ccx_episode_stats_disable": (C.c_int, [_H]),
    "ccx_episode_stats_view": (C.c_int, [_H, C.POINTER(CcxEpisodeStats)]),
    "ccx_episode_stats_launches": (C.c_int, [_H, C.POINTER(C.c_int32)]),
    "ccx_episode_stats_update": (C.c_int, [_H, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]),
    "ccx_episode_stats_reset": (C.c_int, [_H, C.c_void_p]),
    "ccx_episode_log_clear": (C.c_int, [_H]),
    "ccx_gae": (C.c_int, [_H, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                          C.c_float, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p]),
    "ccx_sample_actions": (C.c_int, [_H, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]),
    "ccx_evaluate_actions": (C.c_int, [_H, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "ccx_evaluate_actions_backward": (C.c_int, [_H, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                                C.c_void_p]),
    "ccx_ppo_workspace_bytes": (C.c_int64, [C.c_int64]),
    "ccx_masked_moments": (C.c_int, [_H, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "ccx_ppo_loss": (C.c_int, [_H, C.c_int64] + [C.c_void_p] * 9 + [C.c_float] * 4 + [C.c_void_p, C.c_void_p]),
    "ccx_ppo_loss_backward": (C.c_int, [_H, C.c_int64] + [C.c_void_p] * 9 + [C.c_float] * 4 + [C.c_void_p] * 4),
    "ccx_mlp_forward": (C.c_int, [_H, C.c_int64] + [C.c_int32] * 4 + [C.c_void_p] * 7),
    "ccx_mlp_sample_actions": (C.c_int, [_H, C.c_int32, C.c_int32] + [C.c_void_p] * 6 + [C.c_int32] + [C.c_void_p] * 4),
    "ccx_mlp_backward_workspace_bytes": (C.c_int64, [C.c_int64, C.c_int32, C.c_int32, C.c_int32]),
    "ccx_mlp_backward": (C.c_int, [_H, C.c_int64] + [C.c_int32] * 4 + [C.c_void_p] * 10),
    "ccx_mlp_wide_forward": (C.c_int, [_H, C.c_int64] + [C.c_int32] * 4 + [C.c_void_p] * 7),
    "ccx_mlp_wide_backward_workspace_bytes": (C.c_int64, [C.c_int64, C.c_int32, C.c_int32, C.c_int32]),
    "ccx_mlp_wide_backward": (C.c_int, [_H, C.c_int64] + [C.c_int32] * 4 + [C.c_void_p] * 10),
    "ccx_mlp_deep_forward": (C.c_int, [_H, C.c_int64] + [C.c_int32] * 5 + [C.c_void_p] * 10),
    "ccx_mlp_deep_sample_actions": (C.c_int, [_H] + [C.c_int32] * 3 + [C.c_void_p] * 8 + [C.c_int32] + [C.c_void_p] * 4),
    "ccx_mlp_deep_q_actions": (C.c_int, [_H] + [C.c_int32] * 4 + [C.c_void_p] * 12),
    "ccx_mlp_deep_backward_workspace_bytes": (C.c_int64, [C.c_int64] + [C.c_int32] * 4),
    "ccx_mlp_deep_backward": (C.c_int, [_H, C.c_int64] + [C.c_int32] * 5 + [C.c_void_p] * 15),
    "ccx_adam_workspace_bytes": (C.c_int64, [C.c_int32, C.POINTER(C.c_int64)]),
    "ccx_adam_step": (C.c_int, [_H, C.c_int32, C.POINTER(CcxAdamTensor), C.c_float, C.c_void_p] + [C.c_float] * 5
                      + [C.c_void_p] * 3),
    "ccx_sides_forward": (C.c_int, [_H, C.c_int64] + [C.c_int32] * 5 + [C.c_void_p, C.c_int32, C.POINTER(CcxSlotGroup), C.c_void_p,
                                    C.c_void_p]),
    "ccx_sides_sample_actions": (C.c_int, [_H, C.c_int32, C.c_int32, C.c_void_p, C.c_int32, C.POINTER(CcxSlotGroup), C.c_void_p,
                                           C.c_int32] + [C.c_void_p] * 4),
    "ccx_sides_backward": (C.c_int, [_H, C.c_int64, C.c_int32, C.c_uint64] + [C.c_int32] * 4 + [C.c_void_p] * 10),
    "ccx_q_actions": (C.c_int, [_H] + [C.c_void_p] * 5),
    "ccx_td_workspace_bytes": (C.c_int64, [C.c_int64]),
    "ccx_td_loss": (C.c_int, [_H, C.c_int64] + [C.c_void_p] * 9 + [C.c_float] * 2 + [C.c_void_p] * 3),
    "ccx_td_loss_backward": (C.c_int, [_H, C.c_int64] + [C.c_void_p] * 9 + [C.c_float] * 2 + [C.c_void_p] * 3),
    "ccx_replay_push": (C.c_int, [_H, C.c_int64] + [C.c_void_p] * 8 + [C.c_int64] + [C.c_void_p] * 8),
    "ccx_replay_sample": (C.c_int, [_H, C.c_int64] + [C.c_void_p] * 8 + [C.c_int64] + [C.c_void_p] * 8),
    "ccx_replay_fetch": (C.c_int, [_H, C.c_int64] + [C.c_void_p] * 8 + [C.c_int64] + [C.c_void_p] * 9),
    "ccx_prio_tree_words": (C.c_int64, [C.c_int64]),
    "ccx_prio_push": (C.c_int, [_H, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]),
    "ccx_prio_update": (C.c_int, [_H, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int32,
                                  C.POINTER(C.c_void_p), C.c_float, C.c_float]),
    "ccx_prio_sample": (C.c_int, [_H, C.c_int64] + [C.c_void_p] * 4 + [C.c_int64, C.c_int32] + [C.c_void_p] * 3),
    "ccx_nstep_push": (C.c_int, [_H, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]),
    "ccx_nstep_mark_cut": (C.c_int, [_H, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p]),
    "ccx_nstep_sample": (C.c_int, [_H, C.c_int64] + [C.c_void_p] * 9 + [C.c_int32, C.c_float, C.c_int64] + [C.c_void_p] * 10),
    "ccx_nstep_fetch": (C.c_int, [_H, C.c_int64] + [C.c_void_p] * 9 + [C.c_int32, C.c_float, C.c_int64] + [C.c_void_p] * 11),
    "ccx_td_loss_discounted": (C.c_int, [_H, C.c_int64] + [C.c_void_p] * 10 + [C.c_float] + [C.c_void_p] * 3),
    "ccx_td_loss_discounted_backward": (C.c_int, [_H, C.c_int64] + [C.c_void_p] * 10 + [C.c_float] + [C.c_void_p] * 3),
    "ccx_c51_workspace_bytes": (C.c_int64, [C.c_int64]),
    "ccx_c51_q_values": (C.c_int, [_H, C.c_int64, C.c_int32, C.c_float, C.c_float, C.c_void_p, C.c_void_p]),
    "ccx_c51_loss": (C.c_int, [_H, C.c_int64, C.c_int32, C.c_float, C.c_float] + [C.c_void_p] * 10 + [C.c_float] + [C.c_void_p] * 4),
    "ccx_c51_loss_backward": (C.c_int, [_H, C.c_int64, C.c_int32] + [C.c_void_p] * 8),
    "ccx_dueling_forward": (C.c_int, [_H, C.c_int64, C.c_int32, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p)]),
    "ccx_dueling_backward": (C.c_int, [_H, C.c_int64, C.c_void_p, C.c_void_p]),
    "ccx_mlp_q_actions": (C.c_int, [_H] + [C.c_int32] * 3 + [C.c_void_p] * 10),
    "ccx_sides_q_actions": (C.c_int, [_H] + [C.c_int32] * 3 + [C.c_void_p, C.c_int32, C.POINTER(CcxSlotGroup)] + [C.c_void_p] * 5),
    "ccx_minibatch_next": (C.c_int, [_H, C.c_int64, C.c_int32] + [C.c_void_p] * 9 + [C.c_int64] + [C.c_void_p] * 8),
    "ccx_minibatch_fetch": (C.c_int, [_H, C.c_int64, C.c_int32] + [C.c_void_p] * 8 + [C.c_int64] + [C.c_void_p] * 9),
    "ccx_minibatch_permutation": (C.c_int, [_H, C.c_int64, C.c_int64, C.c_void_p]),
    "ccx_set_check_inputs":(C.c_int, [_H, C.c_int32]),
    "ccx_check_inputs": (C.c_int, [_H]),
    "ccx_set_rng_seed": (C.c_int, [_H, C.c_uint64]),
    "ccx_set_policy_epsilon": (C.c_int, [_H, C.c_double]),
    "ccx_set_policy_stream": (C.c_int, [_H, C.c_int32, C.c_void_p, C.c_uint32]),
    "ccx_get_policy_stream": (C.c_int, [_H, C.POINTER(C.c_int32), C.c_void_p]),
    "ccx_zero_counters": (C.c_int, [_H]),
    "ccx_read_counters": (C.c_int, [_H, C.POINTER(CcxCounters)]),
    "ccx_counters_device_ptr": (C.c_int, [_H, C.POINTER(C.c_void_p)]),
    "ccx_rccl_unique_id": (C.c_int, [C.c_void_p]),
    "ccx_rccl_comm_create": (C.c_int, [C.c_int32, C.c_void_p, C.c_int32, C.c_int32, C.POINTER(C.c_void_p)]),
    "ccx_rccl_comm_destroy": (C.c_int, [C.c_void_p]),
    "ccx_rccl_allreduce_counters": (C.c_int, [_H, C.c_void_p, C.c_void_p, C.POINTER(C.c_int32)]),
    "ccx_set_timing": (C.c_int, [_H, C.c_int32]),
    "ccx_last_launch_ms": (C.c_int, [_H, C.POINTER(C.c_float)]),
    "ccx_set_launch_shape": (C.c_int, [_H, C.c_int32, C.c_int32]),
    "ccx_set_writers": (C.c_int, [_H, C.c_int32]),
    "ccx_set_store_throttle": (C.c_int, [_H, C.c_int32]),
    "ccx_set_step_pace": (C.c_int, [_H, C.c_int32]),
    "ccx_get_step_pace": (C.c_int, [_H, C.POINTER(C.c_float)]),
    "ccx_get_pace_state": (C.c_int, [_H, C.POINTER(C.c_float)]),
    "ccx_set_step_pace_start": (C.c_int, [_H, C.c_float]),
    "ccx_set_pace_calibration": (C.c_int, [_H, C.c_int32]),
    "ccx_get_pace_start": (C.c_int, [_H, C.POINTER(C.c_float), C.POINTER(C.c_int32), C.POINTER(C.c_float)]),
    "ccx_set_tunable": (C.c_int, [_H, C.c_char_p, C.c_int32]),
    "ccx_get_residency": (C.c_int, [_H, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "ccx_get_writer_shape": (C.c_int, [_H, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "ccx_get_step_shape": (C.c_int, [_H] + [C.POINTER(C.c_int32)] * 5),
    "ccx_set_reward_table": (C.c_int, [_H, C.c_void_p, C.c_void_p]),
    "ccx_set_terminated_table": (C.c_int, [_H, C.c_void_p, C.c_void_p]),
    "ccx_get_launch_shape": (C.c_int, [_H, C.POINTER(C.c_int32), C.POINTER(C.c_int32),
                                       C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "ccx_host_device_pointer": (C.c_int, [_H, C.c_void_p, C.POINTER(C.c_void_p)]),
    "ccx_set_stream": (C.c_int, [_H, C.c_void_p]),
    "ccx_synchronize": (C.c_int, [_H]),
}
