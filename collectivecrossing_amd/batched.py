"""Array-native batched environment: E independent CollectiveCrossing envs on one MI355X.

Thin Python over the C-ABI of libccx (``include/ccx.h``).  torch is used for plumbing only --
device buffers, the HIP stream, and (in :mod:`.sharding`) the RCCL process group; every compute
call goes through ``ctypes`` into the HIP library.  Layouts are the library's: env-major SoA,
``[E, N]`` per-agent arrays, observations ``[E, N, L]`` with ``L = 6 + 4N``.

The reference has no batched API; the per-env semantics are those of
``CollectiveCrossingEnv.reset/step`` (collectivecrossing.py:91-261).  The dict API of the
reference is layered on top of this class in :mod:`.env`.
"""

from __future__ import annotations

import contextlib
import ctypes as C
import json
import os
from dataclasses import dataclass
from pathlib import Path

import numpy as np
import torch

from . import _abi
from ._lib import check, load
from .configs import CollectiveCrossingConfig
from .learner import (MLP_ACTIVATIONS, EvalResult, GaeResult, LearnerOps, MlpGradResult, MlpHead,  # noqa: F401 (re-exported)
                      PpoLossResult, SampleResult, _EvaluateActions, _MlpForward, _PpoLoss, _require)
from .params import agent_ids, array_form_strategies, lower_config, position_only_tables
from .reset import build_reset_pool, seeded_positions


@dataclass
class StepResult:
    """Device tensors of one step (views into buffers owned by the env, overwritten next step)."""

    obs: torch.Tensor | None  # f32 [E, N, L]
    reward: torch.Tensor      # f64 [E, N]
    agent_flags: torch.Tensor  # u8 [E, N]  (_abi.AF_*)
    env_flags: torch.Tensor   # u8 [E]     (_abi.EF_*)
    obs_compact: torch.Tensor | None = None   # f32 [E, N, 4]  (x, y, type, active), CCX_OBS_COMPACT
    term_present: torch.Tensor | None = None  # u8 [E, N]: 1 where terminateds[id] exists (step_finish / array-form strategies)
    action_masks: torch.Tensor | None = None  # u8 [E, N]: legal actions of the state behind the step (want_masks; unpack_action_masks)
    final_obs: torch.Tensor | None = None     # f32 [E, N, L]: reset_obs="next": terminal rows of the envs with EF_RESET (other rows: untouched)
    final_compact: torch.Tensor | None = None  # f32 [E, N, 4]: likewise


@dataclass
class RolloutResult:
    obs: torch.Tensor | None   # f32 [K, E, N, L]
    reward: torch.Tensor | None  # f64 [K, E, N]
    agent_flags: torch.Tensor | None  # u8 [K, E, N]
    env_flags: torch.Tensor | None    # u8 [K, E]
    obs_compact: torch.Tensor | None = None   # f32 [K, E, N, 4], CCX_OBS_COMPACT
    term_present: torch.Tensor | None = None  # u8 [K, E, N]: batches with array-form strategies only
    final_obs: torch.Tensor | None = None     # f32 [K, E, N, L]: reset_obs="next": terminal rows at the (s, e) with EF_RESET (alloc_rollout(want_final=True))
    final_compact: torch.Tensor | None = None  # f32 [K, E, N, 4]: likewise; rows of (s, e) without EF_RESET are never written


@dataclass
class EpisodeStats:
    """Zero-copy device views of a batch's episode statistics (``ccx_episode_stats``, include/ccx.h CCX_EPISODE_STATS):
    they change with every tracked call.  ``ret`` / ``live_steps`` / ``steps`` belong to the episode in progress (``closed``
    = it has ended and the env has not been restarted), ``last_*`` to the most recent finished one (zero before the
    first), ``finished`` counts the finished episodes of every env since tracking was enabled."""

    ret: torch.Tensor              # f64 [E, N]
    live_steps: torch.Tensor       # i32 [E, N]
    steps: torch.Tensor            # i32 [E]
    closed: torch.Tensor           # u8  [E]
    finished: torch.Tensor         # i32 [E]
    last_ret: torch.Tensor         # f64 [E, N]
    last_live_steps: torch.Tensor  # i32 [E, N]
    last_steps: torch.Tensor       # i32 [E]
    last_end: torch.Tensor         # u8  [E]: EF_ALL_TERMINATED | EF_ALL_TRUNCATED of the step that ended it
    log_count: torch.Tensor        # i64 [2]: records stored, records dropped (the library's u64 pair)
    log_capacity: int


@dataclass
class FinishedEpisodes:
    """The stored records of the finished-episode log as NumPy arrays, in log order (:meth:`finished_episodes`)."""

    env: np.ndarray         # i64 [R]: GLOBAL env index (env_offset + e): logs of shards concatenate
    episode: np.ndarray     # i32 [R]: ordinal of the episode within its env since tracking was enabled
    steps: np.ndarray       # i32 [R]
    end: np.ndarray         # u8  [R]: 1 terminated, 2 truncated, 3 both
    ret: np.ndarray         # f64 [R, N]
    live_steps: np.ndarray  # i32 [R, N]
    dropped: int            # records that found the log full

    def __len__(self) -> int:
        return len(self.env)


def _check_cell_px(cell_px) -> int:
    """Pixels per grid cell of a rendered frame: an integer in 1..64 (ccx_render)."""
    if isinstance(cell_px, bool) or not isinstance(cell_px, (int, np.integer)) or not 1 <= int(cell_px) <= 64:
        raise ValueError(f"cell_px must be an integer in 1..64, got {cell_px!r}")
    return int(cell_px)


RESET_OBS_MODES = {"terminal": 0, "next": 1}   # CCX_RESET_OBS_TERMINAL / CCX_RESET_OBS_NEXT (include/ccx.h: CCX_RESET_OBS)
ACTION_MASK_WAIT_ONLY = 0x10   # the mask byte of an agent that is terminated or truncated


def unpack_action_masks(masks):
    """Mask bytes (``ccx_action_masks``: bit a = action a is legal, bit 4 = wait, always set) -> ``bool [..., 5]`` indexed
    by action id, for ``logits.masked_fill(~mask, -inf)``.  Takes a torch tensor (the result lives on its device) or
    anything numpy converts; needs no GPU.  On a device tensor it only launches kernels, so it captures into a graph."""
    if isinstance(masks, torch.Tensor):
        if masks.dtype is not torch.uint8:
            raise TypeError(f"action masks are uint8, got {masks.dtype}")
        # (built on the device, without a host-to-device copy: the call may sit inside a graph capture)
        one = torch.ones(5, dtype=torch.uint8, device=masks.device)
        bits = torch.bitwise_left_shift(one, torch.arange(5, dtype=torch.uint8, device=masks.device))
        return (masks.unsqueeze(-1) & bits) != 0
    arr = np.asarray(masks)
    if arr.dtype != np.uint8:
        raise TypeError(f"action masks are uint8, got {arr.dtype}")
    return (arr[..., None] & np.array([1, 2, 4, 8, 16], np.uint8)) != 0


def pack_action_masks(mask5) -> np.ndarray:
    """Inverse of :func:`unpack_action_masks` on the host: ``bool [..., 5]`` -> ``uint8 [...]``."""
    m = np.asarray(mask5.cpu() if isinstance(mask5, torch.Tensor) else mask5).astype(bool)
    if m.shape[-1:] != (5,):
        raise ValueError(f"expected [..., 5], got {m.shape}")
    return (m * np.array([1, 2, 4, 8, 16], np.uint8)).sum(-1).astype(np.uint8)


def scripted_slot_mask(config: CollectiveCrossingConfig, scripted) -> int:
    """Which agent slots a mixed-control step scripts, as the 64-bit mask of ``ccx_rollout_mixed`` (bit a = slot a,
    boarding slots first).  ``scripted`` is ``"exiting"``, ``"boarding"``, ``"all"``, an iterable of slot indices and / or
    agent ids (``"exiting_0"``), or an int mask.  Pure: needs no GPU.  Unknown ids, slots outside 0..N-1 and mask bits at
    or above N raise ``ValueError``."""
    nb, ne = int(config.num_boarding_agents), int(config.num_exiting_agents)
    n = nb + ne
    full = (1 << n) - 1
    if isinstance(scripted, str):
        sides = {"boarding": (1 << nb) - 1, "exiting": full & ~((1 << nb) - 1), "all": full}
        if scripted in sides:
            return sides[scripted]
        scripted = [scripted]                      # (one agent id)
    if isinstance(scripted, bool):
        raise ValueError(f"scripted must name agent slots, got {scripted!r}")
    if isinstance(scripted, (int, np.integer)):
        mask = int(scripted)
        if mask < 0 or mask & ~full:
            raise ValueError(f"scripted mask {mask:#x} has bits outside the {n} agent slots")
        return mask
    try:
        items = list(scripted)
    except TypeError:
        raise ValueError(f"scripted must be 'exiting', 'boarding', 'all', slot indices / agent ids or an int mask, "
                         f"got {scripted!r}") from None
    ids = {aid: i for i, aid in enumerate(agent_ids(config))}
    mask = 0
    for it in items:
        if isinstance(it, str):
            if it not in ids:
                raise ValueError(f"unknown agent id {it!r}")
            slot = ids[it]
        elif isinstance(it, (int, np.integer)) and not isinstance(it, bool):
            slot = int(it)
            if not 0 <= slot < n:
                raise ValueError(f"agent slot {slot} outside 0..{n - 1}")
        else:
            raise ValueError(f"scripted entries are slot indices or agent ids, got {it!r}")
        mask |= 1 << slot
    return mask


def _ptr(t: torch.Tensor | None) -> C.c_void_p:
    return C.c_void_p(None if t is None else t.data_ptr())


def _result_tensors(res) -> list:
    """The tensors of a StepResult / RolloutResult (``None``: none)."""
    return [] if res is None else [v for v in vars(res).values() if isinstance(v, torch.Tensor)]


class BatchedCollectiveCrossing(LearnerOps):
    """E envs sharing one config, resident on one GPU for their whole life.

    Every method that enqueues device work keeps the stream-order contract stated in :class:`LearnerOps` (DESIGN.md
    3.18): launches go to the handle's stream, ordered behind what torch's current stream held before the call and in
    front of what it gets afterwards, at no cost when the two are the same stream.  Outside it, because they synchronise
    with the host: ``reset``, ``reset_host``, ``make_reset_pool``, ``set_state`` / ``get_state``, ``counters``,
    ``finished_episodes``, ``track_episodes``, ``check_inputs``, ``policy_stream_state``, ``set_policy_stream``, the
    table setters, the pace queries, ``use_stream``, ``synchronize`` and ``close``."""

    def __init__(self, config: CollectiveCrossingConfig, num_envs: int, device: int | str | None = None,
                 env_offset: int = 0, total_envs: int | None = None, check_inputs: bool | None = None):
        self._lib = load()
        self.config = config
        # (position-only user strategies -- strategies.RewardFunction.position_only -- run inside the kernels as tables)
        # (array-form user strategies -- strategies.ARRAY_METHODS -- run between the halves of the split step)
        self.params = lower_config(config, allow_position_only=True, allow_array_form=True)
        self._user_tables = position_only_tables(config)
        self._array_strategies = array_form_strategies(config)
        self._view = None
        self._finish_cache: dict = {}
        self._term_present: torch.Tensor | None = None
        self.num_envs = int(num_envs)
        self.num_agents = self.params.num_agents
        self.obs_len = 6 + 4 * self.num_agents
        self.agent_ids = agent_ids(config)
        self.env_offset = int(env_offset)
        self.total_envs = int(total_envs if total_envs is not None else num_envs)
        if not torch.cuda.is_available():
            raise RuntimeError("collectivecrossing_amd needs an MI355X: torch sees no GPU and libccx "
                               "has no CPU path")
        dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        if dev.type != "cuda":
            raise ValueError(f"device must be a GPU, got {dev}")
        self.device = torch.device("cuda", dev.index if dev.index is not None else torch.cuda.current_device())
        self._stream = torch.cuda.current_stream(self.device)
        self._stream_raw = self._stream.cuda_stream
        handle = C.c_void_p()
        check(self._lib.ccx_create(C.byref(self.params), self.num_envs, self.env_offset, self.total_envs,
                                   self.device.index, C.c_void_p(self._stream.cuda_stream),
                                   C.byref(handle)))
        self._h = handle
        self._pool: torch.Tensor | None = None
        self._step_bufs: StepResult | None = None
        self._step_out_cache: dict = {}
        self._masks_buf: torch.Tensor | None = None      # u8 [E, N] behind StepResult.action_masks
        self._masks_bound = 0                            # the pointer ccx_bind_action_masks holds (0 = none)
        self._reset_obs_mode = 0                         # what ccx_set_reset_obs holds
        self._final_bound = (0, 0)                       # the pointers ccx_bind_final_obs holds
        self._final_keep: list = [None, None]            # ... and the tensors behind them, alive while bound
        self._final_bufs: list = [None, None]            # f32 [E, N, L] / [E, N, 4] behind StepResult.final_* (step_finish)
        self._rollouts_with_obs = 0
        self._tracking = False                           # track_episodes: every result-producing call updates the stats
        self._stats_view: EpisodeStats | None = None
        self._stats_raw = None
        if check_inputs is None:
            check_inputs = os.environ.get("CCX_CHECK_INPUTS", "0") not in ("", "0")
        if check_inputs:
            self.set_check_inputs(True)
        rew, term = self._user_tables
        if term is not None:
            self.set_terminated_table(*term)
        if rew is not None:
            self.set_reward_table(*rew)
        self._apply_pace_memory()

    # ------------------------------------------------------------------ lifetime
    def close(self) -> None:
        if getattr(self, "_h", None):
            try:
                self._remember_pace()
            except Exception:
                pass
            self._lib.ccx_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ------------------------------------------------------------------ helpers
    def _new(self, shape, dtype) -> torch.Tensor:
        return torch.empty(shape, dtype=dtype, device=self.device)

    def _as_dev_u8(self, a, shape, cur=False) -> torch.Tensor:
        """``a`` as a contiguous u8 device tensor of ``shape``, ordered in front of the launch.  ``cur``: what
        :meth:`_other_stream` answered earlier in the same call (``None``: the streams are the same, nothing to order)."""
        if isinstance(a, torch.Tensor):
            # (fast path first: a step-wise loop hands over a ready device tensor every few microseconds)
            t = a if (a.dtype is torch.uint8 and a.device == self.device) else a.to(device=self.device, dtype=torch.uint8)
        else:
            t = torch.from_numpy(np.ascontiguousarray(a, np.uint8)).to(self.device)
        if tuple(t.shape) != tuple(shape):
            raise ValueError(f"expected shape {tuple(shape)}, got {tuple(t.shape)}")
        if not t.is_contiguous():
            t = t.contiguous()
        if cur is not None:
            self._order_after_current_stream(t, cur=cur)
        return t

    def _order_after_current_stream(self, *tensors, cur=False):
        """The entry of every enqueueing method (rules (a) and (c) of the stream-order contract, :class:`LearnerOps`).  The
        library launches on the stream captured at construction (or `use_stream`).  Inputs are produced / copied on
        torch's CURRENT stream, and earlier work there may still read or write the outputs: when that is another stream,
        make the launch stream wait for it and tell the caching allocator that the launch stream uses the buffers
        (otherwise nothing orders the H2D copy before the kernel, and a temporary could be recycled while the kernel still
        reads it).  ``tensors``: everything the launch touches, outputs included.  ``cur``: what :meth:`_other_stream`
        answered earlier in the same call (default: ask now); returns it for the exit, :meth:`_current_stream_waits`."""
        if cur is False:
            cur = self._other_stream()                                   # (one raw read: this is the per-step path)
        if cur is not None:
            self._stream.wait_stream(cur)
            for t in tensors:
                if t is not None and t.is_cuda:
                    t.record_stream(self._stream)
        return cur

    # ------------------------------------------------------------------ state
    def set_state(self, x=None, y=None, active=None, terminated=None, truncated=None,
                  step_count=None, episode=None) -> None:
        """Overwrite (parts of) the SoA state from host arrays (``ccx_set_state_host``)."""
        E, N = self.num_envs, self.num_agents
        keep = []

        def conv(a, dt, shape):
            if a is None:
                return None
            arr = np.ascontiguousarray(np.asarray(a, dt).reshape(shape))
            keep.append(arr)
            return arr.ctypes.data

        st = _abi.CcxState(conv(x, np.int32, (E, N)), conv(y, np.int32, (E, N)),
                           conv(active, np.uint8, (E, N)), conv(terminated, np.uint8, (E, N)),
                           conv(truncated, np.uint8, (E, N)), conv(step_count, np.int32, (E,)),
                           conv(episode, np.int32, (E,)))
        check(self._lib.ccx_set_state_host(self._h, C.byref(st)))

    def get_state(self) -> dict[str, np.ndarray]:
        E, N = self.num_envs, self.num_agents
        out = dict(x=np.empty((E, N), np.int32), y=np.empty((E, N), np.int32),
                   active=np.empty((E, N), np.uint8), terminated=np.empty((E, N), np.uint8),
                   truncated=np.empty((E, N), np.uint8), step_count=np.empty((E,), np.int32),
                   episode=np.empty((E,), np.int32))
        st = _abi.CcxState(*[out[k].ctypes.data for k in
                             ("x", "y", "active", "terminated", "truncated", "step_count", "episode")])
        check(self._lib.ccx_get_state_host(self._h, C.byref(st)))
        return out

    # ------------------------------------------------------------------ reset
    def reset(self, seeds, env_mask=None) -> torch.Tensor:
        """``reset(seed=seeds[e])`` for every (masked) env ON THE DEVICE (``ccx_reset_seeded``:
        numpy's SeedSequence -> PCG64 -> bounded-integer stream and the reference's rejection
        sampling, bit-identical); returns the observations [E,N,L]."""
        if isinstance(seeds, torch.Tensor):
            s = seeds.to(device=self.device).view(-1)
            s = s.view(torch.int64) if s.dtype == torch.uint64 else s.to(torch.int64)
        else:
            s = torch.from_numpy(np.asarray(seeds, dtype=np.uint64).reshape(-1).view(np.int64)).to(self.device)
        if s.numel() != self.num_envs:
            raise ValueError(f"need {self.num_envs} seeds, got {s.numel()}")
        m = None if env_mask is None else self._as_dev_u8(env_mask, (self.num_envs,), cur=None)
        s = s.contiguous()
        self._enqueue(self._lib.ccx_reset_seeded, s, m)
        return self.observe()

    def reset_host(self, seeds) -> torch.Tensor:
        """Same placements computed with numpy on the host (``reset.py``) and uploaded."""
        seeds = np.asarray(seeds).reshape(-1)
        if len(seeds) != self.num_envs:
            raise ValueError(f"need {self.num_envs} seeds, got {len(seeds)}")
        pos = seeded_positions(self.config, seeds)
        E, N = self.num_envs, self.num_agents
        self.set_state(x=pos[..., 0], y=pos[..., 1], active=np.ones((E, N), np.uint8),
                       terminated=np.zeros((E, N), np.uint8), truncated=np.zeros((E, N), np.uint8),
                       step_count=np.zeros(E, np.int32))
        return self.observe()

    def set_reset_pool(self, pool_xy) -> None:
        """Install seeded placements ``u8 [P, N, 2]`` for ``reset_from_pool`` / auto-reset."""
        if isinstance(pool_xy, torch.Tensor):
            t = pool_xy.to(device=self.device, dtype=torch.uint8).contiguous()
        else:
            t = torch.from_numpy(np.ascontiguousarray(pool_xy, np.uint8)).to(self.device)
        if t.ndim != 3 or tuple(t.shape[1:]) != (self.num_agents, 2):
            raise ValueError(f"pool must be [P, {self.num_agents}, 2], got {tuple(t.shape)}")
        self._pool = t
        self._order_after_current_stream(t)                  # (copied on the current stream, read by later launches)
        check(self._lib.ccx_set_reset_pool(self._h, _ptr(t), t.shape[0]))

    def make_reset_pool(self, seed0: int, size: int, on_device: bool = True) -> None:
        """Pool of ``reset(seed=seed0 + p)`` placements, p < size; generated on the GPU by default
        (``ccx_fill_reset_pool_seeded``), or with numpy on the host."""
        if not on_device:
            self.set_reset_pool(build_reset_pool(self.config, seed0, size))
            return
        t = self._new((size, self.num_agents, 2), torch.uint8)
        self._enqueue(self._lib.ccx_fill_reset_pool_seeded, t, size, seed0)
        self._pool = t
        check(self._lib.ccx_set_reset_pool(self._h, _ptr(t), size))

    def reset_pool(self) -> torch.Tensor | None:
        return self._pool

    def reset_from_pool(self, env_mask=None) -> None:
        m = None if env_mask is None else self._as_dev_u8(env_mask, (self.num_envs,), cur=None)
        self._enqueue(self._lib.ccx_reset_from_pool, m)      # (the state: strategy_view / episode_stats readers)

    # ------------------------------------------------------------------ scripted policy
    def policy_actions(self, policy: str = "greedy", out: torch.Tensor | None = None) -> torch.Tensor:
        """``GreedyPolicy`` / ``WaitingPolicy`` action of every live agent for the current state, u8 [E, N]
        (255 for agents that are terminated or truncated) -- ``ccx_policy_actions``; epsilon 0 unless
        :meth:`set_policy_epsilon` is in effect (then the same draws as inside ``rollout_policy``)."""
        if out is None:
            out = self._new((self.num_envs, self.num_agents), torch.uint8)
        self._enqueue(self._lib.ccx_policy_actions, _abi.POLICIES[policy], out)
        return out

    def greedy_actions(self, out: torch.Tensor | None = None) -> torch.Tensor:
        """``GreedyPolicy(epsilon=0)`` for every live agent (``ccx_greedy_actions``; never explores)."""
        if out is None:
            out = self._new((self.num_envs, self.num_agents), torch.uint8)
        self._enqueue(self._lib.ccx_greedy_actions, out)
        return out

    # ------------------------------------------------------------------ legal-action masks
    def _check_masks(self, t) -> torch.Tensor:
        E, N = self.num_envs, self.num_agents
        if not isinstance(t, torch.Tensor) or t.dtype is not torch.uint8 or t.device != self.device:
            raise ValueError(f"action masks go to a torch.uint8 tensor on {self.device}")
        if tuple(t.shape) != (E, N) or not t.is_contiguous():
            raise ValueError(f"action masks need a contiguous tensor of shape {(E, N)}, got {tuple(t.shape)}")
        return t

    def _bind_masks(self, t: torch.Tensor | None) -> None:
        """While a tensor is bound every launch that advances the state leaves the masks of its final state there
        (``ccx_bind_action_masks``); only a CHANGE of the pointer reaches the library (this is on the per-step path)."""
        ptr = 0 if t is None else t.data_ptr()
        if ptr != self._masks_bound:
            check(self._lib.ccx_bind_action_masks(self._h, C.c_void_p(ptr or None)))
            self._masks_bound = ptr

    def _step_masks(self, want_masks: bool) -> None:
        if want_masks and self._masks_buf is None:
            self._masks_buf = self._new((self.num_envs, self.num_agents), torch.uint8)
        self._bind_masks(self._masks_buf if want_masks else None)

    def action_masks(self, out: torch.Tensor | None = None) -> torch.Tensor:
        """Legal actions of every agent slot in the CURRENT state, u8 [E, N] (``ccx_action_masks``): bit a = action a
        would move the agent (the reference's ``_is_valid_action``: bounds, walls, door row, no other active agent on the
        target), bit 4 = wait, always set; 0x10 for agents that are terminated or truncated.
        :func:`unpack_action_masks` turns the bytes into ``bool [E, N, 5]``.  Only enqueues (no host synchronisation)."""
        out = self._new((self.num_envs, self.num_agents), torch.uint8) if out is None else self._check_masks(out)
        self._enqueue(self._lib.ccx_action_masks, out)
        return out

    def masks_fused(self, num_steps: int = 1, order: bool = False, mixed: bool = False) -> bool:
        """Whether such a call writes its masks from the step's own launch (``ccx_get_masks_fused``) -- one env-step
        without a move order on a handle whose short launches take the step kernel -- or is followed by the stand-alone
        mask kernel on the same stream.  The bytes are the same either way."""
        v = C.c_int32()
        check(self._lib.ccx_get_masks_fused(self._h, int(num_steps), int(bool(order)), int(bool(mixed)), C.byref(v)))
        return bool(v.value)

    # ------------------------------------------------------------------ reset-observation mode
    def _reset_obs(self, mode: str, final_obs: torch.Tensor | None = None, final_compact: torch.Tensor | None = None,
                   like=(None, None)) -> None:
        """Select what the rows of a restarted env hold for the next call (``ccx_set_reset_obs``) and bind the side buffers
        of its terminal rows (``ccx_bind_final_obs``); only CHANGES reach the library (this is on the per-step path)."""
        try:
            m = RESET_OBS_MODES[mode]
        except (KeyError, TypeError):
            raise ValueError(f"reset_obs must be 'terminal' or 'next', got {mode!r}") from None
        if m != self._reset_obs_mode:
            check(self._lib.ccx_set_reset_obs(self._h, m))
            self._reset_obs_mode = m
        # The mode and the two pointers are STICKY on the handle (include/ccx.h) and only the paths that take `reset_obs=`
        # refresh them: every such call rebinds (a "terminal" call unbinds), and the batch holds the bound tensors
        # (_final_keep) so that the handle never keeps a pointer into freed memory.  A new caller of ccx_step_finish /
        # ccx_rollout_mixed / ccx_rollout with auto_reset=1 must come through here first.
        ptrs, keep = [0, 0], [None, None]
        if m:
            for n, (t, ref, name) in enumerate(((final_obs, like[0], "final_obs"), (final_compact, like[1], "final_compact"))):
                if t is None or ref is None:
                    continue
                _require(name, t, torch.float32, ref.shape, self.device)
                ptrs[n], keep[n] = t.data_ptr(), t
        self._final_keep = keep
        if tuple(ptrs) != self._final_bound:
            check(self._lib.ccx_bind_final_obs(self._h, C.c_void_p(ptrs[0] or None), C.c_void_p(ptrs[1] or None)))
            self._final_bound = tuple(ptrs)

    def _reset_obs_out(self, mode: str, out) -> None:
        if out is None:
            self._reset_obs(mode)
        else:
            self._reset_obs(mode, out.final_obs, out.final_compact, (out.obs, out.obs_compact))

    @contextlib.contextmanager
    def _rollout_call(self, K, auto_reset, out, want_traj, want_obs, want_compact, reset_obs, check_pool=False, cur=False,
                      extra=()):
        """Head and tail of every rollout wrapper.  Before the call: the pool an auto-reset needs (``check_pool``; the other
        wrappers leave that refusal to the library), the refusal of a tracked call without a trajectory, the result
        (allocated unless the caller's, ``None`` without a trajectory), the reset-observation mode with that result's
        side buffers, and the entry of the stream-order contract over the result and ``extra`` (the other outputs).
        Yields ``(result, byref of its CcxRolloutOut or None)``; behind the body the tracked update and the exit."""
        if check_pool and auto_reset and self._pool is None:
            raise ValueError("auto_reset needs a reset pool (set_reset_pool / make_reset_pool)")
        self._track_check(out, want_traj)
        if out is None and want_traj:
            out = self.alloc_rollout(K, want_obs, want_compact)
        self._reset_obs_out(reset_obs, out)
        if cur is not None:
            cur = self._order_after_current_stream(*_result_tensors(out), *extra, cur=cur)
        ro = None if out is None else C.byref(_abi.CcxRolloutOut(
            _ptr(out.obs).value, _ptr(out.reward).value, _ptr(out.agent_flags).value, _ptr(out.env_flags).value,
            _ptr(out.obs_compact).value))
        yield out, ro
        if self._tracking:
            self._track(K, out)
        if cur is not None:
            self._current_stream_waits(cur=cur)

    def step_final_buffers(self, want_obs: bool = True, want_compact: bool = False):
        """The batch's own one-step side buffers ``(final_obs f32 [E, N, L], final_compact f32 [E, N, 4])`` that
        ``step_finish(reset_obs="next", want_final=True)`` fills at restarted envs and hands out as
        ``StepResult.final_obs`` / ``final_compact`` (``None`` where not asked for here or earlier).  Allocated (zeroed) on
        first use; rows of envs without ``EF_RESET`` are never written, so whatever the caller puts there stays."""
        E, N = self.num_envs, self.num_agents
        if want_obs and self._final_bufs[0] is None:
            self._final_bufs[0] = self._new((E, N, self.obs_len), torch.float32).zero_()
        if want_compact and self._final_bufs[1] is None:
            self._final_bufs[1] = self._new((E, N, 4), torch.float32).zero_()
        return tuple(self._final_bufs)

    def reset_obs_fused(self, num_steps: int = 1, order: bool = False, mixed: bool = False) -> bool:
        """Whether such a call with ``reset_obs="next"`` redirects the rows of restarted envs inside the step's own launch
        (``ccx_get_reset_obs_fused``) -- one env-step from an action tensor without a move order on a batch whose short
        launches take the step kernel -- or is followed by the fix-up kernel on the same stream.  Same bytes either way."""
        v = C.c_int32(0)
        check(self._lib.ccx_get_reset_obs_fused(self._h, int(num_steps), int(bool(order)), int(bool(mixed)), C.byref(v)))
        return bool(v.value)

    # ------------------------------------------------------------------ episode statistics
    def track_episodes(self, log_capacity: int | bool = 0) -> None:
        """Episode returns and lengths on the device (``ccx_episode_stats_enable``, include/ccx.h CCX_EPISODE_STATS).
        From now on every call that hands out rewards and flags -- ``step``, ``step_mixed``, ``step_finish``, ``rollout``,
        ``rollout_mixed``, ``rollout_greedy`` / ``rollout_policy``, also on batches with array-form strategies -- is followed
        by the update kernel on the buffers it hands out, on the handle's stream; a call that writes no trajectory
        (``want_traj=False`` without ``out``) raises ``ValueError``.  ``log_capacity`` > 0 also keeps a log of that many
        finished episodes (:meth:`finished_episodes`).  Calling it again starts from zero; ``track_episodes(False)`` turns
        tracking off.  Synchronous."""
        self._stats_view = self._stats_raw = None
        if log_capacity is False:
            if self._tracking:
                self._tracking = False
                check(self._lib.ccx_episode_stats_disable(self._h))
            return
        cap = 0 if log_capacity is True else int(log_capacity)
        if cap < 0:
            raise ValueError(f"log_capacity must be >= 0, got {log_capacity!r}")
        check(self._lib.ccx_episode_stats_enable(self._h, cap))
        self._tracking = True

    def _need_tracking(self) -> None:
        if not self._tracking:
            raise RuntimeError("episode statistics are not tracked: call track_episodes() first")

    def _stats_struct(self):
        if self._stats_raw is None:
            self._need_tracking()
            raw = _abi.CcxEpisodeStats()
            check(self._lib.ccx_episode_stats_view(self._h, C.byref(raw)))
            self._stats_raw = raw
        return self._stats_raw

    def _dev_view(self, ptr, count, typestr, dtype, shape) -> torch.Tensor:
        return torch.as_tensor(_CudaArrayView(ptr, count, typestr), device=self.device).view(dtype).view(shape)

    def episode_stats(self) -> EpisodeStats:
        """:class:`EpisodeStats`: zero-copy views of the handle's own buffers (valid until tracking is turned off or
        enabled again).  Reading them needs the handle's stream to be done (``synchronize()``, or work on that stream)."""
        if self._stats_view is None:
            v = self._stats_struct()
            E, N = self.num_envs, self.num_agents
            en, dv = E * N, self._dev_view
            self._stats_view = EpisodeStats(
                dv(v.ret, en, "<f8", torch.float64, (E, N)), dv(v.live_steps, en, "<i4", torch.int32, (E, N)),
                dv(v.steps, E, "<i4", torch.int32, (E,)), dv(v.closed, E, "|u1", torch.uint8, (E,)),
                dv(v.finished, E, "<i4", torch.int32, (E,)), dv(v.last_ret, en, "<f8", torch.float64, (E, N)),
                dv(v.last_live_steps, en, "<i4", torch.int32, (E, N)), dv(v.last_steps, E, "<i4", torch.int32, (E,)),
                dv(v.last_end, E, "|u1", torch.uint8, (E,)), dv(v.log_count, 2, "<i8", torch.int64, (2,)),
                int(v.log_capacity))
        return self._stats_view

    def episode_stats_launches(self) -> int:
        """Kernels one update enqueues (``ccx_episode_stats_launches``): 1 without a log, 3 with one."""
        n = C.c_int32()
        check(self._lib.ccx_episode_stats_launches(self._h, C.byref(n)))
        return int(n.value)

    def update_episode_stats(self, reward: torch.Tensor, agent_flags: torch.Tensor, env_flags: torch.Tensor) -> None:
        """Feed a trajectory the caller holds (``ccx_episode_stats_update``): ``reward`` f64 [K, E, N], ``agent_flags`` u8
        [K, E, N], ``env_flags`` u8 [K, E] (or one step without the leading axis), contiguous device tensors.  Only
        enqueues (no host synchronisation)."""
        self._need_tracking()
        E, N = self.num_envs, self.num_agents
        for name, t, dt in (("reward", reward, torch.float64), ("agent_flags", agent_flags, torch.uint8),
                            ("env_flags", env_flags, torch.uint8)):
            _require(name, t, dt, None, self.device)
        if reward.dim() == 2:
            reward, agent_flags, env_flags = reward[None], agent_flags[None], env_flags[None]
        K = int(reward.shape[0]) if reward.dim() == 3 else 0
        if K < 1 or tuple(reward.shape) != (K, E, N) or tuple(agent_flags.shape) != (K, E, N) or tuple(env_flags.shape) != (K, E):
            raise ValueError(f"expected reward / agent_flags [K, {E}, {N}] and env_flags [K, {E}], got {tuple(reward.shape)}, "
                             f"{tuple(agent_flags.shape)}, {tuple(env_flags.shape)}")
        self._enqueue(self._lib.ccx_episode_stats_update, K, reward, agent_flags, env_flags)

    def _track(self, K: int, res) -> None:
        """The update behind a tracked call, on the buffers that call hands out."""
        if res is None or res.reward is None or res.agent_flags is None or res.env_flags is None:
            raise ValueError("episode statistics are tracked (track_episodes): this call must write rewards and flags "
                             "(want_traj=True, or an `out` with reward, agent_flags and env_flags)")
        check(self._lib.ccx_episode_stats_update(self._h, K, res.reward.data_ptr(), res.agent_flags.data_ptr(),
                                                 res.env_flags.data_ptr()))

    def _track_check(self, out, want_traj: bool) -> None:
        """Refuse BEFORE the state advances: a tracked call without a trajectory would lose its steps."""
        if self._tracking and ((out is None and not want_traj) or
                               (out is not None and (out.reward is None or out.agent_flags is None or out.env_flags is None))):
            raise ValueError("episode statistics are tracked (track_episodes): this call must write rewards and flags "
                             "(want_traj=True, or an `out` with reward, agent_flags and env_flags)")

    def reset_episode_stats(self, env_mask=None) -> None:
        """Forget the episode in progress of the masked envs (all by default): running return, lengths and the latch go
        to zero; no record is written, ``finished`` and ``last_*`` stay (``ccx_episode_stats_reset``).  ``reset`` and
        ``reset_from_pool`` do this for the envs they restart.  Only enqueues."""
        self._need_tracking()
        m = None if env_mask is None else self._as_dev_u8(env_mask, (self.num_envs,), cur=None)
        self._enqueue(self._lib.ccx_episode_stats_reset, m)  # (readers of the episode_stats views)

    def finished_episodes(self, clear: bool = True) -> FinishedEpisodes:
        """Synchronise and return the stored records of the log (:class:`FinishedEpisodes`; needs
        ``track_episodes(log_capacity > 0)``).  One update's records follow those of earlier updates in env-major order.
        ``clear=True`` empties the log afterwards (``ccx_episode_log_clear``)."""
        v = self._stats_struct()
        cap, N = int(v.log_capacity), self.num_agents
        if cap <= 0:
            raise RuntimeError("no finished-episode log: call track_episodes(log_capacity=...) with a capacity")
        self.synchronize()
        stored, dropped = (int(x) for x in self.episode_stats().log_count.cpu().numpy())
        dv = self._dev_view

        def host(ptr, count, typestr, dtype, shape):
            return dv(ptr, count, typestr, dtype, shape)[:stored].cpu().numpy()

        rec = FinishedEpisodes(host(v.log_env, cap, "<i8", torch.int64, (cap,)), host(v.log_episode, cap, "<i4", torch.int32, (cap,)),
                               host(v.log_steps, cap, "<i4", torch.int32, (cap,)), host(v.log_end, cap, "|u1", torch.uint8, (cap,)),
                               host(v.log_ret, cap * N, "<f8", torch.float64, (cap, N)),
                               host(v.log_live_steps, cap * N, "<i4", torch.int32, (cap, N)), dropped)
        if clear:
            self.clear_episode_log()
        return rec

    def clear_episode_log(self) -> None:
        """Empty the finished-episode log: stored = dropped = 0 (``ccx_episode_log_clear``).  Only enqueues."""
        self._need_tracking()
        self._enqueue(self._lib.ccx_episode_log_clear)

    # ------------------------------------------------------------------ compute
    def observe(self, out: torch.Tensor | None = None) -> torch.Tensor:
        if out is None:
            out = self._new((self.num_envs, self.num_agents, self.obs_len), torch.float32)
        self._enqueue(self._lib.ccx_observe, out)
        return out

    def step(self, actions, order=None, want_obs: bool = True, want_compact: bool = False,
             want_masks: bool = False) -> StepResult:
        """One env-step (``ccx_step``).  ``want_masks``: ``StepResult.action_masks`` (u8 [E, N]) holds the legal actions
        of the state BEHIND the step, written by the same launch where :meth:`masks_fused` says so."""
        # (_other_stream, inline: the raw stream is read once per call and the answer shared, so the same-stream path --
        # a few microseconds of Python per step -- makes no other call into torch and pays no call for asking)
        cur = (None if torch._C._cuda_getCurrentRawStream(self.device.index) == self._stream_raw
               else torch.cuda.current_stream(self.device))
        self._step_masks(want_masks)
        if self._array_strategies:
            res = self._step_array(actions, order, want_obs, want_compact, cur=cur)
            if self._tracking:
                self._track(1, res)
            if cur is not None:
                self._current_stream_waits(self._masks_buf if want_masks else None, cur=cur)
            return res if not want_masks else StepResult(res.obs, res.reward, res.agent_flags, res.env_flags, res.obs_compact,
                                                         res.term_present, self._masks_buf)
        E, N = self.num_envs, self.num_agents
        a = self._as_dev_u8(actions, (E, N), cur)
        o = None if order is None else self._as_dev_u8(order, (E, N), cur)
        cached = self._step_out(_abi.CcxStepOut, want_obs, want_compact, want_masks)
        if cur is not None:                  # (buffers allocated just now, and earlier readers of the static ones)
            self._order_after_current_stream(*_result_tensors(cached[2]), cur=cur)
        check(self._lib.ccx_step(self._h, a.data_ptr(), None if o is None else o.data_ptr(), cached[1]))
        if self._tracking:
            self._track(1, cached[2])
        if cur is not None:
            self._current_stream_waits(cur=cur)
        return cached[2]

    def _step_out(self, struct, want_obs, want_compact, want_masks=False):
        """(output struct, its byref, StepResult) over the env's static one-step buffers, built once per struct type and
        output selection -- this is the per-step path of a policy-in-the-loop caller, a few microseconds end to end."""
        key = (struct, bool(want_obs), bool(want_compact), bool(want_masks))
        cached = self._step_out_cache.get(key)
        if cached is None:
            b = self._step_buffers(want_compact)
            so = struct(_ptr(b.obs if want_obs else None).value, _ptr(b.reward).value,
                        _ptr(b.agent_flags).value, _ptr(b.env_flags).value,
                        _ptr(b.obs_compact if want_compact else None).value)
            cached = (so, C.byref(so), StepResult(b.obs if want_obs else None, b.reward, b.agent_flags, b.env_flags,
                                                  b.obs_compact if want_compact else None,
                                                  action_masks=self._masks_buf if want_masks else None))
            self._step_out_cache[key] = cached
        return cached

    def _step_buffers(self, want_compact) -> StepResult:
        """The env's static one-step output buffers, allocated on first use (the compact rows when first asked for)."""
        E, N = self.num_envs, self.num_agents
        if self._step_bufs is None:
            self._step_bufs = StepResult(self._new((E, N, self.obs_len), torch.float32), self._new((E, N), torch.float64),
                                         self._new((E, N), torch.uint8), self._new((E,), torch.uint8))
        if want_compact and self._step_bufs.obs_compact is None:
            self._step_bufs.obs_compact = self._new((E, N, 4), torch.float32)
        return self._step_bufs

    # ------------------------------------------------------------------ mixed control
    def _mixed_args(self, scripted, policy):
        if self._array_strategies:
            raise NotImplementedError("mixed-control steps are not combined with array-form strategy classes (the split "
                                      "step): use policy_actions + step on such a batch")
        if policy not in ("greedy", "waiting"):
            raise ValueError(f"a mixed-control step scripts 'greedy' or 'waiting', got {policy!r}")
        return scripted_slot_mask(self.config, scripted), _abi.POLICIES[policy]

    def step_mixed(self, actions, scripted, policy: str = "greedy", order=None, want_obs: bool = True,
                   want_compact: bool = False, actions_out: torch.Tensor | None = None,
                   want_masks: bool = False) -> StepResult:
        """One step in which the ``scripted`` slots (:func:`scripted_slot_mask`) take the on-device ``policy``'s action
        and the others the bytes of ``actions`` -- ``policy_actions`` + ``torch.where`` + ``step`` in ONE launch
        (``ccx_rollout_mixed``).  Bytes of ``actions`` in scripted slots are ignored; ``actions`` may be ``None`` when every
        slot is scripted; ``actions_out`` (u8 [E, N]) receives the merged actions.  Returns the views :meth:`step` returns;
        ``want_masks`` as for :meth:`step`."""
        mask, pol = self._mixed_args(scripted, policy)
        self._step_masks(want_masks)
        E, N = self.num_envs, self.num_agents
        if actions is None and mask != (1 << N) - 1:
            raise ValueError("actions may be None only when every slot is scripted")
        cur = self._other_stream()
        a = None if actions is None else self._as_dev_u8(actions, (E, N), cur)
        o = None if order is None else self._as_dev_u8(order, (E, N), cur)
        if actions_out is not None:
            self._check_actions_out(actions_out, (E, N))
        cached = self._step_out(_abi.CcxRolloutOut, want_obs, want_compact, want_masks)
        if cur is not None:
            self._order_after_current_stream(*_result_tensors(cached[2]), actions_out, cur=cur)
        check(self._lib.ccx_rollout_mixed(self._h, 1, pol, mask, None if a is None else a.data_ptr(),
                                          None if o is None else o.data_ptr(), 0, cached[1],
                                          None if actions_out is None else actions_out.data_ptr()))
        if self._tracking:
            self._track(1, cached[2])
        if cur is not None:
            self._current_stream_waits(cur=cur)
        return cached[2]

    def _check_actions_out(self, t, shape) -> None:
        if not isinstance(t, torch.Tensor) or t.dtype is not torch.uint8 or t.device != self.device:
            raise ValueError(f"actions_out must be a torch.uint8 tensor on {self.device}")
        if tuple(t.shape) != tuple(shape) or not t.is_contiguous():
            raise ValueError(f"actions_out must be contiguous with shape {tuple(shape)}, got {tuple(t.shape)}")

    def rollout_mixed(self, actions, scripted, policy: str = "greedy", order=None, auto_reset: bool = False,
                      out: RolloutResult | None = None, actions_out: torch.Tensor | None = None, num_steps: int | None = None,
                      want_obs: bool = True, want_traj: bool = True, want_compact: bool = False,
                      masks_out: torch.Tensor | None = None, reset_obs: str = "terminal") -> RolloutResult | None:
        """K mixed-control steps (``ccx_rollout_mixed``; launches of at most 16 steps): ``actions`` u8 [K, E, N], or
        ``None`` with ``num_steps`` when every slot is scripted.  Mirrors :meth:`rollout`; ``actions_out`` (u8 [K, E, N])
        receives the merged actions; ``masks_out`` (u8 [E, N]) the legal actions of the state behind the LAST step;
        ``reset_obs`` as for :meth:`rollout`."""
        mask, pol = self._mixed_args(scripted, policy)
        self._bind_masks(None if masks_out is None else self._check_masks(masks_out))
        E, N = self.num_envs, self.num_agents
        cur = self._other_stream()
        if actions is None:
            if mask != (1 << N) - 1:
                raise ValueError("actions may be None only when every slot is scripted")
            if num_steps is None:
                raise ValueError("num_steps is needed when actions is None")
            K, a = int(num_steps), None
        else:
            K = int(actions.shape[0])
            if num_steps is not None and int(num_steps) != K:
                raise ValueError(f"num_steps = {num_steps} but actions holds {K} steps")
            a = self._as_dev_u8(actions, (K, E, N), cur)
        o = None if order is None else self._as_dev_u8(order, (K, E, N), cur)
        if actions_out is not None:
            self._check_actions_out(actions_out, (K, E, N))
        with self._rollout_call(K, auto_reset, out, want_traj, want_obs, want_compact, reset_obs, check_pool=True, cur=cur,
                                extra=(actions_out, masks_out)) as (out, ro):
            check(self._lib.ccx_rollout_mixed(self._h, K, pol, mask, _ptr(a), _ptr(o), int(bool(auto_reset)), ro,
                                              _ptr(actions_out)))
        return out

    # ------------------------------------------------------------------ the split step / array-form strategies
    @property
    def has_array_strategies(self) -> bool:
        """The config names user strategy classes that run in array form: ``step`` goes begin -> their batched methods ->
        finish (``ccx_step_begin`` / ``ccx_step_finish``)."""
        return bool(self._array_strategies)

    def strategy_view(self):
        """:class:`strategies.StrategyView` over the handle's own state (zero-copy; valid for the life of the batch).  The
        flag arrays are the state's bytes seen as ``torch.bool``: they hold 0 / 1 only (the kernels write nothing else and
        ``set_state`` refuses other values, include/ccx.h: ccx_set_state_host)."""
        if self._view is None:
            from .strategies import StrategyView
            st = _abi.CcxState()
            check(self._lib.ccx_state_view(self._h, C.byref(st)))
            E, N = self.num_envs, self.num_agents
            en = E * N

            def dev(ptr, count, typestr, dtype, shape):
                return torch.as_tensor(_CudaArrayView(ptr, count, typestr), device=self.device).view(dtype).view(shape)

            self._view = StrategyView(
                self.config, dev(st.x, en, "<i4", torch.int32, (E, N)), dev(st.y, en, "<i4", torch.int32, (E, N)),
                dev(st.active, en, "|u1", torch.bool, (E, N)), dev(st.terminated, en, "|u1", torch.bool, (E, N)),
                dev(st.truncated, en, "|u1", torch.bool, (E, N)), dev(st.step_count, E, "<i4", torch.int32, (E,)))
        return self._view

    def step_begin(self, actions, order=None) -> None:
        """First half of ``step`` (``ccx_step_begin``, collectivecrossing.py:188-212): the step counter, the ordered moves,
        deactivation on arrival.  No flag changes and nothing is written out; :meth:`strategy_view` shows the result."""
        cur = self._other_stream()
        self._begin(actions, order, cur)
        if cur is not None:
            self._current_stream_waits(cur=cur)              # (readers of the strategy_view)

    def _begin(self, actions, order, cur) -> None:
        E, N = self.num_envs, self.num_agents
        a = self._as_dev_u8(actions, (E, N), cur)
        o = None if order is None else self._as_dev_u8(order, (E, N), cur)
        if cur is not None:
            self._order_after_current_stream(cur=cur)        # (the state: earlier readers of the strategy_view)
        check(self._lib.ccx_step_begin(self._h, a.data_ptr(), None if o is None else o.data_ptr()))

    def _user_array(self, name: str, t, dtypes, to_dtype, cur=False):
        """A caller's reward / terminated / truncated array for ``step_finish``: a device tensor [E, N] of the C type."""
        if t is None:
            return None
        E, N = self.num_envs, self.num_agents
        if not isinstance(t, torch.Tensor):
            t = torch.as_tensor(np.asarray(t))
        if t.dtype not in dtypes:
            raise TypeError(f"{name} must be one of {[str(d) for d in dtypes]}, got {t.dtype}")
        if tuple(t.shape) != (E, N):
            raise TypeError(f"{name} must have shape {(E, N)}, got {tuple(t.shape)}")
        t = t.to(self.device).contiguous()
        if t.dtype is torch.bool:
            t = t.to(to_dtype) if to_dtype is torch.int8 else t.view(torch.uint8)
        if cur is not None:
            self._order_after_current_stream(t, cur=cur)
        return t

    def step_finish(self, reward=None, terminated=None, truncated=None, want_obs: bool = True, want_compact: bool = False,
                    auto_reset: bool = False, reset_obs: str = "terminal", want_final: bool = False) -> StepResult:
        """Second half of ``step`` (``ccx_step_finish``, collectivecrossing.py:214-259) with the caller's arrays in place of
        the strategies: ``reward`` f64 [E, N], ``terminated`` bool or int8 [E, N] (-1 = no ``terminateds[id]`` entry),
        ``truncated`` bool or uint8 [E, N]; ``None`` = the handle's built-in rule.  Reward and truncation values count
        where the agent was live before the step.  ``begin`` + ``finish()`` is ``step``.  ``auto_reset`` restarts envs
        whose step raised ``__all__`` from the reset pool (``EF_RESET``), as ``rollout`` does; ``reset_obs="next"`` then
        leaves the restarted state's rows at those envs (:meth:`rollout`), and with ``want_final`` their terminal rows in
        ``StepResult.final_obs`` / ``final_compact`` (rows of other envs there are never written).

        On a batch whose config names array-form classes, an argument left ``None`` is filled by the config's own class of
        that kind (:meth:`run_array_strategies`), never by the stand-in mode the handle was built with: ``step_begin`` +
        ``step_finish()`` is ``step`` there too."""
        self._bind_masks(None)
        cur = self._other_stream()
        r = self._user_array("reward", reward, (torch.float64,), None, cur)
        t = self._user_array("terminated", terminated, (torch.bool, torch.int8), torch.int8, cur)
        u = self._user_array("truncated", truncated, (torch.bool, torch.uint8), torch.uint8, cur)
        if self._array_strategies:
            kinds = [k for k, v in (("reward", r), ("termination", t), ("truncation", u)) if v is None]
            own = self._run_array(kinds, cur)
            r, t, u = (v if v is not None else o for v, o in zip((r, t, u), own))
        res = self._finish(r, t, u, want_obs, want_compact, auto_reset, reset_obs, want_final, cur)
        if self._tracking:
            self._track(1, res)
        if cur is not None:
            self._current_stream_waits(cur=cur)
        return res

    def _finish(self, r, t, u, want_obs, want_compact, auto_reset, reset_obs: str = "terminal", want_final: bool = False,
                cur=False) -> StepResult:
        E, N = self.num_envs, self.num_agents
        want_final = bool(want_final) and reset_obs == "next"
        key = (bool(want_obs), bool(want_compact), want_final)
        cached = self._finish_cache.get(key)
        if cached is None:
            b = self._step_buffers(want_compact)
            if self._term_present is None:
                self._term_present = self._new((E, N), torch.uint8)
            so = _abi.CcxStepOut(_ptr(b.obs if want_obs else None).value, _ptr(b.reward).value, _ptr(b.agent_flags).value,
                                 _ptr(b.env_flags).value, _ptr(b.obs_compact if want_compact else None).value)
            if want_final:
                self.step_final_buffers(want_obs, want_compact)
            cached = (so, C.byref(so), StepResult(b.obs if want_obs else None, b.reward, b.agent_flags, b.env_flags,
                                                  b.obs_compact if want_compact else None, self._term_present,
                                                  final_obs=self._final_bufs[0] if want_final and want_obs else None,
                                                  final_compact=self._final_bufs[1] if want_final and want_compact else None))
            self._finish_cache[key] = cached
        res = cached[2]
        self._reset_obs(reset_obs, res.final_obs, res.final_compact, (res.obs, res.obs_compact))
        if cur is not None:                  # (buffers allocated or zeroed just now, and earlier readers of the static ones)
            self._order_after_current_stream(*_result_tensors(res), cur=cur)
        check(self._lib.ccx_step_finish(self._h, _ptr(r), _ptr(t), _ptr(u), cached[1], _ptr(self._term_present),
                                        int(bool(auto_reset))))
        return cached[2]

    def run_array_strategies(self, kinds=("reward", "termination", "truncation")):
        """The config's array-form classes on the state ``begin`` left: ``(reward, terminated, truncated)`` device tensors
        in the C types of ``ccx_step_finish``, ``None`` where the strategy is built-in (or its kind is not in ``kinds``).
        Runs on the handle's stream, inside the stream-order contract: the results come from that stream's pool and are
        recorded for torch's current stream when it is another one."""
        return self._run_array(kinds, self._other_stream())

    def _run_array(self, kinds, cur):
        from .strategies import ARRAY_METHODS, check_batch_result
        view = self.strategy_view()
        out = []
        if cur is not None:
            self._order_after_current_stream(cur=cur)
        ctx = torch.cuda.stream(self._stream) if cur is not None else contextlib.nullcontext()
        with ctx:
            for kind in ("reward", "termination", "truncation"):
                fn = self._array_strategies.get(kind) if kind in kinds else None
                out.append(None if fn is None else check_batch_result(kind, fn, getattr(fn, ARRAY_METHODS[kind])(view), view))
        if cur is not None:
            self._current_stream_waits(cur=cur)
            for t in out:
                if t is not None:
                    t.record_stream(cur)
        return out

    def _step_array(self, actions, order, want_obs, want_compact, auto_reset: bool = False, cur=False) -> StepResult:
        if cur is False:
            cur = self._other_stream()
        self._begin(actions, order, cur)
        r, t, u = self._run_array(("reward", "termination", "truncation"), cur)
        return self._finish(r, t, u, want_obs, want_compact, auto_reset, cur=cur)

    def _finish_into(self, r, t, u, out: "RolloutResult | None", s: int, auto_reset: bool, reset_obs: str = "terminal") -> None:
        fields = ("obs", "reward", "agent_flags", "env_flags", "obs_compact", "term_present")
        if out is None:
            self._reset_obs(reset_obs)
        else:       # (the side buffers of step s: the slices of the result's own)
            at = [None if v is None else v[s] for v in (out.final_obs, out.final_compact, out.obs, out.obs_compact)]
            self._reset_obs(reset_obs, at[0], at[1], (at[2], at[3]))
        ptrs = [_ptr(None if out is None or getattr(out, f) is None else getattr(out, f)[s]) for f in fields]
        so = _abi.CcxStepOut(*(p.value for p in ptrs[:5]))
        check(self._lib.ccx_step_finish(self._h, _ptr(r), _ptr(t), _ptr(u), C.byref(so), ptrs[5], int(bool(auto_reset))))

    def _rollout_array(self, K, actions, order, policy, auto_reset, out, want_traj, want_obs, want_compact, actions_out,
                       reset_obs: str = "terminal", cur=False):
        """``rollout`` / ``rollout_policy`` of a batch with array-form strategies: the split step once per tick (three
        launches plus the user's tensor code per step: launch-bound, not the fused kernel's speed).  A result allocated
        here carries ``term_present``; a caller's own ``out`` gets it only if its ``term_present`` is set; without a
        trajectory (``want_traj=False``) nothing is written out."""
        E, N = self.num_envs, self.num_agents
        own = out is None and want_traj
        if cur is False:
            cur = self._other_stream()
        with self._rollout_call(K, auto_reset, out, want_traj, want_obs, want_compact, reset_obs, check_pool=True, cur=cur,
                                extra=(actions_out,)) as (out, _):
            if own:
                out.term_present = self._new((K, E, N), torch.uint8)
                if cur is not None:
                    out.term_present.record_stream(self._stream)
            row_align = 16 if N % 2 == 0 else 8       # (odd agent counts write the rows in 8-byte units)
            if out is not None and out.obs is not None and K > 1 and (E * N * self.obs_len * 4) % row_align:
                raise ValueError(f"{E} envs x {N} agents: a step's observation rows are not a multiple of {row_align} bytes")
            for s in range(K):
                if policy is None:
                    self._begin(actions[s], None if order is None else order[s], cur)
                else:
                    a = self.policy_actions(policy, out=None if actions_out is None else actions_out[s])
                    self._begin(a, None, cur)
                r, t, u = self._run_array(("reward", "termination", "truncation"), cur)
                self._finish_into(r, t, u, out, s, auto_reset, reset_obs)
        return out

    def rows_alignment(self) -> int:
        """Smallest batch-size multiple for which one env-step's slab of observation rows ([E][N][L] floats) is a whole number
        of 128-byte lines.  A batch that is not such a multiple still gives bit-identical results, but every step's slab then
        starts somewhere else within a line: wide rows (about 40 agents and more) take a per-step layout and lose ~5 %, narrow
        ones keep the region-relative layout and lose 10-30 %."""
        row_bytes, m = self.num_agents * self.obs_len * 4, 1
        while (row_bytes * m) % 128:
            m *= 2
        return m

    def alloc_rollout(self, num_steps: int, want_obs: bool = True, want_compact: bool = False,
                      want_final: bool = False) -> RolloutResult:
        """Output tensors of a K-step rollout.  ``want_final``: also the side buffers ``final_obs`` / ``final_compact`` that
        a ``reset_obs="next"`` call fills with the terminal rows of restarted envs (zeroed here; only those rows are written)."""
        K, E, N = num_steps, self.num_envs, self.num_agents
        if want_obs and K >= 32 and E % self.rows_alignment() and not getattr(self, "_warned_alignment", False):
            import warnings
            self._warned_alignment = True
            warnings.warn(f"{E} envs x {N} agents: a step's observation rows are not a whole number of 128-byte lines; rollouts with "
                          f"rows run faster with a batch size that is a multiple of {self.rows_alignment()} (results are identical)",
                          RuntimeWarning, stacklevel=2)
        return RolloutResult(self._new((K, E, N, self.obs_len), torch.float32) if want_obs else None,
                             self._new((K, E, N), torch.float64), self._new((K, E, N), torch.uint8),
                             self._new((K, E), torch.uint8),
                             self._new((K, E, N, 4), torch.float32) if want_compact else None,
                             final_obs=self._new((K, E, N, self.obs_len), torch.float32).zero_() if want_final and want_obs else None,
                             final_compact=self._new((K, E, N, 4), torch.float32).zero_() if want_final and want_compact else None)

    def expand_observations(self, obs_compact: torch.Tensor, out: torch.Tensor | None = None) -> torch.Tensor:
        """Compact rows ``[..., N, 4]`` -> DefaultObservation rows ``[..., N, L]`` on the device
        (``ccx_expand_observations``: the gather of ``ccx_observe``, bit for bit; observations.py:43-94)."""
        c = obs_compact.to(device=self.device, dtype=torch.float32).contiguous()
        if c.shape[-2:] != (self.num_agents, 4):
            raise ValueError(f"expected [..., {self.num_agents}, 4], got {tuple(c.shape)}")
        rows = int(c.numel() // (self.num_agents * 4))
        if out is None:
            out = self._new((*c.shape[:-1], self.obs_len), torch.float32)
        self._enqueue(self._lib.ccx_expand_observations, c, rows, out)
        return out

    # ------------------------------------------------------------------ rendering
    def frame_shape(self, cell_px: int = 8) -> tuple[int, int, int]:
        """(H * cell_px, W * cell_px, 3): one rgb_array frame of :meth:`render`."""
        cp = _check_cell_px(cell_px)
        return (self.params.height * cp, self.params.width * cp, 3)

    def _frames_out(self, lead: tuple, cell_px: int, out: torch.Tensor | None) -> torch.Tensor:
        shape = (*lead, *self.frame_shape(cell_px))
        if out is None:
            return self._new(shape, torch.uint8)
        if not isinstance(out, torch.Tensor) or out.dtype is not torch.uint8:
            raise ValueError("out must be a torch.uint8 tensor")
        if out.device != self.device:
            raise ValueError(f"out must live on {self.device}, got {out.device}")
        if tuple(out.shape) != shape:
            raise ValueError(f"out must have shape {shape}, got {tuple(out.shape)}")
        if not out.is_contiguous() or out.data_ptr() % 16:
            raise ValueError("out must be contiguous and 16-byte aligned")
        return out

    def render(self, env_ids=None, cell_px: int = 8, out: torch.Tensor | None = None) -> torch.Tensor:
        """rgb_array frames of the current state (``ccx_render``): ``torch.uint8 [R, H*cell_px, W*cell_px, 3]`` on the
        device, R = E (``env_ids=None``) or ``len(env_ids)``.  The picture of the reference's rendering.py without text,
        ticks, title and legend (the frame spec is in include/ccx.h, CCX_RENDER); an id outside [0, E) gives a frame of
        the static layers only.  Only enqueues (no host synchronisation), so it captures into a graph after ``step``."""
        cp = _check_cell_px(cell_px)
        ids = None
        if env_ids is not None:
            if isinstance(env_ids, torch.Tensor):
                if env_ids.is_cuda and env_ids.device != self.device:
                    raise ValueError(f"env_ids must live on {self.device} or the host, got {env_ids.device}")
                if env_ids.dtype.is_floating_point or env_ids.dtype is torch.bool or env_ids.is_complex():
                    raise ValueError(f"env_ids must be integers, got {env_ids.dtype}")
                ids = env_ids
            else:
                arr = np.asarray(env_ids)
                if arr.size and arr.dtype.kind not in "iu":
                    raise ValueError(f"env_ids must be integers, got {arr.dtype}")
                if arr.size and (arr.min() < np.iinfo(np.int32).min or arr.max() > np.iinfo(np.int32).max):
                    raise ValueError("env_ids must fit int32")
                ids = torch.from_numpy(np.ascontiguousarray(arr, np.int32))
            if ids.dim() != 1:
                raise ValueError(f"env_ids must be 1-D, got shape {tuple(ids.shape)}")
            ids = ids.to(device=self.device, dtype=torch.int32).contiguous()
        rows = self.num_envs if ids is None else int(ids.shape[0])
        frames = self._frames_out((rows,), cp, out)
        if rows:
            self._enqueue(self._lib.ccx_render, ids, rows, cp, frames)
        return frames

    def render_compact(self, obs_compact: torch.Tensor, cell_px: int = 8, out: torch.Tensor | None = None) -> torch.Tensor:
        """Frames of compact rows ``[..., N, 4]`` (``ccx_render_compact``) -> ``[..., H*cell_px, W*cell_px, 3]`` uint8:
        a ``[K, E, N, 4]`` trajectory of ``rollout(..., want_compact=True)`` becomes K x E video frames in one launch."""
        cp = _check_cell_px(cell_px)
        if not isinstance(obs_compact, torch.Tensor):
            obs_compact = torch.from_numpy(np.ascontiguousarray(obs_compact, np.float32))
        if obs_compact.dim() < 2 or tuple(obs_compact.shape[-2:]) != (self.num_agents, 4):
            raise ValueError(f"expected [..., {self.num_agents}, 4], got {tuple(obs_compact.shape)}")
        c = obs_compact.to(device=self.device, dtype=torch.float32).contiguous()
        lead = tuple(c.shape[:-2])
        rows = int(np.prod(lead, dtype=np.int64)) if lead else 1
        frames = self._frames_out(lead, cp, out)
        if rows:
            self._enqueue(self._lib.ccx_render_compact, c, rows, cp, frames)
        return frames

    def rollout(self, actions, order=None, auto_reset: bool = False,
                out: RolloutResult | None = None, want_obs: bool = True,
                want_traj: bool = True, want_compact: bool = False,
                masks_out: torch.Tensor | None = None, reset_obs: str = "terminal") -> RolloutResult | None:
        """K fused steps (``ccx_rollout``); ``actions`` u8 [K, E, N] on the device.  ``masks_out`` (u8 [E, N]) receives the
        legal actions (:meth:`action_masks`) of the state behind the LAST step, after an auto-reset if one happened.
        ``reset_obs="next"`` (with ``auto_reset``): wherever ``env_flags`` carries ``EF_RESET``, ``obs`` / ``obs_compact``
        hold the first observation of the episode that step opened -- what a policy fed from ``out.obs`` needs -- and the
        terminal rows go to ``out.final_obs`` / ``out.final_compact`` when the result has them
        (``alloc_rollout(want_final=True)``); rewards and flags keep describing the finished step (include/ccx.h:
        CCX_RESET_OBS).  The default "terminal" writes the finished step's own rows.  A batch with array-form user
        strategies runs the split step once per tick instead (launch-bound: three launches plus the user's tensor code per
        step) into the same preallocated result, with ``term_present`` filled."""
        K = int(actions.shape[0])
        E, N = self.num_envs, self.num_agents
        cur = self._other_stream()
        a = self._as_dev_u8(actions, (K, E, N), cur)
        o = None if order is None else self._as_dev_u8(order, (K, E, N), cur)
        self._bind_masks(None if masks_out is None else self._check_masks(masks_out))
        if self._array_strategies:
            return self._rollout_array(K, a, o, None, auto_reset, out, want_traj, want_obs, want_compact, None, reset_obs, cur)
        with self._rollout_call(K, auto_reset, out, want_traj, want_obs, want_compact, reset_obs, cur=cur,
                                extra=(masks_out,)) as (out, ro):
            check(self._lib.ccx_rollout(self._h, K, _ptr(a), _ptr(o), int(bool(auto_reset)), ro))    # (no trajectory: NULL)
            self._rollouts_with_obs += int(out is not None and out.obs is not None and K >= 64)
        return out

    def rollout_greedy(self, num_steps: int, auto_reset: bool = False, out: RolloutResult | None = None,
                       want_obs: bool = True, actions_out: torch.Tensor | None = None,
                       want_actions: bool = True, policy: str = "greedy", masks_out: torch.Tensor | None = None,
                       reset_obs: str = "terminal"):
        """K fused steps driven by an on-device scripted policy ("greedy" or "waiting",
        ``ccx_rollout_policy``); returns ``(RolloutResult, actions u8 [K, E, N])``.  ``masks_out`` and ``reset_obs`` as for
        :meth:`rollout`."""
        K, E, N = int(num_steps), self.num_envs, self.num_agents
        self._bind_masks(None if masks_out is None else self._check_masks(masks_out))
        if actions_out is None and want_actions:
            actions_out = self._new((K, E, N), torch.uint8)
        cur = self._other_stream()
        if self._array_strategies:
            return self._rollout_array(K, None, None, policy, auto_reset, out, True, want_obs, False, actions_out,
                                       reset_obs, cur), actions_out
        with self._rollout_call(K, auto_reset, out, True, want_obs, False, reset_obs, cur=cur,
                                extra=(actions_out, masks_out)) as (out, ro):
            check(self._lib.ccx_rollout_policy(self._h, K, _abi.POLICIES[policy], int(bool(auto_reset)), ro, _ptr(actions_out)))
            self._rollouts_with_obs += int(out.obs is not None and K >= 64)
        return out, actions_out

    def rollout_policy(self, num_steps: int, policy: str, auto_reset: bool = False, **kw):
        """``ccx_rollout_policy`` under its general name: "greedy", "waiting" or "random" (uniform actions drawn
        on the device, seeded by :meth:`set_rng_seed`)."""
        return self.rollout_greedy(num_steps, auto_reset=auto_reset, policy=policy, **kw)

    def set_rng_seed(self, seed: int) -> None:
        """Seed of the on-device action RNG (``CCX_POLICY_RANDOM``)."""
        check(self._lib.ccx_set_rng_seed(self._h, int(seed) & (2**64 - 1)))

    def set_policy_epsilon(self, epsilon: float) -> None:
        """``randomness_factor`` of the on-device greedy / waiting policies (``ccx_set_policy_epsilon``): with
        probability epsilon an agent takes one of its valid actions uniformly (the reference's
        ``create_greedy_policy(epsilon=0.1)``), drawn from the counter-based RNG seeded by :meth:`set_rng_seed`
        -- not numpy's stream; the host classes in ``baseline_policies`` keep that one.  0 = deterministic."""
        check(self._lib.ccx_set_policy_epsilon(self._h, float(epsilon)))

    def set_policy_stream(self, kind: str = "mt19937", seeds=42) -> None:
        """Where the policies' exploration draws come from (``ccx_set_policy_stream``): ``"counter"`` (default) or
        ``"mt19937"`` -- every env owns numpy's ``RandomState(seeds[e])`` (one int: the same seed for every env, like one
        ``create_greedy_policy()`` object per env, seed 42) and the device walks it exactly as the reference's
        ``get_action`` calls do, so epsilon episodes of the reference replay action for action.  Policy rollouts then
        run policy and step as separate launches (a validation mode, not the fast path)."""
        kinds = {"counter": 0, "mt19937": 1}
        if kind not in kinds:
            raise ValueError(f"unknown epsilon stream {kind!r}; one of {sorted(kinds)}")
        if np.ndim(seeds) == 0:
            check(self._lib.ccx_set_policy_stream(self._h, kinds[kind], None, int(seeds) & 0xFFFFFFFF))
            return
        arr = np.ascontiguousarray(np.asarray(seeds, np.uint32).reshape(self.num_envs))
        check(self._lib.ccx_set_policy_stream(self._h, kinds[kind], arr.ctypes.data, 0))

    def policy_stream_state(self) -> np.ndarray:
        """u32 [E, 625]: every env's MT19937 generator (key[624], pos) as ``RandomState.get_state()`` has it."""
        out = np.empty((self.num_envs, 625), np.uint32)
        check(self._lib.ccx_get_policy_stream(self._h, None, out.ctypes.data))
        return out

    # ------------------------------------------------------------------ counters / timing / shape
    def zero_counters(self) -> None:
        self._enqueue(self._lib.ccx_zero_counters)           # (readers of counters_tensor)

    def counters(self) -> dict[str, int]:
        c = _abi.CcxCounters()
        check(self._lib.ccx_read_counters(self._h, C.byref(c)))
        return c.as_dict()

    def counters_tensor(self) -> torch.Tensor:
        """Zero-copy int64 view of the 6 device counters (for the RCCL all-reduce)."""
        p = C.c_void_p()
        check(self._lib.ccx_counters_device_ptr(self._h, C.byref(p)))
        return _device_view_i64(p.value, len(_abi.COUNTER_FIELDS), self.device)

    def set_check_inputs(self, enabled: bool = True) -> None:
        """Opt-in validation of action / move-order tensors on the device (``ccx_set_check_inputs``): what
        the reference's ``_check_action_and_agent_validity`` raises on (collectivecrossing.py:685-711).
        Violations surface as :class:`CcxInputError` (a ``ValueError``) from the next ``synchronize()``,
        ``counters()`` or ``check_inputs()``.  Also enabled by ``CCX_CHECK_INPUTS=1``."""
        check(self._lib.ccx_set_check_inputs(self._h, int(bool(enabled))))

    def check_inputs(self) -> None:
        """Synchronise and raise ``CcxInputError`` if a checked launch saw invalid actions / orders."""
        check(self._lib.ccx_check_inputs(self._h))

    def set_tunable(self, name: str, value: int) -> None:
        """Performance experiment knobs (``ccx_set_tunable``); results never depend on them."""
        check(self._lib.ccx_set_tunable(self._h, name.encode(), int(value)))

    def set_step_pace_start(self, ns_per_env_step: float) -> None:
        """Start value of the adaptive pace controller (``ccx_set_step_pace_start``), 0 = library default."""
        check(self._lib.ccx_set_step_pace_start(self._h, float(ns_per_env_step)))

    # -- where the pace controller starts.  By default the library MEASURES it in-process (ccx_set_pace_calibration: a
    # ~2.5 ms write probe of the caller's own trajectory buffer at the first long rollout).  A pace memory across processes
    # is opt-in: only when CCX_PACE_CACHE names a file does a handle start from the pace an earlier handle of the same
    # shape settled at, and only then is the file updated on close() (never from a multi-rank job: N ranks would
    # read-modify-write one file).  Nothing is ever read from or written to $HOME implicitly.  Never affects results.
    PACE_START_SOURCES = {0: "unpaced", 1: "assumed", 2: "caller", 3: "calibration", 4: "fixed"}

    @staticmethod
    def _pace_cache_path() -> Path | None:
        p = os.environ.get("CCX_PACE_CACHE")
        try:
            world = int(os.environ.get("WORLD_SIZE", "1") or "1")
        except ValueError:                     # (an empty or non-numeric value must not break handle construction: ADVICE r3)
            world = 1
        if not p or world > 1:
            return None
        return Path(p)

    def _pace_key(self) -> str:
        s = self.launch_shape()
        c = self.config
        props = torch.cuda.get_device_properties(self.device)
        name = str(getattr(props, "gcnArchName", "") or props.name).split(":")[0]    # "gfx950" (the marketing name varies)
        return (f"{name}|grid{c.width}x{c.height}|E{self.num_envs}|N{self.num_agents}|lanes{s['lanes_per_wave']}"
                f"|tpb{s['waves_per_block']}|w{s['writers_per_tile']}")

    def _apply_pace_memory(self) -> None:
        """(Re)applied whenever the launch shape changes: the key names the shape."""
        self._pace_from_cache = False
        path = self._pace_cache_path()
        if path is None:
            return
        try:
            ns = float(json.loads(path.read_text())[self._pace_key()]["pace_ns"])
        except Exception:
            return
        if ns > 0:
            self.set_step_pace_start(ns * 1.01)      # start a notch on the safe side of the remembered pace
            self._pace_from_cache = True

    def _remember_pace(self) -> None:
        path = self._pace_cache_path()
        if path is None or self._rollouts_with_obs < 40:
            return
        ns = self.step_pace_ns()
        if not ns > 0:
            return
        try:
            data = json.loads(path.read_text())
        except Exception:
            data = {}
        data[self._pace_key()] = {"pace_ns": round(ns, 2), "launches": self._rollouts_with_obs}
        path.parent.mkdir(parents=True, exist_ok=True)
        tmp = path.with_suffix(f".tmp{os.getpid()}")
        tmp.write_text(json.dumps(data, indent=1, sort_keys=True))
        tmp.replace(path)

    def pace_start(self) -> dict:
        """Where the adaptive pace controller started (``ccx_get_pace_start``): ``ns`` per env-step, ``source`` in
        {"unpaced", "assumed", "caller", "calibration", "fixed", "user_cache"} ("user_cache" = a caller's value that came
        from the CCX_PACE_CACHE file), ``probe_GBs`` = the write rate the calibration probe measured (0 = it has not run)."""
        ns, src, gbs = C.c_float(), C.c_int32(), C.c_float()
        check(self._lib.ccx_get_pace_start(self._h, C.byref(ns), C.byref(src), C.byref(gbs)))
        source = self.PACE_START_SOURCES.get(int(src.value), str(src.value))
        if source == "caller" and getattr(self, "_pace_from_cache", False):
            source = "user_cache"
        return {"ns": float(ns.value), "source": source, "probe_GBs": float(gbs.value)}

    def set_pace_calibration(self, enabled: bool = True) -> None:
        """In-process start-up calibration of the pace controller (``ccx_set_pace_calibration``; default on)."""
        check(self._lib.ccx_set_pace_calibration(self._h, int(bool(enabled))))

    def set_timing(self, enabled: bool = True) -> None:
        """Record HIP events around every launch so that ``last_launch_ms`` works (off by default)."""
        check(self._lib.ccx_set_timing(self._h, int(bool(enabled))))

    def last_launch_ms(self) -> float:
        ms = C.c_float()
        check(self._lib.ccx_last_launch_ms(self._h, C.byref(ms)))
        return float(ms.value)

    def set_launch_shape(self, lanes_per_wave: int = 0, waves_per_block: int = 0) -> None:
        check(self._lib.ccx_set_launch_shape(self._h, lanes_per_wave, waves_per_block))
        self._shape_changed()

    def set_writers(self, writers_per_tile: int = 0) -> None:
        check(self._lib.ccx_set_writers(self._h, writers_per_tile))
        self._shape_changed()

    def _shape_changed(self) -> None:
        """A remembered start value belongs to ONE launch shape: drop it, look the new shape up."""
        if getattr(self, "_pace_from_cache", False):
            self.set_step_pace_start(0.0)
        self._apply_pace_memory()

    def set_store_throttle(self, max_stores_in_flight: int = 0) -> None:
        check(self._lib.ccx_set_store_throttle(self._h, max_stores_in_flight))

    def set_step_pace(self, ns_per_env_step: int = 0) -> None:
        """0 = adaptive (default), -1 = off, > 0 = fixed nanoseconds per env-step (``ccx_set_step_pace``)."""
        check(self._lib.ccx_set_step_pace(self._h, int(ns_per_env_step)))

    def step_pace_ns(self) -> float:
        ns = C.c_float()
        check(self._lib.ccx_get_step_pace(self._h, C.byref(ns)))
        return float(ns.value)

    def pace_state(self) -> dict[str, float]:
        """The pace controller's state (``ccx_get_pace_state``): next pace / floor in ns, launches since the
        last collapse, whether rollouts of this shape are paced at all."""
        v = (C.c_float * 6)()
        check(self._lib.ccx_get_pace_state(self._h, v))
        return dict(zip(("next_pace_ns", "floor_ns", "calm_launches", "paced", "cliff_ns", "cliff_confirmations"),
                        (float(x) for x in v)))

    def launch_shape(self) -> dict[str, int]:
        v = [C.c_int32() for _ in range(4)]
        check(self._lib.ccx_get_launch_shape(self._h, *[C.byref(x) for x in v]))
        w = [C.c_int32() for _ in range(2)]
        check(self._lib.ccx_get_writer_shape(self._h, *[C.byref(x) for x in w]))
        r = [C.c_int32() for _ in range(2)]
        check(self._lib.ccx_get_residency(self._h, *[C.byref(x) for x in r]))
        return dict(zip(("lanes_per_wave", "waves_per_block", "group_lanes", "num_blocks",
                         "writers_per_tile", "store_throttle", "resident_blocks"),
                        (int(x.value) for x in v + w + r[:1])))

    def set_reward_table(self, boarding, exiting) -> None:
        """Per-(agent type, cell) rewards, f64 ``[height + 1, width + 1]`` each (``ccx_set_reward_table``): what a
        position-only user ``RewardFunction`` (rewards.py:16-38) is lowered to.  ``None, None`` restores the built-in reward."""
        if boarding is None and exiting is None:
            check(self._lib.ccx_set_reward_table(self._h, None, None))
        else:
            shape = (self.config.height + 1, self.config.width + 1)
            b, e = (np.ascontiguousarray(t, np.float64) for t in (boarding, exiting))
            if b.shape != shape or e.shape != shape:
                raise ValueError(f"reward tables must be {shape} (rows y, columns x), got {b.shape} / {e.shape}")
            check(self._lib.ccx_set_reward_table(self._h, b.ctypes.data, e.ctypes.data))
        self._shape_changed()

    def set_terminated_table(self, boarding, exiting) -> None:
        """Per-(agent type, cell) ``terminateds[id]`` values, u8 ``[height + 1, width + 1]`` each (``ccx_set_terminated_table``)."""
        if boarding is None and exiting is None:
            check(self._lib.ccx_set_terminated_table(self._h, None, None))
            return
        shape = (self.config.height + 1, self.config.width + 1)
        b, e = (np.ascontiguousarray(np.asarray(t) != 0, np.uint8) for t in (boarding, exiting))
        if b.shape != shape or e.shape != shape:
            raise ValueError(f"terminated tables must be {shape} (rows y, columns x), got {b.shape} / {e.shape}")
        check(self._lib.ccx_set_terminated_table(self._h, b.ctypes.data, e.ctypes.data))

    def step_shape(self) -> dict[str, int]:
        """Launch shape of the short-launch kernel (``ccx_get_step_shape``): ``ok`` = 1 when ``step`` / rollouts of at most
        16 steps without a move order run the short-launch kernel (csrc/ccx_step.hip: a sim wave + ``row_waves`` row waves per tile)."""
        v = [C.c_int32() for _ in range(5)]
        check(self._lib.ccx_get_step_shape(self._h, *[C.byref(x) for x in v]))
        return dict(zip(("ok", "lanes_per_wave", "row_waves", "num_blocks", "lds_bytes"), (int(x.value) for x in v)))

    def use_stream(self, stream: "torch.cuda.Stream | None" = None) -> None:
        """Launch on ``stream`` (default: torch's current stream of the device) from now on."""
        self._stream = stream if stream is not None else torch.cuda.current_stream(self.device)
        self._stream_raw = self._stream.cuda_stream
        check(self._lib.ccx_set_stream(self._h, C.c_void_p(self._stream_raw)))

    def synchronize(self) -> None:
        check(self._lib.ccx_synchronize(self._h))


class _CudaArrayView:
    """Minimal ``__cuda_array_interface__`` carrier so torch can wrap library-owned memory."""

    def __init__(self, ptr: int, n: int, typestr: str = "<i8"):
        self.__cuda_array_interface__ = {"shape": (n,), "typestr": typestr, "data": (ptr, False),
                                         "version": 3, "strides": None}


def _device_view_i64(ptr: int, n: int, device: torch.device) -> torch.Tensor:
    return torch.as_tensor(_CudaArrayView(ptr, n), device=device)
