"""The learner's half of the loop on the device: advantages (CCX_GAE), masked sampling (CCX_SAMPLE), stored actions under
new logits (CCX_EVALUATE), the PPO loss (CCX_PPO_LOSS), the two-layer policy head with its backward pass (CCX_MLP) and the
optimiser step (CCX_ADAM) of ``include/ccx.h``.

:class:`LearnerOps` carries the methods and is mixed into :class:`~collectivecrossing_amd.batched.BatchedCollectiveCrossing`;
the result dataclasses, :class:`MlpHead`, :class:`DeviceAdam` and the three ``torch.autograd.Function`` classes live here with it.  What a tensor
argument must be is stated once, in :func:`_require`: a pure function of the tensor and the device, so it runs without a
batch.  What stands around a loss over the rows that count -- :meth:`LearnerOps.ppo_loss`, ``QLearning.td_loss``,
``CategoricalQ.loss`` -- is stated once too: :func:`_loss_over_rows` and the helpers in front of it."""

from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from typing import ClassVar

import numpy as np
import torch

from ._abi import ADAM_MAX_TENSORS, CcxAdamTensor
from ._lib import check


@dataclass
class GaeResult:
    """Advantages and value targets of a trajectory (:meth:`BatchedCollectiveCrossing.compute_gae`, include/ccx.h CCX_GAE).
    Every element is written: +0.0 / 0 where the agent had no step (``valid`` = 0)."""

    advantages: torch.Tensor  # f32 [K, E, N]
    returns: torch.Tensor     # f32 [K, E, N]: advantages + values, the critic's regression target
    valid: torch.Tensor | None  # u8 [K, E, N]: 1 where the agent was live in the step (a loss averages over these)


@dataclass
class SampleResult:
    """Actions sampled from a policy's logits (:meth:`BatchedCollectiveCrossing.sample_actions`, include/ccx.h CCX_SAMPLE).
    Every element is written: 255 / +0.0 / +0.0 for agents that are terminated or truncated."""

    actions: torch.Tensor         # u8 [E, N]: what step / rollout consume
    logp: torch.Tensor | None     # f32 [E, N]: log pi(action | state) under the masked distribution
    entropy: torch.Tensor | None  # f32 [E, N]: entropy of the masked distribution


@dataclass
class EvalResult:
    """Stored actions evaluated under new logits (:meth:`BatchedCollectiveCrossing.evaluate_actions`, include/ccx.h
    CCX_EVALUATE).  Every element is written: +0.0 / +0.0 for rows whose stored action is 255."""

    logp: torch.Tensor            # f32 [...]: log pi_new(stored action | state) under the masked distribution; -inf: not a legal action
    entropy: torch.Tensor | None  # f32 [...]: entropy of the masked distribution


@dataclass
class PpoLossResult:
    """The PPO loss over the rows that count (:meth:`BatchedCollectiveCrossing.ppo_loss`, include/ccx.h CCX_PPO_LOSS).
    ``stats`` = {loss, policy, value, entropy, approx_kl, clip_frac, count, 0}; the named accessors are 0-dim views of it.
    ``workspace`` / ``grad_logits`` / ``grad_values`` are the static buffers of :meth:`alloc_ppo_loss` (else ``None``)."""

    loss: torch.Tensor                        # f32 0-dim: stats[0]; carries the autograd graph when an input required grad
    stats: torch.Tensor                       # f32 [8]
    workspace: torch.Tensor | None = None     # u8 [ccx_ppo_workspace_bytes(rows)]
    grad_logits: torch.Tensor | None = None   # f32 [..., 5]
    grad_values: torch.Tensor | None = None   # f32 [...]
    _frame: ClassVar = ("ccx_ppo_workspace_bytes", "alloc_ppo_loss", "logits or values require")    # (_loss_over_rows)

    policy = property(lambda self: self.stats[1])
    value = property(lambda self: self.stats[2])
    entropy = property(lambda self: self.stats[3])
    approx_kl = property(lambda self: self.stats[4])
    clip_frac = property(lambda self: self.stats[5])
    count = property(lambda self: self.stats[6])


@dataclass
class MlpGradResult:
    """The parameter gradients of an :class:`MlpHead` (:meth:`BatchedCollectiveCrossing.mlp_backward`, include/ccx.h
    CCX_MLP, backward): every element of every tensor is written, and every bit follows the written rule.  ``grad_a`` is the
    gradient at the pre-activations (``None`` unless asked for); ``workspace`` is the static buffer of
    :meth:`alloc_mlp_backward` (else ``None``)."""

    w1t: torch.Tensor                         # f32 [L, H]
    b1: torch.Tensor                          # f32 [H]
    w2: torch.Tensor                          # f32 [O, H]
    b2: torch.Tensor                          # f32 [O]
    grad_a: torch.Tensor | None = None        # f32 [..., H]
    workspace: torch.Tensor | None = None     # u8 [ccx_mlp_backward_workspace_bytes(rows, L, H, O)]


def _require_aligned(name: str, t: torch.Tensor | None, align: int) -> None:
    if t is not None and t.data_ptr() % align:
        raise ValueError(f"{name} must be {align}-byte aligned (a view at an odd offset of its storage is not)")


def _require(name, t, dtype, shape, device, *, optional=False, align=0, hint="", verb="be") -> None:
    """THE contract of a tensor argument: ``t`` is a contiguous ``torch.Tensor`` of ``dtype`` and ``shape`` on ``device``
    whose ``data_ptr`` is a multiple of ``align`` (0: any), else ``ValueError``.  ``shape`` is a tuple, ``(..., n)`` for any
    leading shape in front of ``n``, or ``None`` for any shape; ``optional`` admits ``None``.  ``hint`` is appended to the
    message, ``verb`` is its "must be" / "must stay"."""
    if t is None and optional:
        return
    ok = isinstance(t, torch.Tensor) and t.dtype is dtype and t.device == device and t.is_contiguous()
    of_shape = ""
    if shape is not None:
        shape = tuple(shape)
        if shape[:1] == (Ellipsis,):
            tail = shape[1:]
            ok = ok and t.dim() >= len(tail) and tuple(t.shape[t.dim() - len(tail):]) == tail
            of_shape = f" of shape [..., {', '.join(map(str, tail))}]"
        else:
            ok = ok and tuple(t.shape) == shape
            of_shape = f" of shape {shape}"
    if not ok:
        raise ValueError(f"{name} must {verb} a contiguous {dtype} tensor{of_shape} on {device}{hint}")
    if align:
        _require_aligned(name, t, align)


def _require_all(device, *rows) -> None:
    """:func:`_require` over ``(name, t, dtype, shape[, keywords])`` rows in order; the alignments are looked at after every
    row has passed the rest."""
    for name, t, dtype, shape, *kw in rows:
        _require(name, t, dtype, shape, device, **{**(kw[0] if kw else {}), "align": 0})
    for name, t, _dtype, _shape, *kw in rows:
        if kw and kw[0].get("align"):
            _require_aligned(name, t, kw[0]["align"])


def _require_out(out, cls, alloc: str) -> None:
    """``out`` is ``None`` or a ``cls`` (what the method ``alloc`` returns)."""
    if out is not None and not isinstance(out, cls):
        raise ValueError(f"out must be {'an' if cls.__name__[0] in 'AEIOU' else 'a'} {cls.__name__} ({alloc})")


def _check_grad_loss(grad_loss, device) -> None:
    """``grad_loss`` of a ``*_loss_backward``: ``None`` or one f32 element in either of two shapes.  (Not :func:`_require`: it
    names no shape.)"""
    if grad_loss is not None and (not isinstance(grad_loss, torch.Tensor) or grad_loss.dtype is not torch.float32
                                  or grad_loss.device != device or grad_loss.numel() < 1 or grad_loss.dim() > 1
                                  or not grad_loss.is_contiguous()):
        raise ValueError(f"grad_loss must be a torch.float32 tensor with one element (0-dim or [1]) on {device}")


def _new_stats(device) -> torch.Tensor:
    """The f32 [8] ``stats`` of a loss over the rows that count."""
    return torch.zeros((8,), dtype=torch.float32, device=device)


def _loss_workspace(batch, cls, workspace, rows: int) -> torch.Tensor:
    """The workspace of the forward whose result class is ``cls`` (``cls._frame``: the library's function for its size, the
    ``alloc_*`` that makes one, the differentiable inputs in words): the caller's, checked, or one from torch's allocator."""
    return batch._workspace_arg(int(getattr(batch._lib, cls._frame[0])(int(rows))), workspace, cls._frame[1])


def _alloc_loss(batch, cls, shape):
    """What every ``alloc_*`` of a loss starts from: ``(shape as a tuple, stats, workspace)``."""
    shape = tuple(int(x) for x in shape)
    return shape, _new_stats(batch.device), _loss_workspace(batch, cls, None, int(np.prod(shape)) if shape else 1)


def _loss_over_rows(batch, cls, owner, fn, forward, diff, rest, rows: int, extras, out):
    """The frame of a loss over the rows that count behind its input checks; returns the ``cls``.  ``diff``: the inputs a
    gradient may reach (the first one tells whether there are rows); ``rest``: every other argument, in the order in which
    ``forward`` and ``fn.forward`` take them behind ``diff``.  ``extras``: the per-row outputs behind ``stats`` in the order
    of ``cls``'s fields, as ``(field, shape, wanted, keywords of _require)``.  ``forward(*diff, *rest, workspace, stats,
    *extras)`` enqueues the library's forward; ``fn`` is the loss's ``autograd.Function``, applied to ``(owner, *diff, *rest,
    *extras)``.  With a gradient to carry, ``out=`` is refused and the workspace comes from torch's allocator inside ``fn``;
    otherwise ``out`` is validated or allocated.  Zero rows give zero stats without calling the library, still connected to
    ``diff``."""
    dev, f = batch.device, torch.float32
    if torch.is_grad_enabled() and any([t.requires_grad for t in diff]):
        if out is not None:
            raise ValueError(f"out= cannot be used when {cls._frame[2]} a gradient (the autograd path allocates its outputs)")
        if rows == 0:
            zero = diff[0].sum()
            for t in diff[1:]:
                zero = zero + t.sum()
            stats = torch.cat([zero.reshape(1) * 0.0, torch.zeros(7, device=dev)])
            made = [diff[0].new_zeros(shape) if want else None for _, shape, want, _ in extras]
        else:
            made = [batch._new(shape, f) if want else None for _, shape, want, _ in extras]
            stats = fn.apply(owner, *diff, *rest, *made)
        return cls(stats[0], stats.detach(), *made)
    _require_out(out, cls, cls._frame[1])
    if out is None:
        stats = _new_stats(dev)
        out = cls(stats[0], stats, *[batch._new(shape, f) if want else None for _, shape, want, _ in extras])
        workspace = None
    else:
        _require("out.stats", out.stats, f, (8,), dev)
        _require_all(dev, *[(f"out.{name}", getattr(out, name), f, shape, kw) for name, shape, _, kw in extras])
        workspace = out.workspace
    if rows == 0:
        out.stats.zero_()
        return out
    forward(*[t.detach() for t in diff], *rest, _loss_workspace(batch, cls, workspace, rows), out.stats,
            *[getattr(out, name) for name, *_ in extras])
    return out


_OPT = {"optional": True}
_Tensor = torch.Tensor                                               # (a global: _enqueue looks at every argument)


class LearnerOps:
    """The learner-side methods of a batch.  The host class provides ``_lib`` (the loaded library), ``_h`` (the handle),
    ``device``, ``num_envs``, ``num_agents``, ``obs_len``, ``_new(shape, dtype)`` (an uninitialised device tensor),
    ``_order_after_current_stream(*tensors)`` (the handle's stream waits for torch's current one), and ``_stream`` /
    ``_stream_raw`` (the handle's stream as torch's object and as the raw pointer).  Every enqueueing library call here goes
    through :meth:`_enqueue`, which orders what it passes.

    **Stream order** (the contract of every method here, of :class:`BatchedCollectiveCrossing`,
    :class:`MlpHead` and :class:`DeviceAdam` that enqueues device work).  The launches go to the handle's stream: the one
    current at construction, or ``use_stream``'s.  The caller's tensors live on torch's CURRENT stream.  (a) Everything
    enqueued on the current stream before the call -- the producers of the inputs, and earlier readers or writers of the
    outputs -- happens before the method's launches.  (b) The launches happen before anything enqueued on the current
    stream after the method returns.  (c) When the two streams differ, every tensor handed in or out is recorded
    (``record_stream``) for the handle's stream.  When the current stream IS the handle's stream none of this costs a wait
    or an event, and nothing enters a captured graph.  Methods that synchronise with the host are outside the contract."""

    def _other_stream(self):
        """torch's current stream of the device when it is NOT the handle's stream, else ``None``: one read of the raw
        stream (an int; ~0.2 us), so the same-stream path makes no other call into torch.  A method reads it once and
        hands it to both helpers as ``cur=``."""
        if torch._C._cuda_getCurrentRawStream(self.device.index) == self._stream_raw:
            return None
        return torch.cuda.current_stream(self.device)

    def _enqueue(self, fn, *args, also=()) -> None:
        """THE way a library call keeps the stream-order contract: ``check(fn(self._h, *args))`` between the entry
        (:meth:`_order_after_current_stream`) and the exit (:meth:`_current_stream_waits`), with every tensor among ``args``
        ordered at the entry and handed to ``fn`` as its ``data_ptr()``.  What is passed is what is ordered; ``None``,
        numbers and ctypes tables pass through as they are.  ``also``: tensors the launch touches whose pointers travel
        inside a by-value table (the rows of a ``CcxAdamTensor`` or ``CcxSlotGroup`` array).  With the handle's stream
        current there is nothing to order and neither helper is entered: the call costs the one raw read of
        :meth:`_other_stream` and the ``data_ptr()`` calls (profiles/enqueue_host_time.txt).

        Deliberately NOT through here: the stepping calls whose pointers sit in a cached ``CcxStepOut`` /
        ``CcxRolloutOut`` (``step`` is the per-step path) use the two helpers directly; the scalar setters
        (``DeviceAdam.lr``, ``QLearning.epsilon``) make no library call; host-synchronous, query and setting calls are
        outside the contract."""
        cur = self._other_stream()
        if cur is not None:
            self._order_after_current_stream(*[a for a in args if isinstance(a, _Tensor)], *also, cur=cur)
        check(fn(self._h, *[a.data_ptr() if isinstance(a, _Tensor) else a for a in args]))
        if cur is not None:
            self._current_stream_waits(cur=cur)

    # ------------------------------------------------------------------ advantages
    def alloc_gae(self, num_steps: int, want_valid: bool = True) -> GaeResult:
        """Output tensors of :meth:`compute_gae` for a K-step trajectory (static buffers for a captured graph)."""
        shape = (int(num_steps), self.num_envs, self.num_agents)
        return GaeResult(self._new(shape, torch.float32), self._new(shape, torch.float32),
                         self._new(shape, torch.uint8) if want_valid else None)

    def compute_gae(self, traj, values: torch.Tensor, last_values: torch.Tensor, final_values: torch.Tensor | None = None,
                    gamma: float = 0.99, lam: float = 0.95, out: GaeResult | None = None) -> GaeResult:
        """Generalised advantage estimates and value targets on the device (``ccx_gae``, include/ccx.h CCX_GAE): one
        kernel on the handle's stream, bit-defined (f32, one rounding per operation, the steps walked backwards).

        ``traj`` is a :class:`RolloutResult` or a ``(reward f64 [K, E, N], agent_flags u8 [K, E, N], env_flags u8 [K, E])``
        tuple; ``values`` f32 [K, E, N] holds the critic's value of the observation each step ACTED ON, ``last_values`` f32
        [E, N] that of the state behind the last step, ``final_values`` f32 [K, E, N] (optional) that of the observation a
        step ENDED ON -- read only where an episode is cut without termination (truncation, ``EF_RESET``); evaluate the
        critic on ``final_obs`` there (``reset_obs="next"``).  Without it a cut bootstraps from 0.  Termination never
        bootstraps.  ``out`` reuses a :class:`GaeResult` (``out.valid`` may be ``None``).  All tensors: contiguous, on the
        batch's device; anything else raises ``ValueError`` before the library is called.
        Only enqueues (no host synchronisation); stream order: :class:`LearnerOps`."""
        from .batched import RolloutResult                           # (batched imports this module)
        if isinstance(traj, RolloutResult):
            reward, agent_flags, env_flags = traj.reward, traj.agent_flags, traj.env_flags
        else:
            try:
                reward, agent_flags, env_flags = traj
            except (TypeError, ValueError):
                raise ValueError("traj must be a RolloutResult or a (reward, agent_flags, env_flags) tuple") from None
        E, N = self.num_envs, self.num_agents
        K = int(reward.shape[0]) if isinstance(reward, torch.Tensor) and reward.dim() == 3 else 0
        if K < 1:
            raise ValueError(f"reward must be a torch.float64 tensor [K, {E}, {N}] with K >= 1")
        gamma, lam = float(gamma), float(lam)
        for name, x in (("gamma", gamma), ("lam", lam)):
            if not 0.0 <= x <= 1.0:                                  # (false for NaN)
                raise ValueError(f"{name} must be in [0, 1], got {x!r}")
        _require_out(out, GaeResult, "alloc_gae")
        if out is None:
            out = self.alloc_gae(K)
        KEN = (K, E, N)
        _require_all(self.device,
                     ("reward", reward, torch.float64, KEN), ("agent_flags", agent_flags, torch.uint8, KEN),
                     ("env_flags", env_flags, torch.uint8, (K, E)), ("values", values, torch.float32, KEN),
                     ("last_values", last_values, torch.float32, (E, N)),
                     ("final_values", final_values, torch.float32, KEN, _OPT),
                     ("out.advantages", out.advantages, torch.float32, KEN),
                     ("out.returns", out.returns, torch.float32, KEN), ("out.valid", out.valid, torch.uint8, KEN, _OPT))
        self._enqueue(self._lib.ccx_gae, K, reward, agent_flags, env_flags, values, last_values, final_values, gamma, lam,
                      out.advantages, out.returns, out.valid)
        return out

    # ------------------------------------------------------------------ sampling from a learned policy
    def alloc_sample(self, want_logp: bool = True, want_entropy: bool = False) -> SampleResult:
        """Output tensors of :meth:`sample_actions` (static buffers for a captured graph)."""
        shape = (self.num_envs, self.num_agents)
        return SampleResult(self._new(shape, torch.uint8), self._new(shape, torch.float32) if want_logp else None,
                            self._new(shape, torch.float32) if want_entropy else None)

    def sample_actions(self, logits: torch.Tensor, masks: torch.Tensor | None = None, deterministic: bool = False,
                       want_logp: bool = True, want_entropy: bool = False, out: SampleResult | None = None) -> SampleResult:
        """Masked categorical actions from a network's logits on the device (``ccx_sample_actions``, include/ccx.h
        CCX_SAMPLE): one kernel on the handle's stream, bit-defined, drawn with the library's counter-based key (global env,
        episode, step of the episode, agent slot; :meth:`set_rng_seed`) -- the same actions for any split into calls, any
        world size, eager or captured.

        ``logits`` f32 [E, N, 5] (index = action id); ``masks`` u8 [E, N] (``action_masks`` / ``masks_out``; ``None`` =
        everything legal); ``deterministic`` takes the masked argmax (lowest index on ties) and draws nothing.  ``logp`` is
        ``log pi(action)`` under the masked distribution, ``entropy`` that distribution's entropy.  Agents that are
        terminated or truncated get action 255, ``logp`` = ``entropy`` = 0.  ``out`` reuses a :class:`SampleResult` (its
        ``logp`` / ``entropy`` may be ``None``; ``want_*`` is then ignored): ``out.actions`` may be a ``[E, N]`` view of the
        ``[1, E, N]`` tensor :meth:`rollout` reads.  All tensors: contiguous, on the batch's device; anything else raises
        ``ValueError`` before the library is called.  Not here: bf16 / f16 logits (cast first), a temperature (scale the
        logits first).
        Only enqueues (no host synchronisation); stream order: :class:`LearnerOps`."""
        E, N = self.num_envs, self.num_agents
        _require_out(out, SampleResult, "alloc_sample")
        if out is None:
            out = self.alloc_sample(want_logp, want_entropy)
        _require_all(self.device,
                     ("logits", logits, torch.float32, (E, N, 5), {"align": 16}), ("masks", masks, torch.uint8, (E, N), _OPT),
                     ("out.actions", out.actions, torch.uint8, (E, N)), ("out.logp", out.logp, torch.float32, (E, N), _OPT),
                     ("out.entropy", out.entropy, torch.float32, (E, N), _OPT))
        self._enqueue(self._lib.ccx_sample_actions, logits, masks, int(bool(deterministic)), out.actions, out.logp, out.entropy)
        return out

    # ------------------------------------------------------------------ the policy head: observation rows to logits
    def mlp_head(self, H: int, O: int = 5, activation: str = "tanh", L: int | None = None, backward: str = "torch") -> "MlpHead":
        """A two-layer perceptron ``Linear(L, H) -> tanh | relu -> Linear(H, O)`` whose forward is ONE kernel with bit-defined
        outputs (:class:`MlpHead`, include/ccx.h CCX_MLP).  ``L`` defaults to ``obs_len``; ``H`` is a multiple of 16 in
        16..256, ``O`` in 1..8.  ``O = 5`` is an actor for :meth:`mlp_sample_actions`, ``O = 1`` a critic.  ``backward``:
        ``"torch"`` (ordinary f32 torch on the saved activations) or ``"device"`` (:meth:`mlp_backward`: bit-defined)."""
        return MlpHead(self, H, O, activation, L, backward)

    def _mlp_forward(self, head: "MlpHead", x: torch.Tensor, y: torch.Tensor, hidden: torch.Tensor | None) -> None:
        self._enqueue(self._lib.ccx_mlp_forward, x.numel() // head.L, head.L, head.H, head.O, head.activation_id, x,
                      head.w1t, head.b1, head.w2, head.b2, y, hidden)

    def _workspace_arg(self, need: int, workspace: torch.Tensor | None, alloc_name: str) -> torch.Tensor:
        """The workspace of a call that needs ``need`` bytes: the caller's, checked, or one from torch's allocator (so a call
        inside a graph capture stays capturable)."""
        if workspace is None:
            return self._new((max(8, need),), torch.uint8)
        # (inline: a minimum length, not a shape, and the alignment is part of the one message)
        if (not isinstance(workspace, torch.Tensor) or workspace.dtype is not torch.uint8 or workspace.device != self.device
                or workspace.dim() != 1 or workspace.numel() < need or not workspace.is_contiguous() or workspace.data_ptr() % 8):
            raise ValueError(f"workspace must be a contiguous, 8-byte aligned torch.uint8 tensor of at least {need} bytes on "
                             f"{self.device} ({alloc_name})")
        return workspace

    def _mlp_backward_workspace(self, dims, rows: int, workspace: torch.Tensor | None) -> torch.Tensor:
        return self._workspace_arg(int(self._lib.ccx_mlp_backward_workspace_bytes(int(rows), *dims[:3])), workspace,
                                   "alloc_mlp_backward")

    def _check_head(self, head) -> None:
        if not isinstance(head, MlpHead) or head.batch is not self:
            raise ValueError("head must be an MlpHead of this batch (mlp_head)")
        head._check_parameters()

    def alloc_mlp_backward(self, head: "MlpHead", shape, want_grad_a: bool = False) -> "MlpGradResult":
        """Static buffers of :meth:`mlp_backward` for rows of the leading shape ``shape``: the four gradients, ``grad_a`` if
        asked for, and the workspace (for a captured graph)."""
        self._check_head(head)
        shape = tuple(int(v) for v in shape)
        rows = int(np.prod(shape)) if shape else 1
        f = torch.float32
        return MlpGradResult(self._new((head.L, head.H), f), self._new((head.H,), f), self._new((head.O, head.H), f),
                             self._new((head.O,), f), self._new(shape + (head.H,), f) if want_grad_a else None,
                             self._mlp_backward_workspace(head.dims, max(rows, 1), None))

    def _mlp_backward(self, dims, x, hidden, grad_y, w2, out: "MlpGradResult") -> "MlpGradResult":
        """:meth:`mlp_backward` on explicit sizes ``dims`` = (L, H, O, activation id) and an explicit ``w2``; ``out`` holds
        the four gradients, ``grad_a`` or ``None`` and a workspace or ``None``."""
        L, H, O, act = dims
        lead = tuple(x.shape[:-1]) if isinstance(x, torch.Tensor) else ()
        f = torch.float32
        _require_all(self.device,
                     ("x", x, f, (..., L), {"align": 16}), ("hidden", hidden, f, lead + (H,), {"align": 16}),
                     ("grad_y", grad_y, f, lead + (O,)), ("w2", w2, f, (O, H)),
                     ("out.w1t", out.w1t, f, (L, H)), ("out.b1", out.b1, f, (H,)), ("out.w2", out.w2, f, (O, H)),
                     ("out.b2", out.b2, f, (O,)), ("out.grad_a", out.grad_a, f, lead + (H,), {"optional": True, "align": 16}))
        rows = x.numel() // L
        if rows == 0:
            for t in (out.w1t, out.b1, out.w2, out.b2):
                t.zero_()
            return out
        workspace = self._mlp_backward_workspace(dims, rows, out.workspace)
        x, hidden, grad_y, w2 = x.detach(), hidden.detach(), grad_y.detach(), w2.detach()
        self._enqueue(self._lib.ccx_mlp_backward, rows, L, H, O, act, x, hidden, grad_y, w2, workspace, out.w1t, out.b1,
                      out.w2, out.b2, out.grad_a)
        return out

    def mlp_backward(self, head: "MlpHead", x: torch.Tensor, hidden: torch.Tensor, grad_y: torch.Tensor,
                     want_grad_a: bool = False, out: "MlpGradResult | None" = None) -> "MlpGradResult":
        """The gradients of ``head``'s four parameter arrays from the gradient of its outputs, on the device
        (``ccx_mlp_backward``, include/ccx.h CCX_MLP): two kernels on the handle's stream, bit-defined -- f32 per row, then
        f64 chains over blocks of 256 rows and CCX_PPO_LOSS's final step, a tree fixed by the number of rows alone -- so the
        same rows give the same gradient bits on any machine, eager or captured.

        ``x`` f32 [..., L] (contiguous, 16-byte aligned), ``hidden`` f32 [..., H] (what the forward saved: ``head(x,
        hidden_out=)``; 16-byte aligned), ``grad_y`` f32 [..., O].  ``want_grad_a`` also returns the gradient at the
        pre-activations, f32 [..., H] (``grad_a @ w1t.t()`` is the gradient with respect to ``x``, which the library does not
        form).  ``out`` reuses a result of :meth:`alloc_mlp_backward` (its ``grad_a`` decides, ``want_grad_a`` is then
        ignored); otherwise the workspace comes from torch's allocator, so the call captures.  A wrong dtype, shape or
        device, a non-contiguous tensor, a misaligned pointer or a workspace that is too small raises ``ValueError`` before
        the library is called; zero rows return zeros without calling it.
        Only enqueues (no host synchronisation); stream order: :class:`LearnerOps`."""
        self._check_head(head)
        _require_out(out, MlpGradResult, "alloc_mlp_backward")
        if out is None:
            f = torch.float32
            lead = tuple(x.shape[:-1]) if isinstance(x, torch.Tensor) else ()
            out = MlpGradResult(self._new((head.L, head.H), f), self._new((head.H,), f), self._new((head.O, head.H), f),
                                self._new((head.O,), f), self._new(lead + (head.H,), f) if want_grad_a else None, None)
        return self._mlp_backward(head.dims, x, hidden, grad_y, head.w2, out)

    def mlp_sample_actions(self, head: "MlpHead", obs: torch.Tensor, masks: torch.Tensor | None = None,
                           deterministic: bool = False, want_logp: bool = True, want_entropy: bool = False,
                           logits_out: torch.Tensor | None = None, out: SampleResult | None = None) -> SampleResult:
        """Observation rows to actions in ONE launch (``ccx_mlp_sample_actions``): by definition
        ``sample_actions(head(obs), ...)`` -- the same key, the same rule for terminated or truncated agents, the same bits
        in ``actions``, ``logp`` and ``entropy`` -- without the logits' round trip through memory and without the second
        launch.  ``head`` is an :class:`MlpHead` with ``O == 5`` and ``L == obs_len``; ``obs`` f32 [E, N, L] (contiguous,
        16-byte aligned: the ``obs`` of :meth:`step` / :meth:`rollout`); ``logits_out`` f32 [E, N, 5] receives the logits of
        every slot, dead ones included.  ``masks``, ``deterministic``, ``want_*`` and ``out`` are :meth:`sample_actions`'.
        No gradient flows through this call (the update re-evaluates stored rows with ``head(rows)``).  Anything else than
        the tensors described raises ``ValueError`` before the library is called.
        Only enqueues (no host synchronisation); stream order: :class:`LearnerOps`."""
        E, N = self.num_envs, self.num_agents
        if not isinstance(head, MlpHead) or head.batch is not self:
            raise ValueError("head must be an MlpHead of this batch (mlp_head)")
        if head.O != 5 or head.L != self.obs_len:
            raise ValueError(f"mlp_sample_actions needs a head with O == 5 and L == obs_len == {self.obs_len}, got O = {head.O}, L = {head.L}")
        head._check_parameters()
        _require_out(out, SampleResult, "alloc_sample")
        if out is None:
            out = self.alloc_sample(want_logp, want_entropy)
        _require_all(self.device,
                     ("obs", obs, torch.float32, (E, N, self.obs_len), {"align": 16}), ("masks", masks, torch.uint8, (E, N), _OPT),
                     ("logits_out", logits_out, torch.float32, (E, N, 5), _OPT),
                     ("out.actions", out.actions, torch.uint8, (E, N)), ("out.logp", out.logp, torch.float32, (E, N), _OPT),
                     ("out.entropy", out.entropy, torch.float32, (E, N), _OPT))
        self._enqueue(self._lib.ccx_mlp_sample_actions, head.H, head.activation_id, obs, head.w1t, head.b1, head.w2, head.b2,
                      masks, int(bool(deterministic)), out.actions, out.logp, out.entropy, logits_out)
        return out

    # ------------------------------------------------------------------ stored actions under new logits
    def alloc_evaluate(self, shape, want_entropy: bool = True) -> EvalResult:
        """Output tensors of :meth:`evaluate_actions` for rows of the leading shape ``shape`` (static buffers for a
        captured graph)."""
        shape = tuple(int(x) for x in shape)
        return EvalResult(self._new(shape, torch.float32), self._new(shape, torch.float32) if want_entropy else None)

    def _check_evaluate(self, logits, actions, masks, extra=()):
        """The input checks :meth:`evaluate_actions` and :meth:`evaluate_actions_backward` share; returns the leading shape."""
        lead = tuple(logits.shape[:-1]) if isinstance(logits, torch.Tensor) else ()
        _require_all(self.device,
                     ("logits", logits, torch.float32, (..., 5), {"align": 16}),
                     ("actions", actions, torch.uint8, lead, {"hint": " (cast stored actions to torch.uint8 first)"}),
                     ("masks", masks, torch.uint8, lead, _OPT), *extra)
        return lead

    def _evaluate_forward(self, logits, actions, masks, out: EvalResult) -> None:
        self._enqueue(self._lib.ccx_evaluate_actions, actions.numel(), logits, actions, masks, out.logp, out.entropy)

    def _current_stream_waits(self, *tensors, cur=False) -> None:
        """The exit of every enqueueing method (rules (b) and (c) of the class docstring): when torch's CURRENT stream is
        not the handle's, it waits for the handle's stream, so whatever consumes the results there runs behind the
        launches, and ``tensors`` (outputs not yet handed to :meth:`_order_after_current_stream`) are recorded for the
        handle's stream.  ``cur``: what :meth:`_other_stream` answered earlier in the same call (default: ask now)."""
        if cur is False:
            cur = self._other_stream()
        if cur is not None:
            cur.wait_stream(self._stream)
            for t in tensors:
                if t is not None and t.is_cuda:
                    t.record_stream(self._stream)

    def evaluate_actions(self, logits: torch.Tensor, actions: torch.Tensor, masks: torch.Tensor | None = None,
                         want_entropy: bool = True, out: EvalResult | None = None) -> EvalResult:
        """``log pi_new(stored action | state)`` and the entropy of the masked distribution under new logits, on the device
        (``ccx_evaluate_actions``, include/ccx.h CCX_EVALUATE): one kernel on the handle's stream, bit-defined, and the very
        distribution :meth:`sample_actions` draws from -- on the logits an action was sampled from, ``logp`` and
        ``entropy`` equal the sampler's bit for bit.

        ``logits`` f32 [..., 5] (contiguous, 16-byte aligned); ``actions`` u8 [...] (what :meth:`sample_actions` stored; cast
        int64 actions first); ``masks`` u8 [...] or ``None`` (everything legal).  Rows whose action is 255 give ``logp`` =
        ``entropy`` = +0.0 whatever their logits hold; an action that is out of range or illegal under its mask gives
        ``logp`` = -inf.  Anything else than the tensors described raises ``ValueError`` before the library is called;
        zero rows return empty tensors without calling it.

        When ``logits.requires_grad`` and grad mode is on, the call is a ``torch.autograd.Function``: its backward is
        ``ccx_evaluate_actions_backward`` (one kernel; illegal places, 255 rows and degenerate rows get exactly +0.0, selected,
        so a NaN there never reaches a gradient), an output the loss did not use is passed as NULL, and ``out=`` is refused.
        Otherwise this is the plain forward and ``out=`` reuses an :class:`EvalResult` (:meth:`alloc_evaluate`).  Only
        enqueues."""
        lead = self._check_evaluate(logits, actions, masks)
        if logits.requires_grad and torch.is_grad_enabled():
            if out is not None:
                raise ValueError("out= cannot be used when logits require a gradient (the autograd path allocates its outputs)")
            if logits.numel() == 0:
                zero = logits.sum(-1) * 0.0
                return EvalResult(zero, zero.clone() if want_entropy else None)
            logp, entropy = _EvaluateActions.apply(self, logits, actions, masks, bool(want_entropy))
            return EvalResult(logp, entropy)
        _require_out(out, EvalResult, "alloc_evaluate")
        if out is None:
            out = self.alloc_evaluate(lead, want_entropy)
        self._check_evaluate(logits, actions, masks, (("out.logp", out.logp, torch.float32, lead),
                                                      ("out.entropy", out.entropy, torch.float32, lead, _OPT)))
        if logits.numel():
            self._evaluate_forward(logits, actions, masks, out)
        return out

    def evaluate_actions_backward(self, logits: torch.Tensor, actions: torch.Tensor, masks: torch.Tensor | None,
                                  grad_logp: torch.Tensor | None, grad_entropy: torch.Tensor | None,
                                  out: torch.Tensor | None = None) -> torch.Tensor:
        """The gradient of :meth:`evaluate_actions` with respect to ``logits`` from the gradients of its two outputs
        (``ccx_evaluate_actions_backward``): one kernel that recomputes the forward quantities from the logits.  Either of
        ``grad_logp`` / ``grad_entropy`` (f32, the leading shape of ``logits``) may be ``None``, not both.  ``out`` reuses a
        f32 tensor of the shape of ``logits`` (16-byte aligned): with :meth:`evaluate_actions` ``(out=)`` the static-buffer
        pair for a captured graph.
        Only enqueues (no host synchronisation); stream order: :class:`LearnerOps`."""
        if grad_logp is None and grad_entropy is None:
            raise ValueError("at least one of grad_logp and grad_entropy is required")
        if out is None and isinstance(logits, torch.Tensor):
            out = torch.empty_like(logits, requires_grad=False)
        lead = tuple(logits.shape[:-1]) if isinstance(logits, torch.Tensor) else ()
        self._check_evaluate(logits, actions, masks, (
            ("grad_logp", grad_logp, torch.float32, lead, _OPT), ("grad_entropy", grad_entropy, torch.float32, lead, _OPT),
            ("out", out, torch.float32, lead + (5,), {"align": 16})))
        if logits.numel():
            self._enqueue(self._lib.ccx_evaluate_actions_backward, actions.numel(), logits, actions, masks, grad_logp,
                          grad_entropy, out)
        return out

    # ------------------------------------------------------------------ the PPO loss over the rows that count
    def alloc_ppo_loss(self, shape, want_logits_grad: bool = True, want_values_grad: bool = True) -> PpoLossResult:
        """Static buffers of :meth:`ppo_loss` / :meth:`ppo_loss_backward` for rows of the leading shape ``shape``: stats,
        the workspace and the two gradients (for a captured graph)."""
        shape, stats, workspace = _alloc_loss(self, PpoLossResult, shape)
        return PpoLossResult(stats[0], stats, workspace,
                             self._new(shape + (5,), torch.float32) if want_logits_grad else None,
                             self._new(shape, torch.float32) if want_values_grad else None)

    @staticmethod
    def _check_ppo_hyper(clip, vf_coef, ent_coef, adv_eps):
        clip, vf_coef, ent_coef, adv_eps = float(clip), float(vf_coef), float(ent_coef), float(adv_eps)
        if not 0.0 < clip < 1.0:                                     # (false for NaN)
            raise ValueError(f"clip must lie in (0, 1), got {clip!r}")
        for name, x in (("vf_coef", vf_coef), ("ent_coef", ent_coef), ("adv_eps", adv_eps)):
            if not 0.0 <= x < float("inf"):
                raise ValueError(f"{name} must be finite and not negative, got {x!r}")
        return clip, vf_coef, ent_coef, adv_eps

    def _check_ppo(self, logits, values, actions, logp_old, advantages, returns, masks, valid, norm):
        """The input checks of :meth:`ppo_loss` and :meth:`ppo_loss_backward`; returns (leading shape, norm f32 [2] or None)."""
        lead = self._check_evaluate(logits, actions, masks, (
            ("values", values, torch.float32, tuple(logits.shape[:-1]) if isinstance(logits, torch.Tensor) else ()),))
        _require_all(self.device, ("logp_old", logp_old, torch.float32, lead), ("advantages", advantages, torch.float32, lead),
                     ("returns", returns, torch.float32, lead), ("valid", valid, torch.uint8, lead, _OPT))
        if norm is not None:                                         # (inline: one message for either of two shapes)
            if (not isinstance(norm, torch.Tensor) or norm.dtype is not torch.float32 or norm.device != self.device
                    or tuple(norm.shape) not in ((2,), (4,)) or not norm.is_contiguous()):
                raise ValueError(f"norm must be a contiguous torch.float32 tensor on {self.device}: masked_moments' [4] "
                                 "(n, mean, std, 0) or [2] (mean, std)")
            if norm.shape[0] == 4:
                norm = norm[1:3]
        return lead, norm

    def masked_moments(self, x: torch.Tensor, valid: torch.Tensor | None = None, out: torch.Tensor | None = None,
                       workspace: torch.Tensor | None = None) -> torch.Tensor:
        """``[n, mean, std, 0]`` (f32 [4] on the device) of ``x`` f32 [...] over the elements where ``valid`` u8 [...] is not
        zero (``None``: all), by ``ccx_masked_moments`` (include/ccx.h CCX_PPO_LOSS): two kernels on the handle's stream, a
        fixed f64 tree, bit-defined, no host synchronisation.  ``std`` is the unbiased one; ``n < 2`` gives mean 0, std 1.
        Hand the result to :meth:`ppo_loss` as ``norm=``.  ``out`` / ``workspace`` reuse buffers (a captured graph).  Zero
        elements return ``[0, 0, 1, 0]`` without calling the library.
        Only enqueues (no host synchronisation); stream order: :class:`LearnerOps`."""
        _require("x", x, torch.float32, None, self.device)
        _require("valid", valid, torch.uint8, x.shape, self.device, optional=True)
        if out is None:
            out = self._new((4,), torch.float32)
        _require("out", out, torch.float32, (4,), self.device)
        rows = x.numel()
        if rows == 0:
            out.copy_(torch.tensor([0.0, 0.0, 1.0, 0.0], dtype=torch.float32))
            return out
        workspace = _loss_workspace(self, PpoLossResult, workspace, rows)
        self._enqueue(self._lib.ccx_masked_moments, rows, x, valid, workspace, out)
        return out

    def _ppo_forward(self, logits, values, actions, logp_old, advantages, returns, masks, valid, norm, hyper, workspace, stats):
        self._enqueue(self._lib.ccx_ppo_loss, actions.numel(), logits, actions, masks, logp_old, advantages, returns, values,
                      valid, norm, *hyper, workspace, stats)

    def ppo_loss(self, logits: torch.Tensor, values: torch.Tensor, actions: torch.Tensor, logp_old: torch.Tensor,
                 advantages: torch.Tensor, returns: torch.Tensor, masks: torch.Tensor | None = None,
                 valid: torch.Tensor | None = None, norm: torch.Tensor | None = None, clip: float = 0.2, vf_coef: float = 0.5,
                 ent_coef: float = 0.01, adv_eps: float = 1e-8, out: PpoLossResult | None = None) -> PpoLossResult:
        """The clipped-surrogate PPO loss ``policy + vf_coef * value - ent_coef * entropy`` over the rows that count, on
        the device (``ccx_ppo_loss``, include/ccx.h CCX_PPO_LOSS): two kernels on the handle's stream, bit-defined (the
        reduction is a fixed f64 tree), shapes static -- ``valid`` is a selection inside the kernel, so nothing is
        compacted, nothing synchronises with the host, and the whole update captures into a graph.

        ``logits`` f32 [..., 5] (contiguous, 16-byte aligned), everything else [...]: ``values`` f32 (the critic's, new
        weights), ``actions`` u8 and ``masks`` u8 or ``None`` as in :meth:`evaluate_actions`, ``logp_old`` f32
        (:meth:`sample_actions`' logp), ``advantages`` / ``returns`` f32 and ``valid`` u8 (:meth:`compute_gae`'s).  A row
        counts iff its ``valid`` byte is not zero and its action is not 255.  ``norm``: :meth:`masked_moments`' result
        (or a [2] = mean, std): advantages enter as ``(a - mean) / (std + adv_eps)``.  The result's ``stats`` holds loss,
        policy, value, entropy, approx_kl (mean of ``ratio - 1 - log ratio``), clip_frac, count, 0.

        When ``logits`` or ``values`` requires grad and grad mode is on, the call is a ``torch.autograd.Function``:
        ``r.loss.backward()`` reaches both through ``ccx_ppo_loss_backward`` (one kernel; rows that do not count get exactly
        +0.0), ``None`` goes to the one that does not require grad, ``out=`` is refused, and the workspace comes from
        torch's allocator, so the call captures.  Otherwise ``out=`` reuses a result of :meth:`alloc_ppo_loss`.  A wrong
        dtype, shape or device, a non-contiguous tensor, a misaligned pointer or a bad hyperparameter raises ``ValueError``
        before the library is called; zero rows return zeros without calling it.
        Only enqueues (no host synchronisation); stream order: :class:`LearnerOps`."""
        hyper = self._check_ppo_hyper(clip, vf_coef, ent_coef, adv_eps)
        lead, norm = self._check_ppo(logits, values, actions, logp_old, advantages, returns, masks, valid, norm)
        return _loss_over_rows(self, PpoLossResult, self, _PpoLoss, self._ppo_forward, (logits, values),
                               (actions, logp_old, advantages, returns, masks, valid, norm, hyper), actions.numel(), (), out)

    def ppo_loss_backward(self, logits: torch.Tensor, values: torch.Tensor, actions: torch.Tensor, logp_old: torch.Tensor,
                          advantages: torch.Tensor, returns: torch.Tensor, masks: torch.Tensor | None = None,
                          valid: torch.Tensor | None = None, norm: torch.Tensor | None = None, clip: float = 0.2,
                          vf_coef: float = 0.5, ent_coef: float = 0.01, adv_eps: float = 1e-8, *, stats: torch.Tensor,
                          grad_loss: torch.Tensor | None = None, want_logits_grad: bool = True, want_values_grad: bool = True,
                          out: PpoLossResult | None = None):
        """``(grad_logits, grad_values)`` of :meth:`ppo_loss`'s ``loss`` (``ccx_ppo_loss_backward``: one kernel that recomputes
        the forward terms from the same inputs and the forward's ``stats``).  ``grad_loss`` f32 [1] or 0-dim on the device
        (``None`` = 1).  ``want_*`` choose the outputs (at least one; the other is returned as ``None`` and not computed);
        ``out`` reuses the gradients of an :meth:`alloc_ppo_loss` result instead (one of them may be ``None``).  Only
        enqueues."""
        hyper = self._check_ppo_hyper(clip, vf_coef, ent_coef, adv_eps)
        lead, norm = self._check_ppo(logits, values, actions, logp_old, advantages, returns, masks, valid, norm)
        _require("stats", stats, torch.float32, (8,), self.device)
        _check_grad_loss(grad_loss, self.device)
        _require_out(out, PpoLossResult, "alloc_ppo_loss")
        if out is None:
            gl = torch.empty_like(logits, requires_grad=False) if want_logits_grad else None
            gv = torch.empty_like(values, requires_grad=False) if want_values_grad else None
        else:
            gl, gv = out.grad_logits, out.grad_values
        if gl is None and gv is None:
            raise ValueError("at least one of the two gradients is required")
        _require_all(self.device, ("grad_logits", gl, torch.float32, lead + (5,), {"optional": True, "align": 16}),
                     ("grad_values", gv, torch.float32, lead, _OPT))
        if logits.numel():
            logits, values = logits.detach(), values.detach()
            self._enqueue(self._lib.ccx_ppo_loss_backward, actions.numel(), logits, actions, masks, logp_old, advantages,
                          returns, values, valid, norm, *hyper, stats, grad_loss, gl, gv)
        return gl, gv

    # ------------------------------------------------------------------ the optimiser step
    def adam(self, params, lr: float = 3e-4, betas=(0.9, 0.999), eps: float = 1e-8, weight_decay: float = 0.0,
             max_grad_norm: float = 0.0) -> "DeviceAdam":
        """An optimiser over ``params`` (up to 32 f32 tensors of this batch's device, e.g. ``[*actor.parameters(),
        *critic.parameters()]``) whose step is ``ccx_adam_step`` (include/ccx.h CCX_ADAM): the global gradient norm by a
        fixed f64 tree, the clip at ``max_grad_norm`` (0: none) and Adam with decoupled weight decay, bit-defined, the step
        count on the device -- three launches on the handle's stream that capture into a graph.  See :class:`DeviceAdam`."""
        return DeviceAdam(self, params, lr, betas, eps, weight_decay, max_grad_norm)

    def _adam_step(self, params, grads, ms, vs, lr: float, lr_dev, hyper, state, workspace, stats) -> None:
        """``ccx_adam_step`` on checked tensors: ``hyper`` = (beta1, beta2, eps, weight_decay, max_grad_norm); ``lr_dev`` f32
        [1] on the device or ``None`` (then ``lr`` by value is the rate)."""
        table =(CcxAdamTensor * len(params))()
        for row, p, g, m, v in zip(table, params, grads, ms, vs):
            row.param, row.grad, row.m, row.v, row.numel = p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), p.numel()
        self._enqueue(self._lib.ccx_adam_step, len(params), table, lr, lr_dev, *hyper, state, workspace, stats,
                      also=(*params, *grads, *ms, *vs))


def _check_adam_hyper(lr, betas, eps, weight_decay, max_grad_norm):
    """The hyper-parameters as the f32 values the library will see, or ``ValueError``: ``(lr, (beta1, beta2, eps,
    weight_decay, max_grad_norm))``."""
    try:
        beta1, beta2 = betas
        vals = [float(np.float32(x)) for x in (lr, beta1, beta2, eps, weight_decay, max_grad_norm)]
    except (TypeError, ValueError):
        raise ValueError("lr, eps, weight_decay and max_grad_norm must be numbers and betas a pair of numbers") from None
    lr, beta1, beta2, eps, weight_decay, max_grad_norm = vals
    inf = float("inf")
    for name, x in (("beta1", beta1), ("beta2", beta2)):
        if not 0.0 <= x < 1.0:                                       # (false for NaN)
            raise ValueError(f"{name} must lie in [0, 1) as a float32, got {x!r}")
    if not 0.0 < eps < inf:
        raise ValueError(f"eps must be finite and positive as a float32, got {eps!r}")
    for name, x in (("lr", lr), ("weight_decay", weight_decay), ("max_grad_norm", max_grad_norm)):
        if not 0.0 <= x < inf:
            raise ValueError(f"{name} must be finite and not negative, got {x!r}")
    return lr, (beta1, beta2, eps, weight_decay, max_grad_norm)


class DeviceAdam:
    """Adam with decoupled weight decay and global-norm gradient clipping over up to 32 f32 tensors, one step =
    ``ccx_adam_step`` (include/ccx.h CCX_ADAM): three launches on the handle's stream, every bit of the new parameters,
    ``m``, ``v`` and of the norm defined by the written rule, so the same gradients give the same update on any machine, eager
    or captured.  Made by :meth:`BatchedCollectiveCrossing.adam`.

    The optimiser owns ``m`` and ``v`` (lists of zeros shaped like the parameters), ``state`` (u8 [64] on the device: the
    running products ``beta^step`` as f64, the step count and the count of skipped steps as i64), the workspace and ``stats``
    (f32 [4] = gradient norm, clip scale, skipped 0 / 1, the rate used; :attr:`grad_norm`, :attr:`scale` and :attr:`skipped`
    are 0-dim views).  A step whose norm is NaN or infinite changes nothing but ``skipped``.  The rate lives in a device
    scalar: ``opt.lr = x`` writes it on the handle's stream, so a schedule works between the replays of a captured graph.

    ``step(grads=None)`` reads every parameter's ``.grad``; ``grads=`` names the gradient tensors instead, in the order of
    the parameters (e.g. the ``w1t, b1, w2, b2`` of an :class:`MlpGradResult` per head: static buffers for a graph).  The
    gradients are read only; the clipped gradient is never stored.  A wrong dtype, shape or device, a non-contiguous or
    misaligned tensor, a missing ``.grad``, more than 32 tensors or a hyper-parameter out of range raises ``ValueError``
    before the library is called.
    Only enqueues (no host synchronisation); stream order: :class:`LearnerOps`."""

    def __init__(self, batch, params, lr=3e-4, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, max_grad_norm=0.0):
        self._lr, self._hyper = _check_adam_hyper(lr, betas, eps, weight_decay, max_grad_norm)
        try:
            params = list(params)
        except TypeError:
            raise ValueError("params must be an iterable of tensors") from None
        if not 1 <= len(params) <= ADAM_MAX_TENSORS:
            raise ValueError(f"params must hold 1..{ADAM_MAX_TENSORS} tensors, got {len(params)}")
        self.batch, self.params = batch, params
        self._check_params()
        dev = batch.device
        self.m = [torch.zeros_like(p, requires_grad=False) for p in params]
        self.v = [torch.zeros_like(p, requires_grad=False) for p in params]
        self.state = torch.zeros((64,), dtype=torch.uint8, device=dev)
        self.state.view(torch.float64)[:2] = 1.0
        self.stats = torch.zeros((4,), dtype=torch.float32, device=dev)
        self._lr_dev = torch.full((1,), self._lr, dtype=torch.float32, device=dev)
        numel = (C.c_int64 * len(params))(*(p.numel() for p in params))
        self.workspace = torch.empty((int(batch._lib.ccx_adam_workspace_bytes(len(params), numel)),), dtype=torch.uint8, device=dev)

    grad_norm = property(lambda self: self.stats[0])
    scale = property(lambda self: self.stats[1])
    skipped = property(lambda self: self.stats[2])

    def _check_params(self) -> None:
        for i, p in enumerate(self.params):
            _require(f"params[{i}]", p, torch.float32, None, self.batch.device, align=16, verb="be and stay")
            if p.numel() < 1:
                raise ValueError(f"params[{i}] must have at least one element")

    @property
    def lr(self) -> float:
        return self._lr

    @lr.setter
    def lr(self, value) -> None:
        self._lr, _ = _check_adam_hyper(value, *self._hyper_args())
        b = self.batch
        cur = b._order_after_current_stream(self._lr_dev)
        with torch.cuda.stream(b._stream):
            self._lr_dev.fill_(self._lr)
        b._current_stream_waits(cur=cur)

    def _hyper_args(self):
        beta1, beta2, eps, weight_decay, max_grad_norm = self._hyper
        return (beta1, beta2), eps, weight_decay, max_grad_norm

    def zero_grad(self, set_to_none: bool = False) -> None:
        """Zero every parameter's ``.grad`` in place (the default: the buffers stay where a graph found them) or drop it."""
        for p in self.params:
            if p.grad is not None:
                if set_to_none:
                    p.grad = None
                else:
                    p.grad.detach_()
                    p.grad.zero_()

    def step(self, grads=None) -> None:
        self._check_params()
        if grads is None:
            grads = [p.grad for p in self.params]
            names = [f"params[{i}].grad" for i in range(len(grads))]
            hint = " (a parameter without .grad: run backward first, or pass grads=)"
        else:
            try:
                grads = list(grads)
            except TypeError:
                raise ValueError("grads must be an iterable of tensors") from None
            if len(grads) != len(self.params):
                raise ValueError(f"grads must hold one tensor per parameter ({len(self.params)}), got {len(grads)}")
            names = [f"grads[{i}]" for i in range(len(grads))]
            hint = ""
        b = self.batch
        _require_all(b.device, *((n, g, torch.float32, tuple(p.shape), {"align": 16, "hint": hint})
                                 for n, g, p in zip(names, grads, self.params)))
        b._adam_step([p.detach() for p in self.params], [g.detach() for g in grads], self.m, self.v, self._lr, self._lr_dev,
                     self._hyper, self.state, self.workspace, self.stats)

    def counts(self) -> tuple[int, int]:
        """``(steps taken, steps skipped)`` from the device state.  Synchronises."""
        self.batch._current_stream_waits()
        step, skipped = self.state.view(torch.int64)[2:4].tolist()
        return int(step), int(skipped)

    def state_dict(self) -> dict:
        """Copies of ``m``, ``v`` and the 64 state bytes, and the hyper-parameters."""
        self.batch._current_stream_waits()
        (beta1, beta2), eps, weight_decay, max_grad_norm = self._hyper_args()
        return {"m": [t.clone() for t in self.m], "v": [t.clone() for t in self.v], "state": self.state.clone(),
                "hyper": {"lr": self._lr, "betas": (beta1, beta2), "eps": eps, "weight_decay": weight_decay,
                          "max_grad_norm": max_grad_norm}}

    def load_state_dict(self, sd: dict) -> None:
        """Continue from a :meth:`state_dict` (of an optimiser over parameters of the same shapes): exact copies."""
        try:
            ms, vs, state, hy = list(sd["m"]), list(sd["v"]), sd["state"], dict(sd["hyper"])
            lr, hyper = _check_adam_hyper(hy["lr"], hy["betas"], hy["eps"], hy["weight_decay"], hy["max_grad_norm"])
        except (KeyError, TypeError):
            raise ValueError("not a DeviceAdam state_dict (keys m, v, state, hyper)") from None
        if len(ms) != len(self.m) or len(vs) != len(self.v):
            raise ValueError(f"the state_dict holds {len(ms)} tensors, the optimiser {len(self.m)}")
        for name, src, dst in (("m", ms, self.m), ("v", vs, self.v)):
            for i, (s, d) in enumerate(zip(src, dst)):
                if not isinstance(s, torch.Tensor) or s.dtype is not torch.float32 or s.shape != d.shape:
                    raise ValueError(f"state_dict {name}[{i}] must be a torch.float32 tensor of shape {tuple(d.shape)}")
        if not isinstance(state, torch.Tensor) or state.dtype is not torch.uint8 or tuple(state.shape) != (64,):
            raise ValueError("state_dict state must be a torch.uint8 tensor of 64 bytes")
        self.batch._current_stream_waits()                           # (a step in flight still reads m, v and the state)
        with torch.no_grad():
            for src, dst in ((ms, self.m), (vs, self.v)):
                for s, d in zip(src, dst):
                    d.copy_(s)
            self.state.copy_(state)
        self._hyper = hyper
        self.lr = lr


class _EvaluateActions(torch.autograd.Function):

    """:meth:`BatchedCollectiveCrossing.evaluate_actions` for logits that require a gradient: forward and backward are
    the two kernels of CCX_EVALUATE; nothing is saved but the inputs."""

    @staticmethod
    def forward(ctx, batch, logits, actions, masks, want_entropy):
        logits = logits.detach()
        out = batch.alloc_evaluate(logits.shape[:-1], want_entropy)
        batch._evaluate_forward(logits, actions, masks, out)
        ctx.batch, ctx.actions, ctx.masks = batch, actions, masks
        ctx.save_for_backward(logits)
        ctx.set_materialize_grads(False)                # an output the loss did not use arrives as None and is passed as NULL
        return out.logp, out.entropy

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_logp, grad_entropy):
        (logits,) = ctx.saved_tensors
        grad_logp = None if grad_logp is None else grad_logp.contiguous()
        grad_entropy = None if grad_entropy is None else grad_entropy.contiguous()
        if grad_logp is None and grad_entropy is None:
            return None, None, None, None, None
        grad = ctx.batch.evaluate_actions_backward(logits, ctx.actions, ctx.masks, grad_logp, grad_entropy)
        return None, grad, None, None, None


class _PpoLoss(torch.autograd.Function):
    """:meth:`BatchedCollectiveCrossing.ppo_loss` for logits or values that require a gradient: the forward is the two
    kernels of ``ccx_ppo_loss``, the backward the one of ``ccx_ppo_loss_backward``; nothing is saved but the inputs and
    ``stats``.  Only ``stats[0]``, the loss, is differentiable: the gradient arriving at the other seven is not read."""

    @staticmethod
    def forward(ctx, batch, logits, values, actions, logp_old, advantages, returns, masks, valid, norm, hyper):
        logits, values = logits.detach(), values.detach()
        stats = _new_stats(batch.device)
        batch._ppo_forward(logits, values, actions, logp_old, advantages, returns, masks, valid, norm, hyper,
                           _loss_workspace(batch, PpoLossResult, None, actions.numel()), stats)
        ctx.batch, ctx.hyper = batch, hyper
        ctx.rest = (actions, logp_old, advantages, returns, masks, valid, norm)
        ctx.save_for_backward(logits, values, stats)
        return stats

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_stats):
        logits, values, stats = ctx.saved_tensors
        actions, logp_old, advantages, returns, masks, valid, norm = ctx.rest
        want_l, want_v = ctx.needs_input_grad[1], ctx.needs_input_grad[2]
        gl, gv = ctx.batch.ppo_loss_backward(logits, values, actions, logp_old, advantages, returns, masks, valid, norm,
                                             *ctx.hyper, stats=stats, grad_loss=grad_stats.contiguous(),
                                             want_logits_grad=want_l, want_values_grad=want_v)
        return (None, gl, gv) + (None,) * 8


MLP_ACTIVATIONS = {"tanh": 0, "relu": 1}
MLP_BACKWARDS = ("torch", "device")


class _TwoLayerHead(torch.nn.Module):
    """What :class:`MlpHead` and :class:`~collectivecrossing_amd.wide.WideMlpHead` share, stated once: the argument checks, the
    four parameters in the kernels' layout with ``torch.nn.Linear``'s initialisation, and the exact conversions.  No method
    here reaches the library."""

    MAX_OUTPUTS = 8

    def _setup(self, batch, H, O, activation, L, backward) -> None:
        L = batch.obs_len if L is None else L
        for name, v, lo, hi in (("L", L, 1, 512), ("H", H, 16, 256), ("O", O, 1, self.MAX_OUTPUTS)):
            if not isinstance(v, int) or isinstance(v, bool) or not lo <= v <= hi:
                raise ValueError(f"{name} must be an int in {lo}..{hi}, got {v!r}")
        if H % 16:
            raise ValueError(f"H must be a multiple of 16, got {H}")
        if activation not in MLP_ACTIVATIONS:
            raise ValueError(f"activation must be one of {sorted(MLP_ACTIVATIONS)}, got {activation!r}")
        if backward not in MLP_BACKWARDS:
            raise ValueError(f"backward must be one of {list(MLP_BACKWARDS)}, got {backward!r}")
        self.backward = backward
        object.__setattr__(self, "batch", batch)                          # (not a submodule, not part of the state dict)
        self.L, self.H, self.O, self.activation = L, H, O, activation
        self.activation_id = MLP_ACTIVATIONS[activation]
        self.dims = (L, H, O, self.activation_id)
        lin1, lin2 = torch.nn.Linear(L, H), torch.nn.Linear(H, O)
        dev = batch.device
        self.w1t = torch.nn.Parameter(lin1.weight.detach().t().contiguous().to(dev))
        self.b1 = torch.nn.Parameter(lin1.bias.detach().clone().to(dev))
        self.w2 = torch.nn.Parameter(lin2.weight.detach().clone().to(dev))
        self.b2 = torch.nn.Parameter(lin2.bias.detach().clone().to(dev))

    @staticmethod
    def _check_linear_pair(lin1, lin2) -> None:
        if (not isinstance(lin1, torch.nn.Linear) or not isinstance(lin2, torch.nn.Linear) or lin1.bias is None
                or lin2.bias is None or lin1.out_features != lin2.in_features or lin1.weight.dtype is not torch.float32
                or lin2.weight.dtype is not torch.float32):
            raise ValueError("from_linear needs two f32 torch.nn.Linear layers with biases, lin1.out_features == lin2.in_features")

    def _copy_linear_pair(self, lin1, lin2):
        with torch.no_grad():
            self.w1t.copy_(lin1.weight.t())
            self.b1.copy_(lin1.bias)
            self.w2.copy_(lin2.weight)
            self.b2.copy_(lin2.bias)
        return self

    def to_sequential(self, dtype: torch.dtype = torch.float32) -> torch.nn.Sequential:
        """``Sequential(Linear(L, H), Tanh | ReLU, Linear(H, O))`` with exact copies of the parameters (cast to ``dtype``)."""
        lin1 = torch.nn.Linear(self.L, self.H, device=self.w1t.device, dtype=dtype)
        lin2 = torch.nn.Linear(self.H, self.O, device=self.w1t.device, dtype=dtype)
        with torch.no_grad():
            lin1.weight.copy_(self.w1t.t())
            lin1.bias.copy_(self.b1)
            lin2.weight.copy_(self.w2)
            lin2.bias.copy_(self.b2)
        return torch.nn.Sequential(lin1, torch.nn.Tanh() if self.activation == "tanh" else torch.nn.ReLU(), lin2)

    def _check_parameters(self) -> None:
        for name, shape in (("w1t", (self.L, self.H)), ("b1", (self.H,)), ("w2", (self.O, self.H)), ("b2", (self.O,))):
            _require(name, getattr(self, name), torch.float32, shape, self.batch.device, verb="stay")


def _torch_head_backward(relu: bool, need, gy, x, w1t, w2, hidden):
    """The f32 torch composition of a head's backward on the saved activations (``backward="torch"``: correct to rounding, not
    bit-defined): ``(None, grad_x, grad_w1t, grad_b1, grad_w2, grad_b2)`` as an autograd Function returns them."""
    L, H, O = x.shape[-1], hidden.shape[-1], w2.shape[0]
    gy, h, x2 = gy.contiguous().reshape(-1, O), hidden.reshape(-1, H), x.reshape(-1, L)
    gh = gy @ w2
    ga = gh * (h > 0) if relu else gh * (1.0 - h * h)
    gx = (ga @ w1t.t()).reshape(x.shape) if need[1] else None
    gw1t = x2.t() @ ga if need[2] else None
    gb1 = ga.sum(0) if need[3] else None
    gw2 = gy.t() @ h if need[4] else None
    gb2 = gy.sum(0) if need[5] else None
    return None, gx, gw1t, gb1, gw2, gb2


class MlpHead(_TwoLayerHead):
    """``Linear(L, H) -> tanh | relu -> Linear(H, O)`` on the batch's device, forward in ONE kernel on the handle's stream
    (``ccx_mlp_forward``, include/ccx.h CCX_MLP).  The outputs of a row are a fixed sequence of f32 operations on that row:
    they do not depend on how many rows the call holds or where the row sits, so ``head(rows)`` on a ``[K, E, N, L]``
    minibatch reproduces, bit for bit, the logits :meth:`BatchedCollectiveCrossing.mlp_sample_actions` drew an action from.

    The parameters are stored in the kernel's layout -- ``w1t`` [L, H] (the first layer INPUT-major:
    ``Linear(L, H).weight.t()``), ``b1`` [H], ``w2`` [O, H], ``b2`` [O] -- so an optimiser updates what the kernel reads and
    no packing launch sits in the loop.  They are initialised as ``torch.nn.Linear`` initialises (the two layers drawn in
    order from torch's generator); :meth:`from_linear` and :meth:`to_sequential` convert by exact copies.

    ``head(x, out=None, hidden_out=None)``: ``x`` f32 [..., L], contiguous, 16-byte aligned, on the batch's device; returns
    f32 [..., O].  Without grad this is the one launch, ``out=`` reuses a tensor and ``hidden_out=`` (f32 [..., H], 16-byte
    aligned) receives the activations: with :meth:`BatchedCollectiveCrossing.mlp_backward` ``(out=)`` the static-buffer
    forward / backward pair for a captured graph.  When grad mode is on and a parameter or ``x`` requires a gradient, the
    call is a ``torch.autograd.Function``: the forward is the same kernel -- the same bits -- with the hidden activations
    saved, ``out=`` and ``hidden_out=`` are refused, and the backward is chosen by ``backward``: ``"torch"`` (the default) is
    a torch composition on those activations (matrix products and sums in ordinary f32: correct to rounding, NOT
    bit-defined); ``"device"`` is ``ccx_mlp_backward``, whose four parameter gradients are bit-defined (the gradient with
    respect to ``x``, formed only when ``x`` requires one, stays a torch product).  Anything else than the tensors described
    raises ``ValueError`` before the library is called; zero rows return an empty tensor without calling it."""

    def __init__(self, batch: BatchedCollectiveCrossing, H: int, O: int = 5, activation: str = "tanh", L: int | None = None,
                 backward: str = "torch"):
        super().__init__()
        self._setup(batch, H, O, activation, L, backward)

    @classmethod
    def from_linear(cls, batch: BatchedCollectiveCrossing, lin1: torch.nn.Linear, lin2: torch.nn.Linear,
                    activation: str = "tanh", backward: str = "torch") -> "MlpHead":
        """The head that computes ``lin2(act(lin1(x)))``: exact copies of the two layers' f32 parameters."""
        cls._check_linear_pair(lin1, lin2)
        return cls(batch, lin1.out_features, lin2.out_features, activation, lin1.in_features, backward)._copy_linear_pair(lin1, lin2)

    def extra_repr(self) -> str:
        return f"L={self.L}, H={self.H}, O={self.O}, activation={self.activation}, backward={self.backward}"

    def forward(self, x: torch.Tensor, out: torch.Tensor | None = None, hidden_out: torch.Tensor | None = None) -> torch.Tensor:
        b = self.batch
        _require("x", x, torch.float32, (..., self.L), b.device, align=16)
        self._check_parameters()
        shape = tuple(x.shape[:-1]) + (self.O,)
        if torch.is_grad_enabled() and (x.requires_grad or any(p.requires_grad for p in self.parameters())):
            if out is not None or hidden_out is not None:
                raise ValueError("out= and hidden_out= cannot be used when a gradient is required (the autograd path allocates "
                                 "its outputs)")
            if x.numel() == 0:
                return x.new_zeros(shape) + self.b2 * 0.0
            return _MlpForward.apply(self, x, self.w1t, self.b1, self.w2, self.b2)
        if out is None:
            out = b._new(shape, torch.float32)
        else:
            _require("out", out, torch.float32, shape, b.device)
        _require("hidden_out", hidden_out, torch.float32, tuple(x.shape[:-1]) + (self.H,), b.device, optional=True, align=16)
        if x.numel():
            b._mlp_forward(self, x.detach(), out, hidden_out)
        return out


class _MlpForward(torch.autograd.Function):
    """:class:`MlpHead` when a gradient is required: the forward is the kernel of CCX_MLP with the activations saved; the
    backward is ordinary f32 torch on them (``backward="torch"``: not bit-defined) or ``ccx_mlp_backward`` (``"device"``:
    the four parameter gradients bit-defined; the gradient of ``x``, where required, a torch product on its ``grad_a``)."""

    @staticmethod
    def forward(ctx, head, x, w1t, b1, w2, b2):
        x = x.detach()
        b = head.batch
        y = b._new(tuple(x.shape[:-1]) + (head.O,), torch.float32)
        hidden = b._new(tuple(x.shape[:-1]) + (head.H,), torch.float32)
        b._mlp_forward(head, x, y, hidden)
        ctx.relu = head.activation == "relu"
        ctx.batch, ctx.dims, ctx.device_backward = b, head.dims, head.backward == "device"
        ctx.save_for_backward(x, w1t.detach(), w2.detach(), hidden)
        return y

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, gy):
        x, w1t, w2, hidden = ctx.saved_tensors
        L, H, O = x.shape[-1], hidden.shape[-1], gy.shape[-1]
        need = ctx.needs_input_grad
        if ctx.device_backward:
            b, f = ctx.batch, torch.float32
            out = MlpGradResult(b._new((L, H), f), b._new((H,), f), b._new((O, H), f), b._new((O,), f),
                                b._new(tuple(hidden.shape), f) if need[1] else None, None)
            b._mlp_backward(ctx.dims, x, hidden, gy.contiguous(), w2, out)
            gx = (out.grad_a.reshape(-1, H) @ w1t.t()).reshape(x.shape) if need[1] else None
            return (None, gx, out.w1t if need[2] else None, out.b1 if need[3] else None, out.w2 if need[4] else None,
                    out.b2 if need[5] else None)
        return _torch_head_backward(ctx.relu, need, gy, x, w1t, w2, hidden)
