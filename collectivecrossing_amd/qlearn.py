"""Q-learning on the device (include/ccx.h CCX_QLEARN): epsilon-greedy actions over the legal set from a network's Q-values
(``ccx_q_actions``, one launch) and the double-DQN TD error with its Huber loss, its means over the rows that count and its
gradient with respect to the Q-values (``ccx_td_loss`` / ``ccx_td_loss_backward``; with a discount per row, as an n-step minibatch brings it, ``ccx_td_loss_discounted`` and its backward).  Q-values are the ``[..., 5]`` outputs of
an :class:`~collectivecrossing_amd.learner.MlpHead` or of :class:`~collectivecrossing_amd.sides.SideHeads`; the online and the
target network are two of them (``target.load_state_dict(online.state_dict())``).

:class:`QLearning` is a class of its own, not a set of methods of the batch, for the reason ``sides.py`` gives: the
stream-order table of the batch's classes (tests/_stream_order.py) is closed, and this class brings its own proof
(tests/test_gpu_stream_order_qlearn.py)."""

from __future__ import annotations

from dataclasses import dataclass

import numpy as np
import torch

from .learner import _OPT, _require, _require_all, _require_out


@dataclass
class QActions:
    """Epsilon-greedy actions (:meth:`QLearning.q_actions`).  Every element is written: 255 / 0 for agents that are
    terminated or truncated."""

    actions: torch.Tensor           # u8 [E, N]: what step / rollout consume
    explored: torch.Tensor | None   # u8 [E, N]: 1 where the slot took the uniform choice instead of the greedy action


@dataclass
class TdLossResult:
    """The TD loss over the rows that count (:meth:`QLearning.td_loss`).  ``stats`` = {loss, mean |td|, mean Q taken, mean
    target, 0, 0, count, bad}; the named accessors are 0-dim views of it.  ``workspace`` / ``grad_q`` are the static buffers
    of :meth:`QLearning.alloc_td_loss` (else ``None``)."""

    loss: torch.Tensor                        # f32 0-dim: stats[0]; carries the autograd graph when q required grad
    stats: torch.Tensor                       # f32 [8]
    td_error: torch.Tensor | None = None      # f32 [...]: q[a] - target; +0.0 at rows that do not count
    workspace: torch.Tensor | None = None     # u8 [ccx_td_workspace_bytes(rows)]
    grad_q: torch.Tensor | None = None        # f32 [..., 5]

    mean_abs_td = property(lambda self: self.stats[1])
    mean_q = property(lambda self: self.stats[2])
    mean_target = property(lambda self: self.stats[3])
    count = property(lambda self: self.stats[6])
    bad = property(lambda self: self.stats[7])


def _check_td_hyper(gamma, huber_delta, discount=None):
    """The two hyper-parameters as the f32 values the library will see, or ``ValueError``.  ``gamma`` is 0.99 where neither
    it nor ``discount`` is given; with ``discount`` it is not read, and giving both is refused."""
    if discount is not None and gamma is not None:
        raise ValueError("give gamma or discount, not both (with discount= every row brings its own)")
    gamma = 0.99 if gamma is None or discount is not None else gamma
    try:
        gamma, huber_delta = float(np.float32(gamma)), float(np.float32(huber_delta))
    except (TypeError, ValueError):
        raise ValueError("gamma and huber_delta must be numbers") from None
    if not 0.0 <= gamma <= 1.0:                                          # (false for NaN)
        raise ValueError(f"gamma must be in [0, 1], got {gamma!r}")
    if not huber_delta > 0.0:
        raise ValueError(f"huber_delta must be > 0 (inf: the squared error), got {huber_delta!r}")
    return gamma, huber_delta


class QLearning:
    """The Q-learning links of one batch: ``QLearning(batch, epsilon=1.0)``.

    ``epsilon`` is a float property backed by a device f32 [1] (:attr:`epsilon_dev`), written on the handle's stream: an
    annealed rate changes between the replays of a captured actor loop without a re-capture.  Every method that enqueues
    keeps the stream-order contract of :class:`~collectivecrossing_amd.learner.LearnerOps` through the batch's ``_enqueue``.
    Anything else than the tensors described raises ``ValueError`` before the library is called; zero rows return without
    calling it.  Not here: a dueling combine, distributional heads, prioritised sampling (``weights`` and
    ``td_error`` are its hooks; the replay buffer itself is :class:`~collectivecrossing_amd.replay.ReplayRing`), the head's forward fused with the action choice, bf16 / f16."""

    def __init__(self, batch, epsilon: float = 1.0):
        from .batched import BatchedCollectiveCrossing

        if not isinstance(batch, BatchedCollectiveCrossing):
            raise ValueError("batch must be a BatchedCollectiveCrossing")
        self.batch = batch
        self._epsilon = self._check_epsilon(epsilon)
        self.epsilon_dev = torch.full((1,), self._epsilon, dtype=torch.float32, device=batch.device)

    @staticmethod
    def _check_epsilon(value) -> float:
        try:
            value = float(np.float32(value))
        except (TypeError, ValueError):
            raise ValueError("epsilon must be a number") from None
        if not 0.0 <= value <= 1.0:                                      # (false for NaN)
            raise ValueError(f"epsilon must be in [0, 1], got {value!r}")
        return value

    @property
    def epsilon(self) -> float:
        return self._epsilon

    @epsilon.setter
    def epsilon(self, value) -> None:
        self._epsilon = self._check_epsilon(value)
        b = self.batch
        cur = b._order_after_current_stream(self.epsilon_dev)
        with torch.cuda.stream(b._stream):
            self.epsilon_dev.fill_(self._epsilon)
        b._current_stream_waits(cur=cur)

    # ------------------------------------------------------------------ Q-values to actions
    def alloc_q_actions(self, want_explored: bool = False) -> QActions:
        """Output tensors of :meth:`q_actions` (static buffers for a captured graph)."""
        b = self.batch
        shape = (b.num_envs, b.num_agents)
        return QActions(b._new(shape, torch.uint8), b._new(shape, torch.uint8) if want_explored else None)

    def q_actions(self, q: torch.Tensor, masks: torch.Tensor | None = None, greedy: bool = False, want_explored: bool = False,
                  out: QActions | None = None) -> QActions:
        """Epsilon-greedy actions over the legal set (``ccx_q_actions``, include/ccx.h CCX_QLEARN): one kernel on the
        handle's stream, bit-defined, drawn with the library's counter-based key (global env, episode, step of the episode,
        agent slot; ``set_rng_seed``) on two streams of its own -- the same actions for any split into calls, any world
        size, eager or captured.

        ``q`` f32 [E, N, 5] (contiguous, 16-byte aligned); ``masks`` u8 [E, N] (``action_masks`` / ``masks_out``; ``None`` =
        everything legal).  With probability :attr:`epsilon` (read from the device scalar when the kernel runs) a live slot
        takes one of its legal actions uniformly, otherwise the legal action of the greatest Q-value (lowest index on ties; a
        NaN never wins).  ``greedy=True`` draws nothing and reads no rate.  Agents that are terminated or truncated get action
        255.  ``explored`` u8 [E, N] is 1 where the uniform choice was taken.  ``out`` reuses a :class:`QActions`
        (:meth:`alloc_q_actions`; its ``explored`` decides, ``want_explored`` is then ignored): ``out.actions`` may be a
        ``[E, N]`` view of the ``[1, E, N]`` tensor ``rollout`` reads.
        Only enqueues (no host synchronisation); stream order: :class:`LearnerOps`."""
        b = self.batch
        E, N = b.num_envs, b.num_agents
        _require_out(out, QActions, "alloc_q_actions")
        if out is None:
            out = self.alloc_q_actions(want_explored)
        _require_all(b.device, ("q", q, torch.float32, (E, N, 5), {"align": 16}), ("masks", masks, torch.uint8, (E, N), _OPT),
                     ("out.actions", out.actions, torch.uint8, (E, N)), ("out.explored", out.explored, torch.uint8, (E, N), _OPT))
        eps = None if greedy else self.epsilon_dev
        q = q.detach()
        b._enqueue(b._lib.ccx_q_actions, q, masks, eps, out.actions, out.explored)
        return out

    # ------------------------------------------------------------------ the TD loss over the rows that count
    def _workspace_arg(self, workspace, rows: int) -> torch.Tensor:
        b = self.batch
        return b._workspace_arg(int(b._lib.ccx_td_workspace_bytes(int(rows))), workspace, "alloc_td_loss")

    def _workspace(self, rows: int) -> torch.Tensor:
        return self._workspace_arg(None, rows)

    def alloc_td_loss(self, shape, want_td_error: bool = True) -> TdLossResult:
        """Static buffers of :meth:`td_loss` / :meth:`td_loss_backward` for rows of the leading shape ``shape``: stats, the
        workspace, ``td_error`` if asked for, and ``grad_q`` (for a captured graph)."""
        b = self.batch
        shape = tuple(int(x) for x in shape)
        rows = int(np.prod(shape)) if shape else 1
        stats = torch.zeros((8,), dtype=torch.float32, device=b.device)
        return TdLossResult(stats[0], stats, b._new(shape, torch.float32) if want_td_error else None, self._workspace(rows),
                            b._new(shape + (5,), torch.float32))

    def _check_td(self, q, actions, reward, done, q_next_target, q_next_online, masks_next, valid, weights, extra=(), discount=None):
        """The input checks :meth:`td_loss` and :meth:`td_loss_backward` share; returns the leading shape."""
        dev = self.batch.device
        lead = tuple(q.shape[:-1]) if isinstance(q, torch.Tensor) else ()
        f, u8 = torch.float32, torch.uint8
        _require_all(dev, ("q", q, f, (..., 5), {"align": 16}),
                     ("actions", actions, u8, lead, {"hint": " (cast stored actions to torch.uint8 first)"}),
                     ("reward", reward, torch.float64, lead, {"hint": " (the rollout's own f64 reward)"}),
                     ("done", done, u8, lead),
                     ("q_next_target", q_next_target, f, lead + (5,), {"align": 16}),
                     ("q_next_online", q_next_online, f, lead + (5,), {"optional": True, "align": 16}),
                     ("masks_next", masks_next, u8, lead, _OPT), ("valid", valid, u8, lead, _OPT),
                     ("weights", weights, f, lead, _OPT), ("discount", discount, f, lead, _OPT), *extra)
        if discount is not None and discount.requires_grad:
            raise ValueError("discount must not require a gradient (it is a constant of the target)")
        for name, t in (("q_next_target", q_next_target), ("q_next_online", q_next_online)):
            if t is not None and t.requires_grad:
                raise ValueError(f"{name} must not require a gradient (the target is a constant: detach it, or evaluate it "
                                 "under torch.no_grad())")
        return lead

    def _forward(self, q, actions, reward, done, qt, qo, masks_next, valid, weights, hyper, workspace, stats, td_error,
                 discount=None) -> None:
        b = self.batch
        if discount is None:
            b._enqueue(b._lib.ccx_td_loss, actions.numel(), q, actions, reward, done, qt, qo, masks_next, valid, weights, *hyper,
                       workspace, stats, td_error)
        else:
            b._enqueue(b._lib.ccx_td_loss_discounted, actions.numel(), q, actions, reward, done, qt, qo, masks_next, valid, weights,
                       discount, hyper[1], workspace, stats, td_error)

    def td_loss(self, q: torch.Tensor, actions: torch.Tensor, reward: torch.Tensor, done: torch.Tensor,
                q_next_target: torch.Tensor, q_next_online: torch.Tensor | None = None, masks_next: torch.Tensor | None = None,
                valid: torch.Tensor | None = None, weights: torch.Tensor | None = None, gamma: float | None = None,
                huber_delta: float = 1.0, want_td_error: bool = False, out: TdLossResult | None = None,
                discount: torch.Tensor | None = None) -> TdLossResult:
        """The Huber loss of the (double-)DQN TD error, averaged over the rows that count, on the device (``ccx_td_loss``,
        include/ccx.h CCX_QLEARN): two kernels on the handle's stream, bit-defined (the reduction is CCX_PPO_LOSS's fixed f64
        tree), shapes static -- ``valid`` is a selection inside the kernel.

        ``q`` f32 [..., 5] (the online network at the state; contiguous, 16-byte aligned); everything else has its leading
        shape: ``actions`` u8, ``reward`` f64 (the rollout's own), ``done`` u8 (not zero: terminated, nothing is
        bootstrapped), ``q_next_target`` f32 [..., 5] (the target network at the next state), ``q_next_online`` f32 [..., 5]
        or ``None`` (double-Q: the online network chooses the bootstrap action, the target network values it),
        ``masks_next`` u8 or ``None`` (the next state's legal set), ``valid`` u8 or ``None``, ``weights`` f32 or ``None``.
        The target is ``reward + (done ? 0 : gamma * q_next_target[argmax])``.  A row counts iff its ``valid`` byte is not
        zero and its action is 0..4; an action in 5..254 is tallied in ``stats[7]``.  ``huber_delta = inf`` is the half
        squared error.  ``td_error`` (``want_td_error``, or ``out``'s) is ``q[a] - target``, +0.0 where the row does not count.
        ``gamma`` defaults to 0.99.  ``discount`` f32 of the leading shape (``NStepBatch.discount``) gives every row its own
        in the place of ``gamma`` (``ccx_td_loss_discounted``: the same rule, tree and outputs; an array filled with one
        value gives the bits of that ``gamma``); ``gamma`` is then not read, giving both raises ``ValueError``, and so does a
        ``discount`` that requires grad.

        When ``q.requires_grad`` and grad mode is on, the call is a ``torch.autograd.Function``: ``r.loss.backward()``
        reaches ``q`` through ``ccx_td_loss_backward`` (one kernel; rows that do not count get exactly +0.0), ``out=`` is
        refused, and the workspace comes from torch's allocator, so the call captures.  The next-state arrays are never
        differentiated: one that requires grad raises ``ValueError``.  Otherwise ``out=`` reuses a result of
        :meth:`alloc_td_loss`.
        Only enqueues (no host synchronisation); stream order: :class:`LearnerOps`."""
        b = self.batch
        hyper = _check_td_hyper(gamma, huber_delta, discount)
        lead = self._check_td(q, actions, reward, done, q_next_target, q_next_online, masks_next, valid, weights, discount=discount)
        if q.requires_grad and torch.is_grad_enabled():
            if out is not None:
                raise ValueError("out= cannot be used when q requires a gradient (the autograd path allocates its outputs)")
            if q.numel() == 0:
                stats = torch.cat([q.sum().reshape(1) * 0.0, torch.zeros(7, device=b.device)])
                return TdLossResult(stats[0], stats.detach(), q.new_zeros(lead) if want_td_error else None)
            td_error = b._new(lead, torch.float32) if want_td_error else None
            stats = _TdLoss.apply(self, q, actions, reward, done, q_next_target, q_next_online, masks_next, valid, weights, hyper,
                                  td_error, discount)
            return TdLossResult(stats[0], stats.detach(), td_error)
        _require_out(out, TdLossResult, "alloc_td_loss")
        if out is None:
            stats = torch.zeros((8,), dtype=torch.float32, device=b.device)
            out = TdLossResult(stats[0], stats, b._new(lead, torch.float32) if want_td_error else None)
            workspace = None
        else:
            _require_all(b.device, ("out.stats", out.stats, torch.float32, (8,)),
                         ("out.td_error", out.td_error, torch.float32, lead, _OPT))
            workspace = out.workspace
        if q.numel() == 0:
            out.stats.zero_()
            return out
        workspace = self._workspace_arg(workspace, actions.numel())
        self._forward(q.detach(), actions, reward, done, q_next_target, q_next_online, masks_next, valid, weights, hyper,
                      workspace, out.stats, out.td_error, discount)
        return out

    def td_loss_backward(self, q: torch.Tensor, actions: torch.Tensor, reward: torch.Tensor, done: torch.Tensor,
                         q_next_target: torch.Tensor, q_next_online: torch.Tensor | None = None,
                         masks_next: torch.Tensor | None = None, valid: torch.Tensor | None = None,
                         weights: torch.Tensor | None = None, gamma: float | None = None, huber_delta: float = 1.0, *,
                         stats: torch.Tensor, grad_loss: torch.Tensor | None = None, out=None,
                         discount: torch.Tensor | None = None) -> torch.Tensor:
        """``grad_q`` f32 [..., 5] of :meth:`td_loss`'s ``loss`` (``ccx_td_loss_backward``: one kernel that recomputes the
        forward terms from the same inputs and the forward's ``stats``).  Every element is written: the gradient sits at the
        taken action of a row that counts, +0.0 everywhere else.  ``grad_loss`` f32 [1] or 0-dim on the device (``None`` =
        1).  ``out`` reuses a f32 tensor of the shape of ``q`` (16-byte aligned) or the ``grad_q`` of an
        :meth:`alloc_td_loss` result.  ``discount`` as in :meth:`td_loss` (``ccx_td_loss_discounted_backward``).
        Only enqueues (no host synchronisation); stream order: :class:`LearnerOps`."""
        b = self.batch
        hyper = _check_td_hyper(gamma, huber_delta, discount)
        if isinstance(out, TdLossResult):
            out = out.grad_q
        if out is None and isinstance(q, torch.Tensor):
            out = torch.empty_like(q, requires_grad=False)
        lead = tuple(q.shape[:-1]) if isinstance(q, torch.Tensor) else ()
        self._check_td(q, actions, reward, done, q_next_target, q_next_online, masks_next, valid, weights, (
            ("stats", stats, torch.float32, (8,)), ("out", out, torch.float32, lead + (5,), {"align": 16})), discount=discount)
        if grad_loss is not None:                                        # (inline: one element in either of two shapes)
            if (not isinstance(grad_loss, torch.Tensor) or grad_loss.dtype is not torch.float32 or grad_loss.device != b.device
                    or grad_loss.numel() < 1 or grad_loss.dim() > 1 or not grad_loss.is_contiguous()):
                raise ValueError(f"grad_loss must be a torch.float32 tensor with one element (0-dim or [1]) on {b.device}")
        if q.numel():
            q = q.detach()
            if discount is None:
                b._enqueue(b._lib.ccx_td_loss_backward, actions.numel(), q, actions, reward, done, q_next_target, q_next_online,
                           masks_next, valid, weights, *hyper, stats, grad_loss, out)
            else:
                b._enqueue(b._lib.ccx_td_loss_discounted_backward, actions.numel(), q, actions, reward, done, q_next_target,
                           q_next_online, masks_next, valid, weights, discount, hyper[1], stats, grad_loss, out)
        return out


class _TdLoss(torch.autograd.Function):
    """:meth:`QLearning.td_loss` for Q-values that require a gradient: the forward is the two kernels of ``ccx_td_loss``, the
    backward the one of ``ccx_td_loss_backward``; nothing is saved but the inputs and ``stats``.  Only ``stats[0]``, the
    loss, is differentiable: the gradient arriving at the other seven is not read."""

    @staticmethod
    def forward(ctx, ql, q, actions, reward, done, qt, qo, masks_next, valid, weights, hyper, td_error, discount=None):
        q = q.detach()
        stats = torch.zeros((8,), dtype=torch.float32, device=ql.batch.device)
        ql._forward(q, actions, reward, done, qt, qo, masks_next, valid, weights, hyper, ql._workspace(actions.numel()), stats,
                    td_error, discount)
        ctx.ql, ctx.hyper, ctx.discount = ql, hyper, discount
        ctx.rest = (actions, reward, done, qt, qo, masks_next, valid, weights)
        ctx.save_for_backward(q, stats)
        return stats

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_stats):
        q, stats = ctx.saved_tensors
        gamma = None if ctx.discount is not None else ctx.hyper[0]
        gq = ctx.ql.td_loss_backward(q, *ctx.rest, gamma, ctx.hyper[1], stats=stats, grad_loss=grad_stats.contiguous(),
                                     discount=ctx.discount)
        return (None, gq) + (None,) * 11
