"""Q-learning on the device (include/ccx.h CCX_QLEARN): epsilon-greedy actions over the legal set from a network's Q-values
(``ccx_q_actions``, one launch) and the double-DQN TD error with its Huber loss, its means over the rows that count and its
gradient with respect to the Q-values (``ccx_td_loss`` / ``ccx_td_loss_backward``; with a discount per row, as an n-step minibatch brings it, ``ccx_td_loss_discounted`` and its backward).  Q-values are the ``[..., 5]`` outputs of
an :class:`~collectivecrossing_amd.learner.MlpHead` or of :class:`~collectivecrossing_amd.sides.SideHeads`; the online and the
target network are two of them (``target.load_state_dict(online.state_dict())``).  A head with six outputs is a dueling head
(CCX_DUELING): its rows go through ``dueling`` to Q-values, and ``mlp_q_actions`` / ``sides_q_actions`` take observation rows
to actions in one launch for either kind.

:class:`QLearning` is a class of its own, not a set of methods of the batch, for the reason ``sides.py`` gives: the
stream-order table of the batch's classes (tests/_stream_order.py) is closed, and this class brings its own proof
(tests/test_gpu_stream_order_qlearn.py)."""

from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from typing import ClassVar

import numpy as np
import torch

from ._abi import DUELING_MAX_ARRAYS
from .learner import (MlpHead, _OPT, _alloc_loss, _check_grad_loss, _loss_over_rows, _loss_workspace, _new_stats, _require,
                      _require_all, _require_out)
from .sides import SideHeads


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
    _frame: ClassVar = ("ccx_td_workspace_bytes", "alloc_td_loss", "q requires")      # (learner._loss_over_rows)

    mean_abs_td = property(lambda self: self.stats[1])
    mean_q = property(lambda self: self.stats[2])
    mean_target = property(lambda self: self.stats[3])
    count = property(lambda self: self.stats[6])
    bad = property(lambda self: self.stats[7])


def _check_gamma(gamma, not_a_number: str = "gamma must be a number") -> float:
    """``gamma`` as the f32 value the library will see, or ``ValueError``: a number in [0, 1]."""
    try:
        gamma = float(np.float32(gamma))
    except (TypeError, ValueError):
        raise ValueError(not_a_number) from None
    if not 0.0 <= gamma <= 1.0:                                          # (false for NaN)
        raise ValueError(f"gamma must be in [0, 1], got {gamma!r}")
    return gamma


def _check_td_hyper(gamma, huber_delta, discount=None):
    """The two hyper-parameters as the f32 values the library will see, or ``ValueError``.  ``gamma`` is 0.99 where neither
    it nor ``discount`` is given; with ``discount`` it is not read, and giving both is refused."""
    if discount is not None and gamma is not None:
        raise ValueError("give gamma or discount, not both (with discount= every row brings its own)")
    gamma = 0.99 if gamma is None or discount is not None else gamma
    numbers = "gamma and huber_delta must be numbers"
    try:
        huber_delta = float(np.float32(huber_delta))
    except (TypeError, ValueError):
        raise ValueError(numbers) from None
    gamma = _check_gamma(gamma, numbers)
    if not huber_delta > 0.0:
        raise ValueError(f"huber_delta must be > 0 (inf: the squared error), got {huber_delta!r}")
    return gamma, huber_delta


class QLearning:
    """The Q-learning links of one batch: ``QLearning(batch, epsilon=1.0)``.

    ``epsilon`` is a float property backed by a device f32 [1] (:attr:`epsilon_dev`), written on the handle's stream: an
    annealed rate changes between the replays of a captured actor loop without a re-capture.  Every method that enqueues
    keeps the stream-order contract of :class:`~collectivecrossing_amd.learner.LearnerOps` through the batch's ``_enqueue``.
    Anything else than the tensors described raises ``ValueError`` before the library is called; zero rows return without
    calling it.  The dueling combine (:meth:`dueling`, :meth:`dueling_into`, :meth:`dueling_backward`) and the head's forward
    fused with the action choice (:meth:`mlp_q_actions`, :meth:`sides_q_actions`) are include/ccx.h CCX_DUELING.
    Distributional (categorical, C51) heads are :class:`~collectivecrossing_amd.categorical.CategoricalQ` (CCX_C51).  Not here:
    prioritised sampling (``weights`` and ``td_error`` are its hooks; the replay buffer itself is
    :class:`~collectivecrossing_amd.replay.ReplayRing`), on-policy minibatches (shuffled without replacement by
    :class:`~collectivecrossing_amd.minibatch.RolloutMinibatches`), bf16 / f16."""

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

    # ------------------------------------------------------------------ observation rows to actions (CCX_DUELING)
    def _check_fused(self, who, net, obs, masks, q_out, want_explored, out):
        """The checks :meth:`mlp_q_actions` and :meth:`sides_q_actions` share, behind the test of ``net`` itself; returns
        ``out``."""
        b = self.batch
        E, N = b.num_envs, b.num_agents
        if net.O not in (5, 6) or net.L != b.obs_len:
            raise ValueError(f"{who} needs O == 5 (plain) or O == 6 (dueling) and L == obs_len == {b.obs_len}, got O = {net.O}, "
                             f"L = {net.L}")
        _require_out(out, QActions, "alloc_q_actions")
        if out is None:
            out = self.alloc_q_actions(want_explored)
        _require_all(b.device, ("obs", obs, torch.float32, (E, N, b.obs_len), {"align": 16}), ("masks", masks, torch.uint8, (E, N), _OPT),
                     ("q_out", q_out, torch.float32, (E, N, 5), _OPT), ("out.actions", out.actions, torch.uint8, (E, N)),
                     ("out.explored", out.explored, torch.uint8, (E, N), _OPT))
        return out

    def mlp_q_actions(self, head, obs: torch.Tensor, masks: torch.Tensor | None = None, greedy: bool = False,
                      want_explored: bool = False, q_out: torch.Tensor | None = None, out: QActions | None = None) -> QActions:
        """Observation rows to epsilon-greedy actions in ONE launch (``ccx_mlp_q_actions``, include/ccx.h CCX_DUELING): by
        definition ``q_actions(head(obs), ...)`` for a head with ``O == 5`` and ``q_actions(dueling(head(obs)), ...)`` for
        one with ``O == 6`` -- the same key, the same rule for terminated or truncated agents, the same bits in ``actions``
        and ``explored`` -- without the Q-values' round trip through memory and without the further launches.  ``head`` is
        an :class:`~collectivecrossing_amd.learner.MlpHead` of this batch with ``L == obs_len``; ``obs`` f32 [E, N, L]
        (contiguous, 16-byte aligned: the ``obs`` of ``step`` / ``rollout``); ``q_out`` f32 [E, N, 5] receives the COMBINED
        Q-values of every slot, dead ones included.  ``masks``, ``greedy``, ``want_explored`` and ``out`` are
        :meth:`q_actions`'.  No gradient flows through this call.
        Only enqueues (no host synchronisation); stream order: :class:`LearnerOps`."""
        b = self.batch
        if not isinstance(head, MlpHead) or head.batch is not b:
            raise ValueError("head must be an MlpHead of this batch (mlp_head)")
        out = self._check_fused("mlp_q_actions", head, obs, masks, q_out, want_explored, out)
        head._check_parameters()
        if obs.numel() == 0:
            return out
        b._enqueue(b._lib.ccx_mlp_q_actions, head.H, head.activation_id, head.O, obs, head.w1t, head.b1, head.w2, head.b2, masks,
                   None if greedy else self.epsilon_dev, out.actions, out.explored, q_out)
        return out

    def sides_q_actions(self, sides, obs: torch.Tensor, masks: torch.Tensor | None = None, greedy: bool = False,
                        want_explored: bool = False, q_out: torch.Tensor | None = None, out: QActions | None = None) -> QActions:
        """:meth:`mlp_q_actions` for :class:`~collectivecrossing_amd.sides.SideHeads` of this batch
        (``ccx_sides_q_actions``): every group's slots get what :meth:`mlp_q_actions` gives with that group's head, in ONE
        launch.  A slot that no head owns gets action 255 and ``explored`` 0 (what ``step_mixed`` expects for the slots it
        scripts); its ``q_out`` elements are not written and it runs no layer.
        Only enqueues (no host synchronisation); stream order: :class:`LearnerOps`."""
        b = self.batch
        if not isinstance(sides, SideHeads) or sides.batch is not b:
            raise ValueError("sides must be SideHeads of this batch")
        out = self._check_fused("sides_q_actions", sides, obs, masks, q_out, want_explored, out)
        table = sides._table()
        if obs.numel() == 0:
            return out
        b._enqueue(b._lib.ccx_sides_q_actions, sides.H, sides.dims[3], sides.O, obs, len(table), table, masks,
                   None if greedy else self.epsilon_dev, out.actions, out.explored, q_out, also=sides._param_tensors())
        return out

    # ------------------------------------------------------------------ the dueling combine (CCX_DUELING)
    def dueling_into(self, va, q) -> tuple:
        """``q[i] = dueling(va[i])`` for 1..4 pairs of equal leading shape in ONE launch (``ccx_dueling_forward``): ``va``
        a tuple of f32 [..., 6], ``q`` a tuple of f32 [..., 5] of the same length (a single pair may be given as two
        tensors), all contiguous and 16-byte aligned -- the static buffers of a captured update, which combines ``q``,
        ``q_next_target`` and ``q_next_online`` in one node.  No gradient flows through this call (:meth:`dueling` is the
        differentiable form).  Returns ``q`` as a tuple.
        Only enqueues (no host synchronisation); stream order: :class:`LearnerOps`."""
        b = self.batch
        vas = (va,) if isinstance(va, torch.Tensor) else tuple(va) if isinstance(va, (tuple, list)) else ()
        qs = (q,) if isinstance(q, torch.Tensor) else tuple(q) if isinstance(q, (tuple, list)) else ()
        if not 1 <= len(vas) <= DUELING_MAX_ARRAYS or len(qs) != len(vas):
            raise ValueError(f"va and q must be tuples of the same length, 1 .. {DUELING_MAX_ARRAYS} tensors each")
        lead = tuple(vas[0].shape[:-1]) if isinstance(vas[0], torch.Tensor) else ()
        _require_all(b.device, *((f"va[{i}]", t, torch.float32, lead + (6,), {"align": 16}) for i, t in enumerate(vas)),
                     *((f"q[{i}]", t, torch.float32, lead + (5,), {"align": 16}) for i, t in enumerate(qs)))
        if vas[0].numel() == 0:
            return qs
        vas = tuple(t.detach() for t in vas)
        table_va = (C.c_void_p * len(vas))(*(t.data_ptr() for t in vas))
        table_q = (C.c_void_p * len(qs))(*(t.data_ptr() for t in qs))
        b._enqueue(b._lib.ccx_dueling_forward, vas[0].numel() // 6, len(vas), table_va, table_q, also=vas + qs)
        return qs

    def dueling(self, va: torch.Tensor, out: torch.Tensor | None = None) -> torch.Tensor:
        """The dueling combine (``ccx_dueling_forward``, include/ccx.h CCX_DUELING; one kernel, bit-defined): ``va`` f32
        [..., 6] -- five advantages and the state value, the output of a head with ``O == 6`` -- to Q-values f32 [..., 5],
        ``q_k = v + (a_k - mean(a))`` with the mean over all five actions whatever a mask says.  Both contiguous and 16-byte
        aligned.  When ``va.requires_grad`` and grad mode is on, the call is a ``torch.autograd.Function`` whose backward is
        :meth:`dueling_backward`, and ``out=`` is refused.
        Only enqueues (no host synchronisation); stream order: :class:`LearnerOps`."""
        b = self.batch
        _require("va", va, torch.float32, (..., 6), b.device, align=16)
        if va.requires_grad and torch.is_grad_enabled():
            if out is not None:
                raise ValueError("out= cannot be used when va requires a gradient (the autograd path allocates its output)")
            if va.numel() == 0:
                return va[..., :5] * 0.0
            return _Dueling.apply(self, va)
        if out is None:
            out = b._new(tuple(va.shape[:-1]) + (5,), torch.float32)
        return self.dueling_into((va,), (out,))[0]

    def dueling_backward(self, grad_q: torch.Tensor, out: torch.Tensor | None = None) -> torch.Tensor:
        """``grad_va`` f32 [..., 6] from ``grad_q`` f32 [..., 5] (``ccx_dueling_backward``; one kernel): a pure function of
        ``grad_q``.  Every element is written; a row of five +0.0 gets six +0.0, so what :meth:`td_loss_backward` leaves at
        rows that do not count stays exactly +0.0 down to ``backward_into``.  Both contiguous and 16-byte aligned; ``out``
        reuses a tensor.
        Only enqueues (no host synchronisation); stream order: :class:`LearnerOps`."""
        b = self.batch
        lead = tuple(grad_q.shape[:-1]) if isinstance(grad_q, torch.Tensor) else ()
        if out is None and isinstance(grad_q, torch.Tensor):
            out = b._new(lead + (6,), torch.float32)
        _require_all(b.device, ("grad_q", grad_q, torch.float32, (..., 5), {"align": 16}),
                     ("out", out, torch.float32, lead + (6,), {"align": 16}))
        if grad_q.numel():
            b._enqueue(b._lib.ccx_dueling_backward, grad_q.numel() // 5, grad_q.detach(), out)
        return out

    # ------------------------------------------------------------------ the TD loss over the rows that count
    def alloc_td_loss(self, shape, want_td_error: bool = True) -> TdLossResult:
        """Static buffers of :meth:`td_loss` / :meth:`td_loss_backward` for rows of the leading shape ``shape``: stats, the
        workspace, ``td_error`` if asked for, and ``grad_q`` (for a captured graph)."""
        b = self.batch
        shape, stats, workspace = _alloc_loss(b, TdLossResult, shape)
        return TdLossResult(stats[0], stats, b._new(shape, torch.float32) if want_td_error else None, workspace,
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

    def _forward(self, q, actions, reward, done, qt, qo, masks_next, valid, weights, hyper, discount, workspace, stats,
                 td_error) -> None:
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
        return _loss_over_rows(b, TdLossResult, self, _TdLoss, self._forward, (q,),
                               (actions, reward, done, q_next_target, q_next_online, masks_next, valid, weights, hyper, discount),
                               actions.numel(), (("td_error", lead, want_td_error, _OPT),), out)

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
        _check_grad_loss(grad_loss, b.device)
        if q.numel():
            q = q.detach()
            if discount is None:
                b._enqueue(b._lib.ccx_td_loss_backward, actions.numel(), q, actions, reward, done, q_next_target, q_next_online,
                           masks_next, valid, weights, *hyper, stats, grad_loss, out)
            else:
                b._enqueue(b._lib.ccx_td_loss_discounted_backward, actions.numel(), q, actions, reward, done, q_next_target,
                           q_next_online, masks_next, valid, weights, discount, hyper[1], stats, grad_loss, out)
        return out


class _Dueling(torch.autograd.Function):
    """:meth:`QLearning.dueling` for rows that require a gradient: the forward is ``ccx_dueling_forward``, the backward
    ``ccx_dueling_backward``; nothing is saved (the backward is a pure function of the gradient)."""

    @staticmethod
    def forward(ctx, ql, va):
        ctx.ql = ql
        q = ql.batch._new(tuple(va.shape[:-1]) + (5,), torch.float32)
        return ql.dueling_into((va,), (q,))[0]

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_q):
        return None, ctx.ql.dueling_backward(grad_q.contiguous())


class _TdLoss(torch.autograd.Function):
    """:meth:`QLearning.td_loss` for Q-values that require a gradient: the forward is the two kernels of ``ccx_td_loss``, the
    backward the one of ``ccx_td_loss_backward``; nothing is saved but the inputs and ``stats``.  Only ``stats[0]``, the
    loss, is differentiable: the gradient arriving at the other seven is not read."""

    @staticmethod
    def forward(ctx, ql, q, actions, reward, done, qt, qo, masks_next, valid, weights, hyper, discount, td_error):
        q = q.detach()
        stats = _new_stats(ql.batch.device)
        ql._forward(q, actions, reward, done, qt, qo, masks_next, valid, weights, hyper, discount,
                    _loss_workspace(ql.batch, TdLossResult, None, actions.numel()), stats, td_error)
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
