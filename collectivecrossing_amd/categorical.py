"""Categorical (C51) Q-heads on the device (include/ccx.h CCX_C51): the expected values of a network's atom logits
(``ccx_c51_q_values``, one launch; what :meth:`QLearning.q_actions` chooses from), the projection of the bootstrapped target
distribution onto the support with the cross-entropy loss and its means over the rows that count (``ccx_c51_loss``, two
launches), and the gradient with respect to the logits (``ccx_c51_loss_backward``, one launch).  The projection is a gather
with a written order of additions, not the two ``index_add_`` of the textbook, so every output is the same bit for bit from
run to run.  Logits are the ``[..., 5, A]`` outputs of a torch network (index = action id, then atom); the online and the
target network are two of them.

:class:`CategoricalQ` is a class of its own, not a set of methods of the batch, for the reason ``qlearn.py`` gives: the
stream-order table of the batch's classes (tests/_stream_order.py) is closed, and this class brings its own proof
(tests/test_gpu_stream_order_c51.py)."""

from __future__ import annotations

from dataclasses import dataclass
from typing import ClassVar

import numpy as np
import torch

from .learner import _OPT, _alloc_loss, _check_grad_loss, _loss_over_rows, _loss_workspace, _new_stats, _require_all
from .qlearn import _check_td_hyper

MIN_ATOMS, MAX_ATOMS = 2, 64


@dataclass
class CategoricalLossResult:
    """The categorical loss over the rows that count (:meth:`CategoricalQ.loss`).  ``stats`` = {loss, mean cross-entropy,
    mean Q taken, mean target, 0, 0, count, bad}; the named accessors are 0-dim views of it.  ``workspace`` / ``grad_logits``
    are the static buffers of :meth:`CategoricalQ.alloc_loss` (else ``None``)."""

    loss: torch.Tensor                        # f32 0-dim: stats[0]; carries the autograd graph when logits required grad
    stats: torch.Tensor                       # f32 [8]
    row_loss: torch.Tensor | None = None      # f32 [...]: the row's cross-entropy, unweighted, >= 0; +0.0 at rows that do not count
    proj: torch.Tensor | None = None          # f32 [..., A]: the projected target distribution; +0.0 at rows that do not count
    workspace: torch.Tensor | None = None     # u8 [ccx_c51_workspace_bytes(rows)]
    grad_logits: torch.Tensor | None = None   # f32 [..., 5, A]
    _frame: ClassVar = ("ccx_c51_workspace_bytes", "alloc_loss", "logits requires")   # (learner._loss_over_rows)

    mean_ce = property(lambda self: self.stats[1])
    mean_q = property(lambda self: self.stats[2])
    mean_target = property(lambda self: self.stats[3])
    count = property(lambda self: self.stats[6])
    bad = property(lambda self: self.stats[7])


class CategoricalQ:
    """The categorical links of one batch: ``CategoricalQ(batch, atoms=51, vmin=-10.0, vmax=10.0)``.

    ``atoms`` in 2..64; ``vmin < vmax`` finite (as f32).  :attr:`support` is the f32 [A] device tensor of the atoms,
    ``z_j = vmin + (float)j * ((vmax - vmin) / (float)(A - 1))`` as the kernels compute them.  Every method that enqueues
    keeps the stream-order contract of :class:`~collectivecrossing_amd.learner.LearnerOps` through the batch's ``_enqueue``.
    Anything else than the tensors described raises ``ValueError`` before the library is called; zero rows return without
    calling it.  Nothing is drawn here: actions are :meth:`QLearning.q_actions` on :meth:`q_values`.  A device network with
    5 A outputs is :meth:`head`.  Not here: the obs -> action fusion for categorical heads, quantile (QR-DQN / IQN) heads, noisy layers,
    dueling combined with categorical heads, more than 64 atoms, bf16 / f16, the vector and RLlib adapters."""

    def __init__(self, batch, atoms: int = 51, vmin: float = -10.0, vmax: float = 10.0):
        from .batched import BatchedCollectiveCrossing

        if not isinstance(batch, BatchedCollectiveCrossing):
            raise ValueError("batch must be a BatchedCollectiveCrossing")
        if isinstance(atoms, bool) or not isinstance(atoms, (int, np.integer)) or not MIN_ATOMS <= int(atoms) <= MAX_ATOMS:
            raise ValueError(f"atoms must be an integer in {MIN_ATOMS} .. {MAX_ATOMS}, got {atoms!r}")
        try:
            lo, hi = np.float32(vmin), np.float32(vmax)
        except (TypeError, ValueError):
            raise ValueError("vmin and vmax must be numbers") from None
        with np.errstate(all="ignore"):
            dz = np.float32(np.float32(hi - lo) / np.float32(int(atoms) - 1))
        if not (np.isfinite(lo) and np.isfinite(hi) and lo < hi and np.isfinite(dz) and dz > 0):
            raise ValueError(f"vmin < vmax must both be finite as f32, with a finite atom spacing above zero, got {vmin!r} and {vmax!r}")
        self.batch = batch
        self.atoms, self.vmin, self.vmax = int(atoms), float(lo), float(hi)
        z = (lo + (np.arange(self.atoms, dtype=np.float32) * dz).astype(np.float32)).astype(np.float32)
        self.support = torch.from_numpy(z).to(batch.device)

    # ------------------------------------------------------------------ a network for the logits
    def head(self, H: int, activation: str = "tanh", L: int | None = None, backward: str = "torch"):
        """A :class:`~collectivecrossing_amd.wide.WideMlpHead` with ``O = 5 * atoms`` outputs shaped ``(5, atoms)``: ``head(x)``
        on f32 [..., L] is the [..., 5, A] logits that :meth:`q_values` and :meth:`loss` take, bit-defined (include/ccx.h
        CCX_MLP_WIDE).  The arguments are :class:`WideMlpHead`'s.  Makes no library call."""
        from .wide import WideMlpHead

        return WideMlpHead(self.batch, H, 5 * self.atoms, activation, L, backward, out_shape=(5, self.atoms))

    # ------------------------------------------------------------------ expected values
    def q_values(self, logits: torch.Tensor, out: torch.Tensor | None = None) -> torch.Tensor:
        """Expected values f32 [..., 5] of atom logits f32 [..., 5, A] (``ccx_c51_q_values``, include/ccx.h CCX_C51; one
        kernel, bit-defined): per (row, action) the softmax over the atoms against :attr:`support`.  For a batch, logits of
        shape ``[E, N, 5, A]`` give what :meth:`QLearning.q_actions` takes, unchanged.  ``logits`` is contiguous (4-byte
        alignment is all it needs); ``out`` reuses a contiguous f32 tensor of the leading shape + (5,), 16-byte aligned.  No
        gradient flows through this call.
        Only enqueues (no host synchronisation); stream order: :class:`LearnerOps`."""
        b = self.batch
        lead = tuple(logits.shape[:-2]) if isinstance(logits, torch.Tensor) and logits.dim() >= 2 else ()
        if out is None and isinstance(logits, torch.Tensor):
            out = b._new(lead + (5,), torch.float32)
        _require_all(b.device, ("logits", logits, torch.float32, (..., 5, self.atoms), {"align": 4}),
                     ("out", out, torch.float32, lead + (5,), {"align": 16}))
        if logits.numel():
            b._enqueue(b._lib.ccx_c51_q_values, out.numel() // 5, self.atoms, self.vmin, self.vmax, logits.detach(), out)
        return out

    # ------------------------------------------------------------------ the loss over the rows that count
    def _workspace_arg(self, workspace, rows: int) -> torch.Tensor:
        return _loss_workspace(self.batch, CategoricalLossResult, workspace, rows)

    def alloc_loss(self, shape, want_row_loss: bool = True) -> CategoricalLossResult:
        """Static buffers of :meth:`loss` / :meth:`loss_backward` for rows of the leading shape ``shape``: stats, the
        workspace, ``row_loss`` if asked for, ``proj`` and ``grad_logits`` (for a captured graph)."""
        b = self.batch
        shape, stats, workspace = _alloc_loss(b, CategoricalLossResult, shape)
        f = torch.float32
        return CategoricalLossResult(stats[0], stats, b._new(shape, f) if want_row_loss else None, b._new(shape + (self.atoms,), f),
                                     workspace, b._new(shape + (5, self.atoms), f))

    def _check_loss(self, logits, actions, reward, done, next_target, next_online, masks_next, valid, weights, discount, extra=()):
        """The input checks of :meth:`loss`; returns the leading shape."""
        dev = self.batch.device
        lead = tuple(logits.shape[:-2]) if isinstance(logits, torch.Tensor) and logits.dim() >= 2 else ()
        f, u8, A = torch.float32, torch.uint8, self.atoms
        _require_all(dev, ("logits", logits, f, (..., 5, A), {"align": 4}),
                     ("actions", actions, u8, lead, {"hint": " (cast stored actions to torch.uint8 first)"}),
                     ("reward", reward, torch.float64, lead, {"hint": " (the rollout's own f64 reward)", "align": 8}),
                     ("done", done, u8, lead),
                     ("next_target", next_target, f, lead + (5, A), {"align": 4}),
                     ("next_online", next_online, f, lead + (5, A), {"optional": True, "align": 4}),
                     ("masks_next", masks_next, u8, lead, _OPT), ("valid", valid, u8, lead, _OPT),
                     ("weights", weights, f, lead, {"optional": True, "align": 4}),
                     ("discount", discount, f, lead, {"optional": True, "align": 4}), *extra)
        for name, t in (("next_target", next_target), ("next_online", next_online), ("discount", discount)):
            if t is not None and t.requires_grad:
                raise ValueError(f"{name} must not require a gradient (the target is a constant: detach it, or evaluate it "
                                 "under torch.no_grad())")
        return lead

    def _forward(self, logits, actions, reward, done, nt, no, masks_next, valid, weights, discount, gamma, workspace, stats, row_loss,
                 proj) -> None:
        b = self.batch
        b._enqueue(b._lib.ccx_c51_loss, actions.numel(), self.atoms, self.vmin, self.vmax, logits, actions, reward, done, nt, no,
                   masks_next, valid, weights, discount, gamma, workspace, stats, row_loss, proj)

    def loss(self, logits: torch.Tensor, actions: torch.Tensor, reward: torch.Tensor, done: torch.Tensor, next_target: torch.Tensor,
             next_online: torch.Tensor | None = None, masks_next: torch.Tensor | None = None, valid: torch.Tensor | None = None,
             weights: torch.Tensor | None = None, gamma: float | None = None, discount: torch.Tensor | None = None,
             want_row_loss: bool = False, out: CategoricalLossResult | None = None) -> CategoricalLossResult:
        """The cross-entropy between the projected target distribution and the online distribution at the stored action,
        averaged over the rows that count, on the device (``ccx_c51_loss``, include/ccx.h CCX_C51): two kernels on the
        handle's stream, bit-defined (the projection is a gather in ascending order, the reduction CCX_PPO_LOSS's fixed f64
        tree), shapes static -- ``valid`` is a selection inside the kernel.

        ``logits`` f32 [..., 5, A] (the online network at the state; contiguous); everything else has its leading shape:
        ``actions`` u8, ``reward`` f64 (the rollout's own), ``done`` u8 (not zero: terminated, nothing is bootstrapped),
        ``next_target`` f32 [..., 5, A] (the target network at the next state), ``next_online`` f32 [..., 5, A] or ``None``
        (double-Q: the online network's expected values choose the bootstrap action, the target network's distribution is
        projected), ``masks_next`` u8 or ``None`` (the next state's legal set), ``valid`` u8 or ``None``, ``weights`` f32 or
        ``None`` (importance weights of a prioritised replay).  The target of a row is the distribution of ``reward + (done ?
        0 : gamma * z)`` under the chosen next-state distribution, projected onto the support.  A row counts iff its
        ``valid`` byte is not zero and its action is 0..4; an action in 5..254 is tallied in ``stats[7]``.  ``gamma``
        defaults to 0.99; ``discount`` f32 of the leading shape (``NStepBatch.discount``) gives every row its own in the
        place of ``gamma``; giving both raises ``ValueError``.  ``row_loss`` (``want_row_loss``, or ``out``'s) is the row's
        unweighted cross-entropy, >= 0 and +0.0 where the row does not count: what
        ``PrioritizedReplay.update_priorities`` takes as ``td_error``.  ``proj`` f32 [..., A] is the projected target (the
        one thing the backward needs beside the inputs).  Every logit, reward and discount that a counting row reads must
        be finite: one that is not reaches ``row_loss`` and the loss as a NaN or an infinity.

        When ``logits.requires_grad`` and grad mode is on, the call is a ``torch.autograd.Function``: ``r.loss.backward()``
        reaches ``logits`` through ``ccx_c51_loss_backward`` (one kernel; rows that do not count and the four other actions
        of a row get exactly +0.0), ``out=`` is refused, and the workspace comes from torch's allocator, so the call
        captures.  The next-state arrays are never differentiated: one that requires grad raises ``ValueError``.  Otherwise
        ``out=`` reuses a result of :meth:`alloc_loss`.
        Only enqueues (no host synchronisation); stream order: :class:`LearnerOps`."""
        b = self.batch
        gamma = _check_td_hyper(gamma, 1.0, discount)[0]
        lead = self._check_loss(logits, actions, reward, done, next_target, next_online, masks_next, valid, weights, discount)
        extras = (("row_loss", lead, want_row_loss, {"optional": True, "align": 4}), ("proj", lead + (self.atoms,), True, {"align": 4}))
        return _loss_over_rows(b, CategoricalLossResult, self, _CategoricalLoss, self._forward, (logits,),
                               (actions, reward, done, next_target, next_online, masks_next, valid, weights, discount, gamma),
                               actions.numel(), extras, out)

    def loss_backward(self, logits: torch.Tensor, actions: torch.Tensor, proj: torch.Tensor, valid: torch.Tensor | None = None,
                      weights: torch.Tensor | None = None, *, stats: torch.Tensor, grad_loss: torch.Tensor | None = None,
                      out=None) -> torch.Tensor:
        """``grad_logits`` f32 [..., 5, A] of :meth:`loss`'s ``loss`` (``ccx_c51_loss_backward``: one kernel, a pure
        function of ``logits``, ``actions``, the forward's ``proj`` and ``stats``, ``valid``, ``weights`` and
        ``grad_loss``).  Every element is written: the gradient sits at the stored action of a row that counts, +0.0
        everywhere else.  ``grad_loss`` f32 [1] or 0-dim on the device (``None`` = 1).  ``out`` reuses a f32 tensor of the
        shape of ``logits`` or the ``grad_logits`` of an :meth:`alloc_loss` result.
        Only enqueues (no host synchronisation); stream order: :class:`LearnerOps`."""
        b = self.batch
        if isinstance(out, CategoricalLossResult):
            out = out.grad_logits
        if out is None and isinstance(logits, torch.Tensor):
            out = torch.empty_like(logits, requires_grad=False)
        lead = tuple(logits.shape[:-2]) if isinstance(logits, torch.Tensor) and logits.dim() >= 2 else ()
        f, u8, A = torch.float32, torch.uint8, self.atoms
        _require_all(b.device, ("logits", logits, f, (..., 5, A), {"align": 4}),
                     ("actions", actions, u8, lead, {"hint": " (cast stored actions to torch.uint8 first)"}),
                     ("proj", proj, f, lead + (A,), {"align": 4}), ("valid", valid, u8, lead, _OPT),
                     ("weights", weights, f, lead, {"optional": True, "align": 4}), ("stats", stats, f, (8,)),
                     ("out", out, f, lead + (5, A), {"align": 4}))
        _check_grad_loss(grad_loss, b.device)
        if logits.numel():
            b._enqueue(b._lib.ccx_c51_loss_backward, actions.numel(), A, logits.detach(), actions, proj.detach(), valid, weights, stats,
                       grad_loss, out)
        return out


class _CategoricalLoss(torch.autograd.Function):
    """:meth:`CategoricalQ.loss` for logits that require a gradient: the forward is the two kernels of ``ccx_c51_loss``, the
    backward the one of ``ccx_c51_loss_backward``; saved are the logits, ``proj`` and ``stats``.  Only ``stats[0]``, the loss,
    is differentiable: the gradient arriving at the other seven is not read."""

    @staticmethod
    def forward(ctx, cq, logits, actions, reward, done, nt, no, masks_next, valid, weights, discount, gamma, row_loss, proj):
        logits = logits.detach()
        stats = _new_stats(cq.batch.device)
        cq._forward(logits, actions, reward, done, nt, no, masks_next, valid, weights, discount, gamma,
                    cq._workspace_arg(None, actions.numel()), stats, row_loss, proj)
        ctx.cq = cq
        ctx.rest = (actions, valid, weights)
        ctx.save_for_backward(logits, proj, stats)
        return stats

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_stats):
        logits, proj, stats = ctx.saved_tensors
        actions, valid, weights = ctx.rest
        g = ctx.cq.loss_backward(logits, actions, proj, valid, weights, stats=stats, grad_loss=grad_stats.contiguous())
        return (None, g) + (None,) * 12
