"""Proportional prioritised replay on the device (include/ccx.h CCX_PRIO) over a :class:`~collectivecrossing_amd.replay.ReplayRing`:
one fixed-point integer priority per record, an exact integer sum tree rebuilt by every draw, keyed draws (stratified or not)
with the library's counter-based word, importance weights in the shape ``td_loss`` takes, and an update from ``td_loss``'s
``td_error`` outputs that is well defined for duplicate indices.

:class:`PrioritizedReplay` composes a ring (``pr.ring``) and is a class of its own for the reason ``replay.py`` gives: it
brings its own proof of the stream-order contract (tests/test_gpu_stream_order_prio.py)."""

from __future__ import annotations

import ctypes as C
from dataclasses import dataclass

import numpy as np
import torch

from ._abi import PRIO_MAX_TD
from .learner import _require_all, _require_out
from .nstep import NStepBatch, NStepReplay
from .replay import ReplayBatch, ReplayRing, _check_batch_size, _check_index

ONE = 65536                                                              # 1.0 in fixed point: 16 fractional bits


@dataclass
class PrioritizedBatch:
    """A prioritised minibatch (:meth:`PrioritizedReplay.sample`)."""

    batch: ReplayBatch | NStepBatch  # the records drawn (``index``: int64 [B], -1 where nothing is drawable); an NStepBatch over an NStepReplay
    weights: torch.Tensor           # f32 [B, N]: (p_min / p_i)^beta, the same for every agent of a record; +0.0 at index -1
    leaf_drawn: torch.Tensor        # int32 [B]: the leaf of each record drawn (0 at index -1)


def _check_unit(name: str, value, lo_open: bool = False) -> float:
    try:
        value = float(np.float32(value))
    except (TypeError, ValueError):
        raise ValueError(f"{name} must be a number") from None
    if not ((0.0 < value < float("inf")) if lo_open else (0.0 <= value <= 1.0)):     # (false for NaN)
        raise ValueError(f"{name} must be " + ("a finite number > 0" if lo_open else "in [0, 1]") + f", got {value!r}")
    return value


class PrioritizedReplay:
    """``PrioritizedReplay(ring, alpha=0.6, beta=0.4, eps=1e-6)``: priorities for the R records of ``ring``.

    ``ring`` is a :class:`ReplayRing`, or an :class:`~collectivecrossing_amd.nstep.NStepReplay` over one: :meth:`push` then
    marks the cuts too, :meth:`sample` fetches through it and ``PrioritizedBatch.batch`` is an ``NStepBatch``.  ``pr.ring`` is
    the :class:`ReplayRing` in either case, ``pr.nstep`` the ``NStepReplay`` or ``None``.

    Storage, allocated here and public (tests, checkpoints): ``leaf`` int32 [R], the record's priority ``p^alpha`` with 16
    fractional bits (0: never pushed, not drawable); ``pstate`` int64 [4] = {max_leaf, draws, T, min_leaf} ON THE DEVICE
    (``draws`` is this class's own launch counter; ``T`` and ``min_leaf`` are as of the latest :meth:`sample`); ``beta_dev``
    f32 [1] behind the float property :attr:`beta` (written on the handle's stream: a rate changed between two replays of a
    captured graph takes effect); and ``tree``, int64 work space of ``ccx_prio_tree_words(R)`` words that every
    :meth:`sample` rebuilds from ``leaf`` -- derived, private, never checkpointed.

    Every method that enqueues keeps the stream-order contract of :class:`~collectivecrossing_amd.learner.LearnerOps`
    through the batch's ``_enqueue``; the leaves, the tree, ``pstate`` and ``beta_dev`` travel as arguments.  Anything else
    than the tensors described raises ``ValueError`` before the library is called.  Not here: rank-based prioritisation,
    sampling without replacement, per-agent priorities, priorities shared across shards or GPUs."""

    def __init__(self, ring: ReplayRing | NStepReplay, alpha: float = 0.6, beta: float = 0.4, eps: float = 1e-6):
        if not isinstance(ring, (ReplayRing, NStepReplay)):
            raise ValueError("ring must be a ReplayRing or an NStepReplay")
        self.nstep = ring if isinstance(ring, NStepReplay) else None
        self.ring = ring = ring.ring if isinstance(ring, NStepReplay) else ring
        self.batch = b = ring.batch
        self.alpha = _check_unit("alpha", alpha)
        self.eps = _check_unit("eps", eps, lo_open=True)
        self._beta = _check_unit("beta", beta)
        dev, R = b.device, ring.records
        self.leaf = torch.zeros((R,), dtype=torch.int32, device=dev)
        self.pstate = torch.tensor([ONE, 0, 0, 0], dtype=torch.int64, device=dev)
        self.beta_dev = torch.full((1,), self._beta, dtype=torch.float32, device=dev)
        self.tree = torch.zeros((int(b._lib.ccx_prio_tree_words(R)),), dtype=torch.int64, device=dev)

    @property
    def beta(self) -> float:
        return self._beta

    @beta.setter
    def beta(self, value) -> None:
        self._beta = _check_unit("beta", value)
        b = self.batch
        cur = b._order_after_current_stream(self.beta_dev)
        with torch.cuda.stream(b._stream):
            self.beta_dev.fill_(self._beta)
        b._current_stream_waits(cur=cur)

    def clear(self) -> None:
        """Leaves to 0, ``pstate`` to {65536, 0, 0, 0}, and the ring cleared: fills on the handle's stream, ordered like a
        launch (only enqueues)."""
        b = self.batch
        cur = b._order_after_current_stream(self.leaf, self.pstate)
        with torch.cuda.stream(b._stream):
            self.leaf.zero_()
            self.pstate.zero_()
            self.pstate[:1].fill_(ONE)
        b._current_stream_waits(cur=cur)
        (self.nstep or self.ring).clear()

    # ------------------------------------------------------------------ rollout arrays to records
    def push(self, obs0_compact: torch.Tensor, actions: torch.Tensor, traj, masks_next: torch.Tensor | None = None) -> None:
        """:meth:`ReplayRing.push` with the same arguments, and ``leaf = max_leaf`` at the K * E slots it wrote
        (``ccx_prio_push``: one kernel behind the ring's two, which reads the ring's head and ``max_leaf`` on the device): a
        new record is drawn at least as often as any other until its TD error is known.  A captured push advances with
        every replay.  Only enqueues (no host synchronisation); stream order: :class:`LearnerOps`."""
        ring, b = self.ring, self.batch
        if self.nstep is None:
            ring.push(obs0_compact, actions, traj, masks_next=masks_next)    # (checks everything, K among it)
        else:
            self.nstep.push(obs0_compact, actions, traj, masks_next=masks_next)      # (the ring's push, and the cuts)
        b._enqueue(b._lib.ccx_prio_push, ring.steps, ring.state, int(actions.shape[0]), self.leaf, self.pstate)

    # ------------------------------------------------------------------ TD errors to priorities
    def update_priorities(self, index: torch.Tensor, td_error, alpha: float | None = None, eps: float | None = None) -> None:
        """New priorities for the records ``index`` int64 [B] from ``td_error``, one f32 [B, N] tensor or a tuple of up to 8
        (the per-side ``td_error`` outputs of ``td_loss``): per record ``(max |td| + eps)^alpha`` over all agents and arrays
        (a NaN never wins, +inf is clamped), in fixed point (``ccx_prio_update``, include/ccx.h CCX_PRIO; two kernels).  A
        slot named several times takes the MAXIMUM of its new values, whatever the order the lanes run in; an index
        outside ``[0, records)`` (the -1 of an empty draw) or of a slot never pushed changes nothing.  ``max_leaf`` follows.
        ``alpha`` in [0, 1] and ``eps`` > 0 default to the constructor's.
        Only enqueues (no host synchronisation); stream order: :class:`LearnerOps`."""
        b = self.batch
        alpha = self.alpha if alpha is None else _check_unit("alpha", alpha)
        eps = self.eps if eps is None else _check_unit("eps", eps, lo_open=True)
        tds = (td_error,) if isinstance(td_error, torch.Tensor) else tuple(td_error) if isinstance(td_error, (tuple, list)) else ()
        if not 1 <= len(tds) <= PRIO_MAX_TD:
            raise ValueError(f"td_error must be a tensor or a tuple of 1 .. {PRIO_MAX_TD} tensors")
        B = _check_index(b.device, index, b.num_agents,
                         lambda B: ((f"td_error[{a}]", t, torch.float32, (B, b.num_agents)) for a, t in enumerate(tds)))
        table = (C.c_void_p * len(tds))(*(t.data_ptr() for t in tds))
        b._enqueue(b._lib.ccx_prio_update, self.ring.steps, self.leaf, self.pstate, B, index, len(tds), table, alpha, eps, also=tds)

    # ------------------------------------------------------------------ records to a minibatch
    def alloc_batch(self, B: int, want_obs: bool = True, want_next_obs: bool = True) -> PrioritizedBatch:
        """Output tensors of :meth:`sample` for B records (static buffers for a captured graph)."""
        b = self.batch
        mb = (self.nstep or self.ring).alloc_batch(B, want_obs, want_next_obs)
        return PrioritizedBatch(mb, b._new((int(B), b.num_agents), torch.float32), b._new((int(B),), torch.int32))

    def sample(self, B: int, out: PrioritizedBatch | None = None, stratified: bool = True, want_obs: bool = True,
               want_next_obs: bool = True) -> PrioritizedBatch:
        """Draw B records in proportion to their leaves (``ccx_prio_sample``, include/ccx.h CCX_PRIO) and fetch them
        (:meth:`ReplayRing.fetch`, the ring's own kernel; over an ``NStepReplay`` its :meth:`fetch`).

        The sums over the leaves are rebuilt first (exact integers: the same bits for any order), ``T`` and ``min_leaf`` go
        to ``pstate``.  Draw b takes the two counter-based words of key ``(b, draws)`` on this class's stream of the batch's
        ``set_rng_seed`` as a 64-bit point ``x`` -- ``stratified``: ``floor((b 2^64 + x) / B)``, so draw b falls into the b-th
        of B equal strata of the total priority --, ``u = (x T) >> 64``, and ``index[b]`` is the smallest i with ``leaf[0] +
        ... + leaf[i] > u``; -1 where nothing is drawable.  ``weights[b, :]`` = ``(min_leaf / leaf[index[b]])^beta`` with
        ``beta`` read from the device: 1.0 exactly for the rarest record, +0.0 at index -1.  Then ``draws`` advances.  The
        same eager or captured, for any split into calls; nothing comes from torch's generator.  ``out`` reuses a
        :class:`PrioritizedBatch` of the same B (:meth:`alloc_batch`).
        Only enqueues (no host synchronisation); stream order: :class:`LearnerOps`."""
        b = self.batch
        B = _check_batch_size(B, b.num_agents)
        if B >= 1 << 31:
            raise ValueError("the batch size must stay below 2^31")
        _require_out(out, PrioritizedBatch, "alloc_batch")
        if out is None:
            out = self.alloc_batch(B, want_obs, want_next_obs)
        _require_out(out.batch, ReplayBatch if self.nstep is None else NStepBatch, "alloc_batch")
        _require_all(b.device, ("out.batch.index", out.batch.index, torch.int64, (B,)),      # (an NStepBatch hands out its records' index)
                     ("out.weights", out.weights, torch.float32, (B, b.num_agents)),
                     ("out.leaf_drawn", out.leaf_drawn, torch.int32, (B,)))
        b._enqueue(b._lib.ccx_prio_sample, self.ring.steps, self.leaf, self.pstate, self.beta_dev, self.tree, B, int(bool(stratified)),
                   out.batch.index, out.weights, out.leaf_drawn)
        if self.nstep is None:
            self.ring.fetch(out.batch.index, out=out.batch)
        else:
            self.nstep.fetch(out.batch.index, out=out.batch)
        return out

    # ------------------------------------------------------------------ checkpoints (host-synchronous: outside the contract)
    def state_dict(self) -> dict:
        """Copies of ``leaf``, ``pstate`` and ``beta``, the hyper-parameters and the ring's own dict; the tree is derived."""
        ring = (self.nstep or self.ring).state_dict()                    # (waits for the handle's stream; an NStepReplay's holds the ring's)
        sd = {"leaf": self.leaf.clone(), "pstate": self.pstate.clone(), "beta": self._beta, "alpha": self.alpha, "eps": self.eps,
              "ring": ring}
        torch.cuda.synchronize(self.batch.device)
        return sd

    def load_state_dict(self, sd: dict) -> None:
        """Continue from a :meth:`state_dict` over a ring of the same geometry: exact copies; host-synchronous."""
        try:
            leaf, pstate, ring = sd["leaf"], sd["pstate"], sd["ring"]
            alpha, eps = _check_unit("alpha", sd["alpha"]), _check_unit("eps", sd["eps"], lo_open=True)
            beta = _check_unit("beta", sd["beta"])
        except (KeyError, TypeError):
            raise ValueError("not a PrioritizedReplay state_dict (keys leaf, pstate, beta, alpha, eps, ring)") from None
        for k, s, d in (("leaf", leaf, self.leaf), ("pstate", pstate, self.pstate)):
            if not isinstance(s, torch.Tensor) or s.dtype is not d.dtype or s.shape != d.shape:
                raise ValueError(f"state_dict {k} must be a {d.dtype} tensor of shape {tuple(d.shape)}")
        (self.nstep or self.ring).load_state_dict(ring)                  # (checks the geometry; synchronises)
        self.leaf.copy_(leaf)
        self.pstate.copy_(pstate)
        self.alpha, self.eps = alpha, eps
        torch.cuda.synchronize(self.batch.device)
        self.beta = beta
        self.batch.synchronize()
