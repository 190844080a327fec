"""N-step targets on the device (include/ccx.h CCX_NSTEP) over a :class:`~collectivecrossing_amd.replay.ReplayRing`: one byte
per record that says whether the env's episode ended with it, and ONE kernel that walks every drawn record forward through
its successors in the ring and writes the minibatch of :meth:`ReplayRing.fetch` with the discounted n-step reward, the state
the window ends on, and per row the discount ``gamma^m`` that :meth:`~collectivecrossing_amd.qlearn.QLearning.td_loss` takes
as ``discount=``.

:class:`NStepReplay` composes a ring (``ns.ring``) and is a class of its own for the reason ``replay.py`` gives: it brings its
own proof of the stream-order contract (tests/test_gpu_stream_order_nstep.py)."""

from __future__ import annotations

from dataclasses import dataclass

import torch

from ._abi import NSTEP_MAX
from .learner import _OPT, _require_all, _require_out
from .qlearn import _check_gamma
from .replay import ReplayBatch, ReplayRing, _check_batch_size, _check_index


@dataclass
class NStepBatch:
    """An n-step minibatch (:meth:`NStepReplay.sample` / :meth:`NStepReplay.fetch`).  ``batch.reward`` is the discounted
    reward of the window, ``batch.done`` / ``batch.next_obs`` / ``batch.masks_next`` are those of the record it ends on,
    ``batch.valid`` is 0 for a dropped row."""

    batch: ReplayBatch              # the records drawn, with the window's target in the place of the step's
    discount: torch.Tensor          # f32 [B, N]: gamma^span, what the row's bootstrap is multiplied by
    span: torch.Tensor              # u8 [B, N]: steps the row's reward covers (1 .. n)

    index = property(lambda self: self.batch.index)                      # int64 [B]: the records drawn, as ``ReplayBatch.index``


def _check_n(n, steps: int) -> int:
    try:
        ok = int(n) == n and 1 <= int(n) <= min(int(steps), NSTEP_MAX)
    except (TypeError, ValueError):
        ok = False
    if not ok:
        raise ValueError(f"n must be an integer in 1 .. min(steps, {NSTEP_MAX}) = {min(int(steps), NSTEP_MAX)}, got {n!r}")
    return int(n)


class NStepReplay:
    """``NStepReplay(ring, n=3, gamma=0.99)``: n-step windows over the R records of ``ring``.

    Storage, allocated here and public (tests, checkpoints): ``cut`` u8 [R], not zero where the env's episode ended with
    the record (initially 0).  ``n`` in ``1 .. min(ring.steps, 16)`` and ``gamma`` in [0, 1] travel by value.

    The window of a record starts at it and runs through the same env's records in the following ring steps: it ends after
    ``n`` steps, at a cut, or at the newest record pushed, whichever comes first (``m_env`` steps); an agent's share of it
    ends earlier where the agent terminates (``span`` steps).  The rule is stated line by line in include/ccx.h CCX_NSTEP.
    With ``n = 1`` everything :meth:`fetch` shares with :meth:`ReplayRing.fetch` has its bits.

    Every method that enqueues keeps the stream-order contract of :class:`~collectivecrossing_amd.learner.LearnerOps`
    through the batch's ``_enqueue``; ``cut`` travels as an argument.  Anything else than the tensors described raises
    ``ValueError`` before the library is called.  Not here: n above 16, a per-agent next state for dropped rows,
    lambda-returns or Retrace, n-step inside the actor, sequences, rings across GPUs."""

    def __init__(self, ring: ReplayRing, n: int = 3, gamma: float = 0.99):
        if not isinstance(ring, ReplayRing):
            raise ValueError("ring must be a ReplayRing")
        self.ring = ring
        self.batch = ring.batch
        self.n = _check_n(n, ring.steps)
        self.gamma = _check_gamma(gamma)
        self.cut = torch.zeros((ring.records,), dtype=torch.uint8, device=self.batch.device)

    def clear(self) -> None:
        """``cut`` to 0 and the ring cleared: fills on the handle's stream, ordered like a launch (only enqueues)."""
        b = self.batch
        cur = b._order_after_current_stream(self.cut)
        with torch.cuda.stream(b._stream):
            self.cut.zero_()
        b._current_stream_waits(cur=cur)
        self.ring.clear()

    # ------------------------------------------------------------------ rollout arrays to records
    def push(self, obs0_compact: torch.Tensor, actions: torch.Tensor, traj, masks_next: torch.Tensor | None = None) -> None:
        """:meth:`ReplayRing.push` with the same arguments, and ``cut`` at the K * E slots it wrote (``ccx_nstep_push``: one
        kernel behind the ring's two, which reads the ring's head on the device): 1 where the step's env flags say the
        episode ended (all terminated, all truncated, or auto-reset), else 0.  A captured push advances with every replay.
        Only enqueues (no host synchronisation); stream order: :class:`LearnerOps`."""
        from .batched import RolloutResult

        ring, b = self.ring, self.batch
        ring.push(obs0_compact, actions, traj, masks_next=masks_next)    # (checks everything, K and env_flags among it)
        env_flags = traj.env_flags if isinstance(traj, RolloutResult) else traj[2]
        b._enqueue(b._lib.ccx_nstep_push, ring.steps, ring.state, int(actions.shape[0]), env_flags, self.cut)

    def mark_cut(self, env_mask: torch.Tensor | None = None) -> None:
        """``cut = 1`` at the newest ring step for the envs whose byte of ``env_mask`` u8 [E] is not zero (``None``: all
        envs); nothing while the ring is empty (``ccx_nstep_mark_cut``, one kernel).  Call it after restarting envs by hand
        between two pushes (``reset``, ``reset_from_pool``): the library cannot see that the next record pushed is not the
        continuation of the last one.
        Only enqueues (no host synchronisation); stream order: :class:`LearnerOps`."""
        ring, b = self.ring, self.batch
        _require_all(b.device, ("env_mask", env_mask, torch.uint8, (b.num_envs,), _OPT))
        b._enqueue(b._lib.ccx_nstep_mark_cut, ring.steps, ring.state, env_mask, self.cut)

    # ------------------------------------------------------------------ records to a minibatch
    def alloc_batch(self, B: int, want_obs: bool = True, want_next_obs: bool = True) -> NStepBatch:
        """Output tensors of :meth:`sample` / :meth:`fetch` for B records (static buffers for a captured graph)."""
        b = self.batch
        mb = self.ring.alloc_batch(B, want_obs, want_next_obs)
        shape = (int(B), b.num_agents)
        return NStepBatch(mb, b._new(shape, torch.float32), b._new(shape, torch.uint8))

    def _out(self, B: int, out, want_obs: bool, want_next_obs: bool) -> NStepBatch:
        b = self.batch
        _require_out(out, NStepBatch, "alloc_batch")
        if out is None:
            return self.alloc_batch(B, want_obs, want_next_obs)
        _require_out(out.batch, ReplayBatch, "alloc_batch")
        self.ring._out(B, out.batch, want_obs, want_next_obs)
        _require_all(b.device, ("out.discount", out.discount, torch.float32, (B, b.num_agents)),
                     ("out.span", out.span, torch.uint8, (B, b.num_agents)))
        return out

    def _window_args(self) -> tuple:
        return (*self.ring._ring_args(), self.cut, self.n, self.gamma)

    def sample(self, B: int, out: NStepBatch | None = None, want_obs: bool = True, want_next_obs: bool = True) -> NStepBatch:
        """Draw B records exactly as :meth:`ReplayRing.sample` draws them (the same stream, key and range: for equal state
        the same ``index``) and write their n-step minibatch (``ccx_nstep_sample``): ONE kernel, and one plain lane behind it
        that advances the ring's ``draws``.  ``out`` reuses an :class:`NStepBatch` of the same B (:meth:`alloc_batch`).
        Only enqueues (no host synchronisation); stream order: :class:`LearnerOps`."""
        b = self.batch
        B = _check_batch_size(B, b.num_agents)
        out = self._out(B, out, want_obs, want_next_obs)
        b._enqueue(b._lib.ccx_nstep_sample, *self._window_args(), B, *ReplayRing._out_args(out.batch), out.discount, out.span)
        return out

    def fetch(self, index: torch.Tensor, out: NStepBatch | None = None, want_obs: bool = True,
              want_next_obs: bool = True) -> NStepBatch:
        """The n-step minibatch of the caller's record indices, int64 [B] (``ccx_nstep_fetch``, ONE kernel; include/ccx.h
        CCX_NSTEP states the rule).  Per record the window covers ``m_env`` steps: it stops at ``n``, behind a record whose
        ``cut`` is set, or at the newest record.  Per agent ``span`` is its share of them (it stops behind the step the
        agent terminated in), ``batch.reward`` = ``sum_k gamma^k reward_k`` over them in f64, ``discount`` = ``gamma^span``
        as f32, ``batch.done`` the agent's ``done`` in its last step; ``batch.next_obs`` and ``batch.masks_next`` are those
        of the record the env's window ends on; ``batch.obs``, ``batch.actions`` and ``batch.index`` those of the record
        itself.  A row whose agent stopped being live inside the window without terminating is dropped (``batch.valid`` 0).
        An index outside ``[0, records)`` gives the EMPTY record with ``discount`` = ``gamma`` and ``span`` 1.
        Only enqueues (no host synchronisation); stream order: :class:`LearnerOps`."""
        b = self.batch
        B = _check_index(b.device, index, b.num_agents)
        out = self._out(B, out, want_obs, want_next_obs)
        b._enqueue(b._lib.ccx_nstep_fetch, *self._window_args(), B, index, *ReplayRing._out_args(out.batch), out.discount,
                   out.span)
        return out

    # ------------------------------------------------------------------ checkpoints (host-synchronous: outside the contract)
    def state_dict(self) -> dict:
        """Copies of ``cut``, ``n``, ``gamma`` and the ring's own dict."""
        ring = self.ring.state_dict()                                    # (waits for the handle's stream)
        sd = {"cut": self.cut.clone(), "n": self.n, "gamma": self.gamma, "ring": ring}
        torch.cuda.synchronize(self.batch.device)
        return sd

    def load_state_dict(self, sd: dict) -> None:
        """Continue from a :meth:`state_dict` over a ring of the same geometry: exact copies; host-synchronous."""
        try:
            cut, ring = sd["cut"], sd["ring"]
            n, gamma = _check_n(sd["n"], self.ring.steps), _check_gamma(sd["gamma"])
        except (KeyError, TypeError):
            raise ValueError("not an NStepReplay state_dict (keys cut, n, gamma, ring)") from None
        if not isinstance(cut, torch.Tensor) or cut.dtype is not torch.uint8 or cut.shape != self.cut.shape:
            raise ValueError(f"state_dict cut must be a torch.uint8 tensor of shape {tuple(self.cut.shape)}")
        self.ring.load_state_dict(ring)                                  # (checks the geometry; synchronises)
        self.cut.copy_(cut)
        self.n, self.gamma = n, gamma
        torch.cuda.synchronize(self.batch.device)
