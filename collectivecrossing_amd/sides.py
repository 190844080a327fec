"""Per-side policy heads (include/ccx.h CCX_SIDES): a set of :class:`~collectivecrossing_amd.learner.MlpHead`, each owning a
set of agent slots, run directly on the ``[..., N, L]`` arrays a rollout wrote -- the actor launch, the learner's forward and
the bit-defined backward -- without a gathered copy.  Every output is, bit for bit, what the existing call gives on the
gathered rows (``MlpHead``, ``mlp_sample_actions``, ``mlp_backward``).

:class:`SideHeads` is a class of its own, not a set of methods of the batch: the stream-order table of the batch's classes
(tests/_stream_order.py) is closed, and this class brings its own proof (tests/test_gpu_sides_stream_order.py)."""

from __future__ import annotations

import numpy as np
import torch

from ._abi import SIDES_MAX_GROUPS, CcxSlotGroup
from .batched import scripted_slot_mask
from .learner import MlpGradResult, MlpHead, SampleResult, _OPT, _require, _require_all, _require_out


def _slots_of(mask: int) -> list[int]:
    return [a for a in range(64) if mask >> a & 1]


class SideHeads(torch.nn.Module):
    """Up to eight heads over disjoint sets of agent slots of one batch, e.g. ``SideHeads(batch, {"boarding":
    batch.mlp_head(64), "exiting": batch.mlp_head(64)})``.  A key is anything :func:`~collectivecrossing_amd.batched.
    scripted_slot_mask` accepts: ``"boarding"``, ``"exiting"``, ``"all"``, an agent id, a list of slots / ids, an int mask.
    All heads share ``(L, H, O, activation)``; slots that no head owns are left alone (a learner beside scripted agents).
    ``groups`` lists ``(mask, head)`` in ascending order of the lowest slot; ``parameters()`` are the heads' in that order
    (``w1t, b1, w2, b2`` each), so two :class:`SideHeads` of eight groups fill a :class:`DeviceAdam`.

    ``sides(x, out=None, hidden_out=None)``: ``x`` f32 ``[..., N, L]`` (contiguous, 16-byte aligned) to f32 ``[..., N, O]``
    in ONE launch (``ccx_sides_forward``): the rows of a head's slots get exactly that head's ``MlpHead`` outputs.  Rows of
    unowned slots are not read; their elements of ``out`` / ``hidden_out`` are not written (+0.0 in an output the call
    allocates itself).  ``hidden_out`` f32 ``[..., N, H]`` receives the activations: with :meth:`backward_into` the
    static-buffer pair for a captured graph.  When grad mode is on and a parameter requires a gradient, the call is a
    ``torch.autograd.Function``: the same launch with the activations saved; its backward is ``ccx_sides_backward`` per
    group -- always the device rule, the members' ``backward=`` is not consulted -- so each head's four ``.grad`` equal,
    bit for bit, what ``mlp_backward`` gives on the gathered rows.  There ``out=`` and ``hidden_out=`` are refused, and an
    ``x`` that requires a gradient raises ``ValueError`` (the gradient with respect to the rows is not formed).

    Anything else than the tensors described raises ``ValueError`` before the library is called; zero rows return empty
    tensors without calling it.  Every method that enqueues keeps the stream-order contract of
    :class:`~collectivecrossing_amd.learner.LearnerOps` through the batch's ``_enqueue``."""

    def __init__(self, batch, heads):
        super().__init__()
        try:
            items = list(heads.items())
        except AttributeError:
            raise ValueError("heads must be a dict {slots: MlpHead}") from None
        if not 1 <= len(items) <= SIDES_MAX_GROUPS:
            raise ValueError(f"heads must hold 1..{SIDES_MAX_GROUPS} groups, got {len(items)}")
        groups, seen = [], 0
        for key, head in items:
            mask = scripted_slot_mask(batch.config, key)
            if not isinstance(head, MlpHead) or head.batch is not batch:
                raise ValueError(f"heads[{key!r}] must be an MlpHead of this batch (mlp_head)")
            if mask == 0:
                raise ValueError(f"heads[{key!r}] owns no agent slot")
            if mask & seen:
                raise ValueError(f"heads[{key!r}] owns slots {_slots_of(mask & seen)}, which an earlier group owns too")
            seen |= mask
            groups.append((mask, head))
        groups.sort(key=lambda g: g[0] & -g[0])
        first = groups[0][1]
        for mask, head in groups:
            if head.dims != first.dims:
                raise ValueError(f"all heads must share (L, H, O, activation): {first.extra_repr()} and {head.extra_repr()}")
        object.__setattr__(self, "batch", batch)                          # (not a submodule, not part of the state dict)
        self.heads = torch.nn.ModuleList(head for _, head in groups)
        self.masks = tuple(mask for mask, _ in groups)
        self.L, self.H, self.O, self.activation = first.L, first.H, first.O, first.activation
        self.dims = first.dims
        self.owned = seen
        self.all_owned = seen == (1 << batch.num_agents) - 1

    @property
    def groups(self) -> list:
        return list(zip(self.masks, self.heads))

    def extra_repr(self) -> str:
        return ", ".join(f"{mask:#x}" for mask in self.masks)

    def slot_mask(self, i: int, device=None) -> torch.Tensor:
        """Group ``i``'s slots as a u8 ``[N]`` tensor of 0 / 1 (broadcast it against ``valid`` for a per-side loss)."""
        n = self.batch.num_agents
        return torch.tensor([self.masks[i] >> a & 1 for a in range(n)], dtype=torch.uint8, device=device or self.batch.device)

    # ------------------------------------------------------------------ helpers
    def _table(self):
        table = (CcxSlotGroup * len(self.masks))()
        for row, mask, head in zip(table, self.masks, self.heads):
            head._check_parameters()
            row.slots, row.w1t, row.b1, row.w2, row.b2 = mask, head.w1t.data_ptr(), head.b1.data_ptr(), head.w2.data_ptr(), head.b2.data_ptr()
        return table

    def _param_tensors(self) -> list:
        return [p.detach() for head in self.heads for p in (head.w1t, head.b1, head.w2, head.b2)]

    def _new_output(self, shape) -> torch.Tensor:
        """An output the call allocates: unowned rows hold +0.0, never whatever the allocator left."""
        b = self.batch
        return b._new(shape, torch.float32) if self.all_owned else torch.zeros(shape, dtype=torch.float32, device=b.device)

    def _forward(self, x, y, hidden) -> None:
        b, N = self.batch, self.batch.num_agents
        table = self._table()
        b._enqueue(b._lib.ccx_sides_forward, x.numel() // (N * self.L), N, *self.dims, x, len(table), table, y, hidden,
                   also=self._param_tensors())

    def _backward(self, x, hidden, grad_y, outs) -> None:
        """``ccx_sides_backward`` per group on checked tensors; ``outs``: one :class:`MlpGradResult` per group."""
        b, N = self.batch, self.batch.num_agents
        M = x.numel() // (N * self.L)
        todo = []
        for mask, head, out in zip(self.masks, self.heads, outs):
            head._check_parameters()
            todo.append((mask, head.w2.detach(), out, b._mlp_backward_workspace(self.dims, M * bin(mask).count("1"), out.workspace)))
        for mask, w2, out, ws in todo:
            b._enqueue(b._lib.ccx_sides_backward, M, N, mask, *self.dims, x, hidden, grad_y, w2, ws, out.w1t, out.b1, out.w2,
                       out.b2, out.grad_a)

    def _check_rows(self, x) -> tuple:
        b = self.batch
        _require("x", x, torch.float32, (..., b.num_agents, self.L), b.device, align=16)
        return tuple(x.shape[:-1])

    # ------------------------------------------------------------------ rows to logits
    def forward(self, x: torch.Tensor, out: torch.Tensor | None = None, hidden_out: torch.Tensor | None = None) -> torch.Tensor:
        b = self.batch
        lead = self._check_rows(x)
        if torch.is_grad_enabled() and any(p.requires_grad for p in self.parameters()):
            if x.requires_grad:
                raise ValueError("x must not require a gradient (the gradient with respect to the rows is not formed)")
            if out is not None or hidden_out is not None:
                raise ValueError("out= and hidden_out= cannot be used when a gradient is required (the autograd path allocates "
                                 "its outputs)")
            if x.numel() == 0:
                return x.new_zeros(lead + (self.O,)) + sum(p.sum() for p in self.parameters()) * 0.0
            return _SidesForward.apply(self, x, *self.parameters())
        if out is None:
            out = self._new_output(lead + (self.O,))
        _require_all(b.device, ("out", out, torch.float32, lead + (self.O,)),
                     ("hidden_out", hidden_out, torch.float32, lead + (self.H,), {"optional": True, "align": 16}))
        if x.numel():
            self._forward(x.detach(), out, hidden_out)
        return out

    # ------------------------------------------------------------------ observation rows to actions
    def sample_actions(self, obs: torch.Tensor, masks: torch.Tensor | None = None, deterministic: bool = False,
                       want_logp: bool = True, want_entropy: bool = False, logits_out: torch.Tensor | None = None,
                       out: SampleResult | None = None) -> SampleResult:
        """Observation rows to actions in ONE launch (``ccx_sides_sample_actions``): by definition
        ``batch.sample_actions(sides(obs), masks, ...)`` -- the same key, the same rule for terminated or truncated agents,
        the same bits in ``actions``, ``logp`` and ``entropy``.  Needs ``O == 5`` and ``L == obs_len``; ``obs`` f32 [E, N, L]
        (contiguous, 16-byte aligned).  A slot that no head owns gets action 255 and ``logp`` = ``entropy`` = +0.0 (what
        :meth:`step_mixed` expects for the slots it scripts); its ``logits_out`` elements are not written.  ``masks``,
        ``deterministic``, ``want_*`` and ``out`` are :meth:`BatchedCollectiveCrossing.sample_actions`'.  No gradient flows
        through this call.  Only enqueues (no host synchronisation); stream order: :class:`LearnerOps`."""
        b = self.batch
        E, N = b.num_envs, b.num_agents
        if self.O != 5 or self.L != b.obs_len:
            raise ValueError(f"sample_actions needs heads with O == 5 and L == obs_len == {b.obs_len}, got O = {self.O}, L = {self.L}")
        _require_out(out, SampleResult, "alloc_sample")
        if out is None:
            out = b.alloc_sample(want_logp, want_entropy)
        _require_all(b.device,
                     ("obs", obs, torch.float32, (E, N, b.obs_len), {"align": 16}), ("masks", masks, torch.uint8, (E, N), _OPT),
                     ("logits_out", logits_out, torch.float32, (E, N, 5), _OPT),
                     ("out.actions", out.actions, torch.uint8, (E, N)), ("out.logp", out.logp, torch.float32, (E, N), _OPT),
                     ("out.entropy", out.entropy, torch.float32, (E, N), _OPT))
        table = self._table()
        b._enqueue(b._lib.ccx_sides_sample_actions, self.H, self.dims[3], obs, len(table), table, masks,
                   int(bool(deterministic)), out.actions, out.logp, out.entropy, logits_out, also=self._param_tensors())
        return out

    # ------------------------------------------------------------------ the backward pass
    def alloc_backward(self, shape, want_grad_a: bool = False) -> list:
        """Static buffers of :meth:`backward_into` for rows of the leading shape ``shape`` = ``(..., N)``: one
        :class:`MlpGradResult` per group (four gradients and a workspace each); with ``want_grad_a`` they share ONE
        ``grad_a`` f32 ``[..., N, H]``, of which every group writes its own rows."""
        b = self.batch
        shape = tuple(int(v) for v in shape)
        if shape[-1:] != (b.num_agents,):
            raise ValueError(f"shape must end in N = {b.num_agents}, got {shape}")
        M = int(np.prod(shape[:-1])) if shape[:-1] else 1
        f = torch.float32
        grad_a = self._new_output(shape + (self.H,)) if want_grad_a else None
        return [MlpGradResult(b._new((self.L, self.H), f), b._new((self.H,), f), b._new((self.O, self.H), f), b._new((self.O,), f),
                              grad_a, b._mlp_backward_workspace(self.dims, max(M, 1) * bin(mask).count("1"), None))
                for mask in self.masks]

    def backward_into(self, x: torch.Tensor, hidden: torch.Tensor, grad_y: torch.Tensor, want_grad_a: bool = False,
                      out: list | None = None) -> list:
        """The gradients of every head's four parameter arrays from the gradient of the outputs (``ccx_sides_backward``
        per group: two launches each), one :class:`MlpGradResult` per group in the order of ``groups``: bit for bit what
        :meth:`BatchedCollectiveCrossing.mlp_backward` gives on the group's gathered rows.  ``x`` f32 [..., N, L], ``hidden``
        f32 [..., N, H] (what ``sides(x, hidden_out=)`` wrote; both 16-byte aligned), ``grad_y`` f32 [..., N, O]; only the
        rows of a group's slots are read.  ``grad_a`` (``want_grad_a``, or ``out``'s) is written at owned rows only.  ``out``
        reuses the list of :meth:`alloc_backward`.  Zero rows give zeros without calling the library.
        Only enqueues (no host synchronisation); stream order: :class:`LearnerOps`."""
        b = self.batch
        lead = self._check_rows(x)
        if out is None:
            out = self.alloc_backward(lead, want_grad_a)
        if not isinstance(out, (list, tuple)) or len(out) != len(self.masks) or not all(isinstance(o, MlpGradResult) for o in out):
            raise ValueError(f"out must be a list of {len(self.masks)} MlpGradResult (alloc_backward)")
        f = torch.float32
        rows = [("hidden", hidden, f, lead + (self.H,), {"align": 16}), ("grad_y", grad_y, f, lead + (self.O,))]
        for i, o in enumerate(out):
            rows += [(f"out[{i}].w1t", o.w1t, f, (self.L, self.H)), (f"out[{i}].b1", o.b1, f, (self.H,)),
                     (f"out[{i}].w2", o.w2, f, (self.O, self.H)), (f"out[{i}].b2", o.b2, f, (self.O,)),
                     (f"out[{i}].grad_a", o.grad_a, f, lead + (self.H,), {"optional": True, "align": 16})]
        _require_all(b.device, *rows)
        if x.numel() == 0:
            for o in out:
                for t in (o.w1t, o.b1, o.w2, o.b2):
                    t.zero_()
            return list(out)
        self._backward(x.detach(), hidden.detach(), grad_y.detach(), out)
        return list(out)


class _SidesForward(torch.autograd.Function):
    """:class:`SideHeads` when a gradient is required: the forward is the one launch of ``ccx_sides_forward`` with the
    activations saved; the backward is ``ccx_sides_backward`` per group."""

    @staticmethod
    def forward(ctx, sides, x, *params):
        x = x.detach()
        lead = tuple(x.shape[:-1])
        y = sides._new_output(lead + (sides.O,))
        hidden = sides.batch._new(lead + (sides.H,), torch.float32)
        sides._forward(x, y, hidden)
        ctx.sides = sides
        ctx.save_for_backward(x, hidden)
        return y

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, gy):
        x, hidden = ctx.saved_tensors
        sides = ctx.sides
        b, f = sides.batch, torch.float32
        L, H, O = sides.L, sides.H, sides.O
        outs = [MlpGradResult(b._new((L, H), f), b._new((H,), f), b._new((O, H), f), b._new((O,), f), None, None)
                for _ in sides.masks]
        sides._backward(x, hidden, gy.contiguous(), outs)
        grads = [g for o in outs for g in (o.w1t, o.b1, o.w2, o.b2)]
        return (None, None) + tuple(g if need else None for g, need in zip(grads, ctx.needs_input_grad[2:]))
