"""Wide MLP heads on the device (include/ccx.h CCX_MLP_WIDE): :class:`MlpHead`'s two-layer perceptron with up to 320 outputs
-- the ``[5, A]`` atom logits of a categorical head (:class:`~collectivecrossing_amd.categorical.CategoricalQ`) -- forward in
one launch (``ccx_mlp_wide_forward``) and the four parameter gradients in two (``ccx_mlp_wide_backward``), by CCX_MLP's
rule: a fixed sequence of f32 operations per row, f64 chains over blocks of 256 rows, the same bits for any split of the
rows into calls.  For ``O <= 8`` the bits are :class:`MlpHead`'s.

:class:`WideMlpHead` is a class of its own, not a wider :class:`MlpHead`, for the reason ``categorical.py`` gives: the
stream-order table of the batch's classes (tests/_stream_order.py) is closed, and this class brings its own proof
(tests/test_gpu_stream_order_mlp_wide.py).  It reaches the library only through the batch's ``_enqueue``."""

from __future__ import annotations

import numpy as np
import torch

from .learner import MlpGradResult, _require, _require_all, _require_out, _torch_head_backward, _TwoLayerHead

MAX_OUTPUTS = 320


class WideMlpHead(_TwoLayerHead):
    """``Linear(L, H) -> tanh | relu -> Linear(H, O)`` with ``1 <= O <= 320`` on the batch's device:
    ``WideMlpHead(batch, H, O, activation="tanh", L=None, backward="torch", out_shape=None)``.

    Everything :class:`~collectivecrossing_amd.learner.MlpHead` says holds here with the wider ``O``: the parameters
    ``w1t`` [L, H], ``b1`` [H], ``w2`` [O, H], ``b2`` [O] in the kernel's layout (``state_dict()`` / ``load_state_dict()`` for
    checkpoints, ``DeviceAdam(batch, head.parameters())`` updates what the kernel reads), initialised as ``torch.nn.Linear``
    initialises (the two layers drawn in order from torch's generator); :meth:`from_linear` / :meth:`to_sequential` convert by
    exact copies.  ``L`` defaults to the batch's ``obs_len``; ``H`` is a multiple of 16 in 16..256.

    ``head(x, out=None, hidden_out=None)``: ``x`` f32 [..., L], contiguous, 16-byte aligned; returns f32 [..., O] -- or
    ``[..., *out_shape]``, a view, when ``out_shape`` (a tuple whose product is ``O``) was given: ``(5, A)`` is what
    :meth:`CategoricalQ.q_values` and :meth:`CategoricalQ.loss` take.  ``out`` (either shape; 4-byte alignment is all it
    needs) and ``hidden_out`` (f32 [..., H], 16-byte aligned) reuse tensors: with :meth:`param_grads` ``(out=)`` the
    static-buffer pair for a captured graph.  When grad mode is on and a parameter or ``x`` requires a gradient the call is
    a ``torch.autograd.Function``: the same kernel, the same bits, ``hidden`` saved; ``out=`` / ``hidden_out=`` are refused;
    ``backward="torch"`` (the default) is the f32 torch composition (correct to rounding, NOT bit-defined), ``"device"`` is
    ``ccx_mlp_wide_backward`` (the four parameter gradients bit-defined; the gradient of ``x``, formed only when ``x``
    requires one, a torch product on ``grad_a``).  Anything else than the tensors described raises ``ValueError`` before the
    library is called; zero rows return empty tensors without calling it.
    Only enqueues (no host synchronisation); stream order: :class:`~collectivecrossing_amd.learner.LearnerOps`.  Not here:
    the fused obs -> action launch, wide heads in ``SideHeads`` or dueling, more than 320 outputs, a second hidden
    layer (``deep.py``'s :class:`~collectivecrossing_amd.deep.DeepMlpHead` has one, with up to 8 outputs), a
    bit-defined gradient with respect to ``x``, bf16 / f16, the vector and RLlib adapters."""

    MAX_OUTPUTS = MAX_OUTPUTS

    def __init__(self, batch, H: int, O: int, activation: str = "tanh", L: int | None = None, backward: str = "torch",
                 out_shape=None):
        from .batched import BatchedCollectiveCrossing

        super().__init__()
        if not isinstance(batch, BatchedCollectiveCrossing):
            raise ValueError("batch must be a BatchedCollectiveCrossing")
        self._setup(batch, H, O, activation, L, backward)
        if out_shape is not None:
            try:
                out_shape = tuple(int(v) for v in out_shape)
            except (TypeError, ValueError):
                raise ValueError(f"out_shape must be a tuple of ints, got {out_shape!r}") from None
            if not out_shape or min(out_shape) < 1 or int(np.prod(out_shape)) != O:
                raise ValueError(f"out_shape must be a tuple of positive ints whose product is O = {O}, got {out_shape!r}")
        self.out_shape = (O,) if out_shape is None else out_shape

    @classmethod
    def from_linear(cls, batch, lin1: torch.nn.Linear, lin2: torch.nn.Linear, activation: str = "tanh", backward: str = "torch",
                    out_shape=None) -> "WideMlpHead":
        """The head that computes ``lin2(act(lin1(x)))``: exact copies of the two layers' f32 parameters."""
        cls._check_linear_pair(lin1, lin2)
        head = cls(batch, lin1.out_features, lin2.out_features, activation, lin1.in_features, backward, out_shape)
        return head._copy_linear_pair(lin1, lin2)

    def extra_repr(self) -> str:
        return (f"L={self.L}, H={self.H}, O={self.O}, activation={self.activation}, backward={self.backward}, "
                f"out_shape={self.out_shape}")

    def _flat(self, name: str, t, lead):
        """``t`` f32 of shape ``lead + (O,)`` or ``lead + out_shape``, contiguous (so either is a view of the other)."""
        if isinstance(t, torch.Tensor) and tuple(t.shape) == lead + self.out_shape:
            shape = lead + self.out_shape
        else:
            shape = lead + (self.O,)
        _require(name, t, torch.float32, shape, self.batch.device, align=4)
        return t

    def _enqueue_forward(self, x, y, hidden) -> None:
        b = self.batch
        b._enqueue(b._lib.ccx_mlp_wide_forward, x.numel() // self.L, self.L, self.H, self.O, self.activation_id, x,
                   self.w1t, self.b1, self.w2, self.b2, y, hidden)

    def forward(self, x: torch.Tensor, out: torch.Tensor | None = None, hidden_out: torch.Tensor | None = None) -> torch.Tensor:
        b = self.batch
        _require("x", x, torch.float32, (..., self.L), b.device, align=16)
        self._check_parameters()
        lead = tuple(x.shape[:-1])
        if torch.is_grad_enabled() and (x.requires_grad or any(p.requires_grad for p in self.parameters())):
            if out is not None or hidden_out is not None:
                raise ValueError("out= and hidden_out= cannot be used when a gradient is required (the autograd path allocates "
                                 "its outputs)")
            if x.numel() == 0:
                return (x.new_zeros(lead + (self.O,)) + self.b2 * 0.0).reshape(lead + self.out_shape)
            return _WideForward.apply(self, x, self.w1t, self.b1, self.w2, self.b2).reshape(lead + self.out_shape)
        if out is None:
            out = b._new(lead + (self.O,), torch.float32)
        else:
            self._flat("out", out, lead)
        _require("hidden_out", hidden_out, torch.float32, lead + (self.H,), b.device, optional=True, align=16)
        if x.numel():
            self._enqueue_forward(x.detach(), out, hidden_out)
        return out.view(lead + self.out_shape)

    # ------------------------------------------------------------------ the parameter gradients
    def _workspace(self, rows: int, workspace):
        b = self.batch
        need = int(b._lib.ccx_mlp_wide_backward_workspace_bytes(int(rows), self.L, self.H, self.O))
        return b._workspace_arg(need, workspace, "alloc_param_grads")

    def alloc_param_grads(self, shape, want_grad_a: bool = False) -> MlpGradResult:
        """Static buffers of :meth:`param_grads` for rows of the leading shape ``shape``: the four gradients, ``grad_a`` if
        asked for, and the workspace (for a captured graph)."""
        b, f = self.batch, torch.float32
        shape = tuple(int(v) for v in shape)
        rows = int(np.prod(shape)) if shape else 1
        return MlpGradResult(b._new((self.L, self.H), f), b._new((self.H,), f), b._new((self.O, self.H), f), b._new((self.O,), f),
                             b._new(shape + (self.H,), f) if want_grad_a else None, self._workspace(max(rows, 1), None))

    def _param_grads(self, x, hidden, grad_y, w2, out: MlpGradResult) -> MlpGradResult:
        b, f = self.batch, torch.float32
        L, H, O = self.L, self.H, self.O
        lead = tuple(x.shape[:-1]) if isinstance(x, torch.Tensor) else ()
        _require("x", x, f, (..., L), b.device)
        self._flat("grad_y", grad_y, lead)
        _require_all(b.device, ("x", x, f, (..., L), {"align": 16}), ("hidden", hidden, f, lead + (H,), {"align": 16}),
                     ("w2", w2, f, (O, H)), ("out.w1t", out.w1t, f, (L, H)), ("out.b1", out.b1, f, (H,)),
                     ("out.w2", out.w2, f, (O, H)), ("out.b2", out.b2, f, (O,)),
                     ("out.grad_a", out.grad_a, f, lead + (H,), {"optional": True, "align": 16}))
        rows = x.numel() // L
        if rows == 0:
            for t in (out.w1t, out.b1, out.w2, out.b2):
                t.zero_()
            return out
        workspace = self._workspace(rows, out.workspace)
        b._enqueue(b._lib.ccx_mlp_wide_backward, rows, L, H, O, self.activation_id, x.detach(), hidden.detach(), grad_y.detach(),
                   w2.detach(), workspace, out.w1t, out.b1, out.w2, out.b2, out.grad_a)
        return out

    def param_grads(self, x: torch.Tensor, hidden: torch.Tensor, grad_y: torch.Tensor, want_grad_a: bool = False,
                    out: MlpGradResult | None = None, workspace: torch.Tensor | None = None) -> MlpGradResult:
        """The gradients of the four parameter arrays from the gradient of the outputs, on the device
        (``ccx_mlp_wide_backward``, include/ccx.h CCX_MLP_WIDE): two kernels on the handle's stream, bit-defined -- f32 per
        row, then f64 chains over blocks of 256 rows and the fixed final step -- so the same rows give the same gradient bits
        on any machine, eager or captured.

        ``x`` f32 [..., L] (contiguous, 16-byte aligned), ``hidden`` f32 [..., H] (what the forward saved: ``head(x,
        hidden_out=)``; 16-byte aligned), ``grad_y`` f32 [..., O] or [..., *out_shape] (contiguous: the ``[..., 5, A]``
        gradient of :meth:`CategoricalQ.loss` is taken as it is, without a copy).  ``want_grad_a`` also returns the gradient
        at the pre-activations, f32 [..., H].  ``out`` reuses a result of :meth:`alloc_param_grads` (its ``grad_a`` and its
        workspace decide; ``want_grad_a`` and ``workspace`` are then ignored); ``workspace`` reuses a u8 tensor of at least
        ``ccx_mlp_wide_backward_workspace_bytes`` bytes, 8-byte aligned; otherwise it comes from torch's allocator, so the
        call captures.  A wrong dtype, shape or device, a non-contiguous tensor, a misaligned pointer or a workspace that
        is too small raises ``ValueError`` before the library is called; zero rows return zeros without calling it.
        Only enqueues (no host synchronisation); stream order: :class:`~collectivecrossing_amd.learner.LearnerOps`."""
        self._check_parameters()
        _require_out(out, MlpGradResult, "alloc_param_grads")
        if out is None:
            b, f = self.batch, torch.float32
            lead = tuple(x.shape[:-1]) if isinstance(x, torch.Tensor) else ()
            out = MlpGradResult(b._new((self.L, self.H), f), b._new((self.H,), f), b._new((self.O, self.H), f), b._new((self.O,), f),
                                b._new(lead + (self.H,), f) if want_grad_a else None, workspace)
        return self._param_grads(x, hidden, grad_y, self.w2, out)


class _WideForward(torch.autograd.Function):
    """:class:`WideMlpHead` when a gradient is required: the forward is the kernel of CCX_MLP_WIDE with the activations
    saved; the backward is ordinary f32 torch on them (``backward="torch"``: not bit-defined) or ``ccx_mlp_wide_backward``
    (``"device"``: the four parameter gradients bit-defined; the gradient of ``x``, where required, a torch product on its
    ``grad_a``)."""

    @staticmethod
    def forward(ctx, head, x, w1t, b1, w2, b2):
        x = x.detach()
        b = head.batch
        y = b._new(tuple(x.shape[:-1]) + (head.O,), torch.float32)
        hidden = b._new(tuple(x.shape[:-1]) + (head.H,), torch.float32)
        head._enqueue_forward(x, y, hidden)
        ctx.head = head
        ctx.save_for_backward(x, w1t.detach(), w2.detach(), hidden)
        return y

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, gy):
        x, w1t, w2, hidden = ctx.saved_tensors
        head = ctx.head
        L, H, O = head.L, head.H, head.O
        need = ctx.needs_input_grad
        gy = gy.contiguous()
        if head.backward == "device":
            b, f = head.batch, torch.float32
            out = MlpGradResult(b._new((L, H), f), b._new((H,), f), b._new((O, H), f), b._new((O,), f),
                                b._new(tuple(hidden.shape), f) if need[1] else None, None)
            head._param_grads(x, hidden, gy, w2, out)
            gx = (out.grad_a.reshape(-1, H) @ w1t.t()).reshape(x.shape) if need[1] else None
            return (None, gx, out.w1t if need[2] else None, out.b1 if need[3] else None, out.w2 if need[4] else None,
                    out.b2 if need[5] else None)
        return _torch_head_backward(head.activation == "relu", need, gy, x, w1t, w2, hidden)
