"""Deep MLP heads on the device (include/ccx.h CCX_MLP_DEEP): ``Linear(L, H1) -> act -> Linear(H1, H2) -> act ->
Linear(H2, O)`` -- the fully connected net of two hidden layers that RLlib trains by default, the usual ``64-64 tanh`` PPO
baseline -- forward in one launch (``ccx_mlp_deep_forward``), fused with the action draw in one launch
(``ccx_mlp_deep_sample_actions``, ``ccx_mlp_deep_q_actions``) and the six parameter gradients in three
(``ccx_mlp_deep_backward``), by CCX_MLP's rule with one more layer: a fixed sequence of f32 operations per row, f64 chains
over blocks of 256 rows, the same bits for any split of the rows into calls.

:class:`DeepMlpHead` is a class of its own for the reason ``wide.py`` gives: the stream-order table of the batch's classes
(tests/_stream_order.py) is closed, and this class brings its own proof (tests/test_gpu_stream_order_mlp_deep.py).  It
reaches the library only through the batch's ``_enqueue``."""

from __future__ import annotations

from dataclasses import dataclass

import numpy as np
import torch

from .learner import MLP_ACTIVATIONS, MLP_BACKWARDS, SampleResult, _require, _require_all, _require_out
from .qlearn import QActions, QLearning

_OPT = {"optional": True}
_NAMES = ("w1t", "b1", "w2t", "b2", "w3", "b3")


@dataclass
class DeepGradResult:
    """The parameter gradients of a :class:`DeepMlpHead` (:meth:`DeepMlpHead.param_grads`, include/ccx.h CCX_MLP_DEEP,
    backward): every element of every tensor is written, and every bit follows the written rule.  ``grad_a1`` / ``grad_a2``
    are the gradients at the pre-activations of the two hidden layers (``None`` unless asked for); ``workspace`` is the
    static buffer of :meth:`DeepMlpHead.alloc_param_grads` (else ``None``)."""

    w1t: torch.Tensor                         # f32 [L, H1]
    b1: torch.Tensor                          # f32 [H1]
    w2t: torch.Tensor                         # f32 [H1, H2]
    b2: torch.Tensor                          # f32 [H2]
    w3: torch.Tensor                          # f32 [O, H2]
    b3: torch.Tensor                          # f32 [O]
    grad_a1: torch.Tensor | None = None       # f32 [..., H1]
    grad_a2: torch.Tensor | None = None       # f32 [..., H2]
    workspace: torch.Tensor | None = None     # u8 [ccx_mlp_deep_backward_workspace_bytes(rows, L, H1, H2, O)]

    def grads(self) -> tuple:
        """The six gradients in the order of ``head.parameters()``."""
        return (self.w1t, self.b1, self.w2t, self.b2, self.w3, self.b3)


class DeepMlpHead(torch.nn.Module):
    """``Linear(L, H1) -> tanh | relu -> Linear(H1, H2) -> tanh | relu -> Linear(H2, O)`` on the batch's device:
    ``DeepMlpHead(batch, H1, H2, O=5, activation="tanh", L=None, backward="torch")``.

    The six parameters are stored in the kernel's layout -- ``w1t`` [L, H1] and ``w2t`` [H1, H2] INPUT-major
    (``Linear.weight.t()``), ``b1`` [H1], ``b2`` [H2], ``w3`` [O, H2] (torch's layout), ``b3`` [O] -- so
    ``DeviceAdam(batch, head.parameters())`` updates what the kernels read; ``state_dict()`` / ``load_state_dict()`` are
    ``nn.Module``'s.  They are initialised as three ``torch.nn.Linear`` layers drawn in order from torch's generator would be;
    :meth:`from_linear` / :meth:`to_sequential` convert by exact copies.  ``L`` defaults to the batch's ``obs_len``
    (1..512); ``H1`` and ``H2`` are multiples of 16 in 16..256 and need not be equal; ``O`` in 1..8.

    ``head(x, out=None, hidden1_out=None, hidden2_out=None)``: ``x`` f32 [..., L], contiguous, 16-byte aligned; returns f32
    [..., O].  The outputs of a row are a fixed sequence of f32 operations on that row: ``head(rows)`` on a minibatch of any
    shape reproduces, bit for bit, the logits :meth:`sample_actions` drew an action from.  ``out`` and the two ``hidden*_out``
    (f32 [..., H1] / [..., H2], 16-byte aligned) reuse tensors: with :meth:`param_grads` ``(out=)`` the static-buffer pair for
    a captured graph.  When grad mode is on and a parameter or ``x`` requires a gradient the call is a
    ``torch.autograd.Function``: the same kernel, the same bits, both hiddens saved; ``out=`` / ``hidden*_out=`` are refused;
    ``backward="torch"`` (the default) is the f32 torch composition (correct to rounding, NOT bit-defined), ``"device"`` is
    ``ccx_mlp_deep_backward`` (the six parameter gradients bit-defined; the gradient of ``x``, formed only when ``x``
    requires one, a torch product on ``grad_a1``).  Anything else than the tensors described raises ``ValueError`` before
    the library is called; zero rows return empty tensors without calling it.
    Only enqueues (no host synchronisation); stream order: :class:`~collectivecrossing_amd.learner.LearnerOps`.  Not here:
    more than two hidden layers, deep heads in ``SideHeads``, more than 8 outputs, a bit-defined gradient with respect to
    ``x``, MFMA, bf16 / f16, the vector and RLlib adapters."""

    def __init__(self, batch, H1: int, H2: int, O: int = 5, activation: str = "tanh", L: int | None = None, backward: str = "torch"):
        from .batched import BatchedCollectiveCrossing

        super().__init__()
        if not isinstance(batch, BatchedCollectiveCrossing):
            raise ValueError("batch must be a BatchedCollectiveCrossing")
        L = batch.obs_len if L is None else L
        for name, v, lo, hi in (("L", L, 1, 512), ("H1", H1, 16, 256), ("H2", H2, 16, 256), ("O", O, 1, 8)):
            if not isinstance(v, int) or isinstance(v, bool) or not lo <= v <= hi:
                raise ValueError(f"{name} must be an int in {lo}..{hi}, got {v!r}")
        if H1 % 16 or H2 % 16:
            raise ValueError(f"H1 and H2 must be multiples of 16, got {H1} and {H2}")
        if activation not in MLP_ACTIVATIONS:
            raise ValueError(f"activation must be one of {sorted(MLP_ACTIVATIONS)}, got {activation!r}")
        if backward not in MLP_BACKWARDS:
            raise ValueError(f"backward must be one of {list(MLP_BACKWARDS)}, got {backward!r}")
        self.backward = backward
        object.__setattr__(self, "batch", batch)                          # (not a submodule, not part of the state dict)
        self.L, self.H1, self.H2, self.O, self.activation = L, H1, H2, O, activation
        self.activation_id = MLP_ACTIVATIONS[activation]
        lin1, lin2, lin3 = torch.nn.Linear(L, H1), torch.nn.Linear(H1, H2), torch.nn.Linear(H2, O)
        dev = batch.device
        self.w1t = torch.nn.Parameter(lin1.weight.detach().t().contiguous().to(dev))
        self.b1 = torch.nn.Parameter(lin1.bias.detach().clone().to(dev))
        self.w2t = torch.nn.Parameter(lin2.weight.detach().t().contiguous().to(dev))
        self.b2 = torch.nn.Parameter(lin2.bias.detach().clone().to(dev))
        self.w3 = torch.nn.Parameter(lin3.weight.detach().clone().to(dev))
        self.b3 = torch.nn.Parameter(lin3.bias.detach().clone().to(dev))

    @classmethod
    def from_linear(cls, batch, lin1: torch.nn.Linear, lin2: torch.nn.Linear, lin3: torch.nn.Linear, activation: str = "tanh",
                    backward: str = "torch") -> "DeepMlpHead":
        """The head that computes ``lin3(act(lin2(act(lin1(x)))))``: exact copies of the three layers' f32 parameters."""
        lins = (lin1, lin2, lin3)
        if (any(not isinstance(m, torch.nn.Linear) or m.bias is None or m.weight.dtype is not torch.float32 for m in lins)
                or lin1.out_features != lin2.in_features or lin2.out_features != lin3.in_features):
            raise ValueError("from_linear needs three f32 torch.nn.Linear layers with biases whose sizes chain")
        head = cls(batch, lin1.out_features, lin2.out_features, lin3.out_features, activation, lin1.in_features, backward)
        with torch.no_grad():
            head.w1t.copy_(lin1.weight.t())
            head.b1.copy_(lin1.bias)
            head.w2t.copy_(lin2.weight.t())
            head.b2.copy_(lin2.bias)
            head.w3.copy_(lin3.weight)
            head.b3.copy_(lin3.bias)
        return head

    def to_sequential(self, dtype: torch.dtype = torch.float32) -> torch.nn.Sequential:
        """``Sequential(Linear(L, H1), act, Linear(H1, H2), act, Linear(H2, O))`` with exact copies of the parameters (cast
        to ``dtype``)."""
        dev = self.w1t.device
        lin1 = torch.nn.Linear(self.L, self.H1, device=dev, dtype=dtype)
        lin2 = torch.nn.Linear(self.H1, self.H2, device=dev, dtype=dtype)
        lin3 = torch.nn.Linear(self.H2, self.O, device=dev, dtype=dtype)
        with torch.no_grad():
            lin1.weight.copy_(self.w1t.t())
            lin1.bias.copy_(self.b1)
            lin2.weight.copy_(self.w2t.t())
            lin2.bias.copy_(self.b2)
            lin3.weight.copy_(self.w3)
            lin3.bias.copy_(self.b3)
        act = torch.nn.Tanh if self.activation == "tanh" else torch.nn.ReLU
        return torch.nn.Sequential(lin1, act(), lin2, act(), lin3)

    def extra_repr(self) -> str:
        return f"L={self.L}, H1={self.H1}, H2={self.H2}, O={self.O}, activation={self.activation}, backward={self.backward}"

    def _shapes(self) -> tuple:
        L, H1, H2, O = self.L, self.H1, self.H2, self.O
        return ((L, H1), (H1,), (H1, H2), (H2,), (O, H2), (O,))

    def _check_parameters(self) -> None:
        for name, shape in zip(_NAMES, self._shapes()):
            _require(name, getattr(self, name), torch.float32, shape, self.batch.device, verb="stay")

    def _params(self) -> tuple:
        return tuple(getattr(self, name) for name in _NAMES)

    # ------------------------------------------------------------------ the forward
    def _enqueue_forward(self, x, y, hidden1, hidden2) -> None:
        b = self.batch
        b._enqueue(b._lib.ccx_mlp_deep_forward, x.numel() // self.L, self.L, self.H1, self.H2, self.O, self.activation_id, x,
                   *self._params(), y, hidden1, hidden2)

    def forward(self, x: torch.Tensor, out: torch.Tensor | None = None, hidden1_out: torch.Tensor | None = None,
                hidden2_out: torch.Tensor | None = None) -> torch.Tensor:
        b = self.batch
        _require("x", x, torch.float32, (..., self.L), b.device, align=16)
        self._check_parameters()
        lead = tuple(x.shape[:-1])
        if torch.is_grad_enabled() and (x.requires_grad or any(p.requires_grad for p in self.parameters())):
            if out is not None or hidden1_out is not None or hidden2_out is not None:
                raise ValueError("out=, hidden1_out= and hidden2_out= cannot be used when a gradient is required (the autograd "
                                 "path allocates its outputs)")
            if x.numel() == 0:
                return x.new_zeros(lead + (self.O,)) + self.b3 * 0.0
            return _DeepForward.apply(self, x, *self._params())
        if out is None:
            out = b._new(lead + (self.O,), torch.float32)
        else:
            _require("out", out, torch.float32, lead + (self.O,), b.device)
        _require("hidden1_out", hidden1_out, torch.float32, lead + (self.H1,), b.device, optional=True, align=16)
        _require("hidden2_out", hidden2_out, torch.float32, lead + (self.H2,), b.device, optional=True, align=16)
        if x.numel():
            self._enqueue_forward(x.detach(), out, hidden1_out, hidden2_out)
        return out

    # ------------------------------------------------------------------ the parameter gradients
    def _workspace(self, rows: int, workspace):
        b = self.batch
        need = int(b._lib.ccx_mlp_deep_backward_workspace_bytes(int(rows), self.L, self.H1, self.H2, self.O))
        return b._workspace_arg(need, workspace, "alloc_param_grads")

    def _new_grads(self, lead, want_grad_a: bool, workspace) -> DeepGradResult:
        b, f = self.batch, torch.float32
        return DeepGradResult(*(b._new(shape, f) for shape in self._shapes()),
                              b._new(lead + (self.H1,), f) if want_grad_a else None,
                              b._new(lead + (self.H2,), f) if want_grad_a else None, workspace)

    def alloc_param_grads(self, shape, want_grad_a: bool = False) -> DeepGradResult:
        """Static buffers of :meth:`param_grads` for rows of the leading shape ``shape``: the six gradients, ``grad_a1`` and
        ``grad_a2`` if asked for, and the workspace (for a captured graph).  The workspace is
        ``ceil(rows / 256) * (L H1 + H1 + H1 H2 + H2 + O H2 + O) * 8`` bytes: 1.26 GB at 524 288 rows of a 256-256 head."""
        shape = tuple(int(v) for v in shape)
        rows = int(np.prod(shape)) if shape else 1
        return self._new_grads(shape, want_grad_a, self._workspace(max(rows, 1), None))

    def _param_grads(self, x, hidden1, hidden2, grad_y, w2t, w3, out: DeepGradResult) -> DeepGradResult:
        b, f = self.batch, torch.float32
        L, H1, H2, O = self.L, self.H1, self.H2, self.O
        lead = tuple(x.shape[:-1]) if isinstance(x, torch.Tensor) else ()
        _require_all(b.device, ("x", x, f, (..., L), {"align": 16}), ("hidden1", hidden1, f, lead + (H1,), {"align": 16}),
                     ("hidden2", hidden2, f, lead + (H2,), {"align": 16}), ("grad_y", grad_y, f, lead + (O,)),
                     ("w2t", w2t, f, (H1, H2)), ("w3", w3, f, (O, H2)),
                     *((f"out.{n}", getattr(out, n), f, s) for n, s in zip(_NAMES, self._shapes())),
                     ("out.grad_a1", out.grad_a1, f, lead + (H1,), {"optional": True, "align": 16}),
                     ("out.grad_a2", out.grad_a2, f, lead + (H2,), {"optional": True, "align": 16}))
        rows = x.numel() // L
        if rows == 0:
            for t in out.grads():
                t.zero_()
            return out
        workspace = self._workspace(rows, out.workspace)
        b._enqueue(b._lib.ccx_mlp_deep_backward, rows, L, H1, H2, O, self.activation_id, x.detach(), hidden1.detach(),
                   hidden2.detach(), grad_y.detach(), w2t.detach(), w3.detach(), workspace, *out.grads(), out.grad_a1, out.grad_a2)
        return out

    def param_grads(self, x: torch.Tensor, hidden1: torch.Tensor, hidden2: torch.Tensor, grad_y: torch.Tensor,
                    want_grad_a: bool = False, out: DeepGradResult | None = None,
                    workspace: torch.Tensor | None = None) -> DeepGradResult:
        """The gradients of the six parameter arrays from the gradient of the outputs, on the device
        (``ccx_mlp_deep_backward``, include/ccx.h CCX_MLP_DEEP): three kernels on the handle's stream, bit-defined -- f32 per
        row, then f64 chains over blocks of 256 rows and the fixed final step -- so the same rows give the same gradient bits
        on any machine, eager or captured.

        ``x`` f32 [..., L] (contiguous, 16-byte aligned), ``hidden1`` f32 [..., H1] and ``hidden2`` f32 [..., H2] (what the
        forward saved: ``head(x, hidden1_out=, hidden2_out=)``; 16-byte aligned), ``grad_y`` f32 [..., O].  ``want_grad_a``
        also returns the gradients at the pre-activations, f32 [..., H1] and [..., H2] (``grad_a1 @ w1t.t()`` is the gradient
        with respect to ``x``, which the library does not form).  ``out`` reuses a result of :meth:`alloc_param_grads` (its
        ``grad_a1`` / ``grad_a2`` and its workspace decide; ``want_grad_a`` and ``workspace`` are then ignored);
        ``workspace`` reuses a u8 tensor of at least ``ccx_mlp_deep_backward_workspace_bytes`` bytes, 8-byte aligned;
        otherwise it comes from torch's allocator, so the call captures.  A wrong dtype, shape or device, a non-contiguous
        tensor, a misaligned pointer or a workspace that is too small raises ``ValueError`` before the library is called;
        zero rows return zeros without calling it.
        Only enqueues (no host synchronisation); stream order: :class:`~collectivecrossing_amd.learner.LearnerOps`."""
        self._check_parameters()
        _require_out(out, DeepGradResult, "alloc_param_grads")
        if out is None:
            lead = tuple(x.shape[:-1]) if isinstance(x, torch.Tensor) else ()
            out = self._new_grads(lead, want_grad_a, workspace)
        return self._param_grads(x, hidden1, hidden2, grad_y, self.w2t, self.w3, out)

    # ------------------------------------------------------------------ observation rows to actions, one launch
    def _check_actor(self, who: str, outputs) -> None:
        b = self.batch
        if self.O not in outputs or self.L != b.obs_len:
            raise ValueError(f"{who} needs O in {tuple(outputs)} and L == obs_len == {b.obs_len}, got O = {self.O}, L = {self.L}")
        self._check_parameters()

    def sample_actions(self, obs: torch.Tensor, masks: torch.Tensor | None = None, deterministic: bool = False,
                       want_logp: bool = True, want_entropy: bool = False, logits_out: torch.Tensor | None = None,
                       out: SampleResult | None = None) -> SampleResult:
        """Observation rows to actions in ONE launch (``ccx_mlp_deep_sample_actions``): by definition
        ``batch.sample_actions(head(obs), ...)`` -- the same key, the same rule for terminated or truncated agents, the same
        bits in ``actions``, ``logp`` and ``entropy``.  Needs ``O == 5`` and ``L == obs_len``; ``obs`` f32 [E, N, L]
        (contiguous, 16-byte aligned); ``logits_out`` f32 [E, N, 5] receives the logits of every slot, dead ones included.
        ``masks``, ``deterministic``, ``want_*`` and ``out`` are ``sample_actions``'.  No gradient flows through this call.
        Only enqueues (no host synchronisation); stream order: :class:`~collectivecrossing_amd.learner.LearnerOps`."""
        b = self.batch
        E, N = b.num_envs, b.num_agents
        self._check_actor("sample_actions", (5,))
        _require_out(out, SampleResult, "alloc_sample")
        if out is None:
            out = b.alloc_sample(want_logp, want_entropy)
        _require_all(b.device, ("obs", obs, torch.float32, (E, N, b.obs_len), {"align": 16}), ("masks", masks, torch.uint8, (E, N), _OPT),
                     ("logits_out", logits_out, torch.float32, (E, N, 5), _OPT),
                     ("out.actions", out.actions, torch.uint8, (E, N)), ("out.logp", out.logp, torch.float32, (E, N), _OPT),
                     ("out.entropy", out.entropy, torch.float32, (E, N), _OPT))
        if obs.numel() == 0:
            return out
        b._enqueue(b._lib.ccx_mlp_deep_sample_actions, self.H1, self.H2, self.activation_id, obs.detach(), *self._params(), masks,
                   int(bool(deterministic)), out.actions, out.logp, out.entropy, logits_out)
        return out

    def q_actions(self, ql: QLearning, obs: torch.Tensor, masks: torch.Tensor | None = None, greedy: bool = False,
                  want_explored: bool = False, q_out: torch.Tensor | None = None, out: QActions | None = None) -> QActions:
        """Observation rows to epsilon-greedy actions in ONE launch (``ccx_mlp_deep_q_actions``): by definition
        ``ql.q_actions(head(obs), ...)`` for ``O == 5`` and ``ql.q_actions(ql.dueling(head(obs)), ...)`` for ``O == 6``, with
        ``ql``'s epsilon (read from its device scalar when the kernel runs).  ``q_out`` f32 [E, N, 5] receives the COMBINED
        Q-values of every slot.  ``masks``, ``greedy``, ``want_explored`` and ``out`` are ``QLearning.q_actions``'.  No
        gradient flows through this call.
        Only enqueues (no host synchronisation); stream order: :class:`~collectivecrossing_amd.learner.LearnerOps`."""
        b = self.batch
        if not isinstance(ql, QLearning) or ql.batch is not b:
            raise ValueError("ql must be a QLearning of this head's batch")
        self._check_actor("q_actions", (5, 6))
        E, N = b.num_envs, b.num_agents
        _require_out(out, QActions, "alloc_q_actions")
        if out is None:
            out = ql.alloc_q_actions(want_explored)
        _require_all(b.device, ("obs", obs, torch.float32, (E, N, b.obs_len), {"align": 16}), ("masks", masks, torch.uint8, (E, N), _OPT),
                     ("q_out", q_out, torch.float32, (E, N, 5), _OPT), ("out.actions", out.actions, torch.uint8, (E, N)),
                     ("out.explored", out.explored, torch.uint8, (E, N), _OPT))
        if obs.numel() == 0:
            return out
        b._enqueue(b._lib.ccx_mlp_deep_q_actions, self.H1, self.H2, self.activation_id, self.O, obs.detach(), *self._params(), masks,
                   None if greedy else ql.epsilon_dev, out.actions, out.explored, q_out)
        return out


class _DeepForward(torch.autograd.Function):
    """:class:`DeepMlpHead` when a gradient is required: the forward is the kernel of CCX_MLP_DEEP with both hiddens saved;
    the backward is ordinary f32 torch on them (``backward="torch"``: not bit-defined) or ``ccx_mlp_deep_backward``
    (``"device"``: the six parameter gradients bit-defined; the gradient of ``x``, where required, a torch product on its
    ``grad_a1``)."""

    @staticmethod
    def forward(ctx, head, x, w1t, b1, w2t, b2, w3, b3):
        x = x.detach()
        b = head.batch
        lead = tuple(x.shape[:-1])
        y = b._new(lead + (head.O,), torch.float32)
        hidden1 = b._new(lead + (head.H1,), torch.float32)
        hidden2 = b._new(lead + (head.H2,), torch.float32)
        head._enqueue_forward(x, y, hidden1, hidden2)
        ctx.head = head
        ctx.save_for_backward(x, w1t.detach(), w2t.detach(), w3.detach(), hidden1, hidden2)
        return y

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, gy):
        x, w1t, w2t, w3, hidden1, hidden2 = ctx.saved_tensors
        head = ctx.head
        L, H1, H2, O = head.L, head.H1, head.H2, head.O
        need = ctx.needs_input_grad
        gy = gy.contiguous()
        if head.backward == "device":
            out = head._new_grads(tuple(x.shape[:-1]), need[1], None)
            head._param_grads(x, hidden1, hidden2, gy, w2t, w3, out)
            gx = (out.grad_a1.reshape(-1, H1) @ w1t.t()).reshape(x.shape) if need[1] else None
            return (None, gx) + tuple(g if n else None for g, n in zip(out.grads(), need[2:]))
        relu = head.activation == "relu"
        gy2, h1, h2, x2 = gy.reshape(-1, O), hidden1.reshape(-1, H1), hidden2.reshape(-1, H2), x.reshape(-1, L)
        gh2 = gy2 @ w3
        ga2 = gh2 * (h2 > 0) if relu else gh2 * (1.0 - h2 * h2)
        gh1 = ga2 @ w2t.t()
        ga1 = gh1 * (h1 > 0) if relu else gh1 * (1.0 - h1 * h1)
        gx = (ga1 @ w1t.t()).reshape(x.shape) if need[1] else None
        return (None, gx, x2.t() @ ga1 if need[2] else None, ga1.sum(0) if need[3] else None, h1.t() @ ga2 if need[4] else None,
                ga2.sum(0) if need[5] else None, gy2.t() @ h2 if need[6] else None, gy2.sum(0) if need[7] else None)
