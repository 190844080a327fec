"""The one tensor contract of the learner ops (``collectivecrossing_amd.learner._require`` and its helpers) on CPU tensors:
every kind of refusal with its full message.  The expected texts are written out literally, as the methods raised them
when each held its own copy of the check; nothing here is computed by the code under test.  Needs no library build."""

import sys
from pathlib import Path

import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))

from collectivecrossing_amd.learner import (EvalResult, GaeResult, PpoLossResult, SampleResult, _require,  # noqa: E402
                                            _require_all, _require_out)

CPU, META = torch.device("cpu"), torch.device("meta")
F32, F64, U8 = torch.float32, torch.float64, torch.uint8


def _refused(text, *args, **kw):
    with pytest.raises(ValueError) as e:
        _require(*args, **kw)
    assert str(e.value) == text


def _misaligned(shape, dtype=F32):
    """A contiguous tensor whose data_ptr is 4 past a multiple of 16."""
    n = 1
    for d in shape:
        n *= d
    base = torch.zeros(n + 8, dtype=dtype)
    assert base.data_ptr() % 16 == 0
    t = base[1:1 + n].reshape(shape)
    assert t.is_contiguous() and t.data_ptr() % 16 == 4
    return t


def test_a_good_tensor_passes_and_none_only_where_optional():
    _require("logits", torch.zeros(3, 4, 5), F32, (3, 4, 5), CPU, align=16)
    _require("masks", None, U8, (3, 4), CPU, optional=True)
    _require("masks", None, U8, (3, 4), CPU, optional=True, align=16)
    _refused("values must be a contiguous torch.float32 tensor of shape (2, 3, 4) on cpu", "values", None, F32, (2, 3, 4), CPU)


def test_fixed_shape_refusals():
    text = "reward must be a contiguous torch.float64 tensor of shape (2, 3, 4) on cpu"
    good = torch.zeros(2, 3, 4, dtype=F64)
    _require("reward", good, F64, (2, 3, 4), CPU)
    _refused(text, "reward", good.numpy(), F64, (2, 3, 4), CPU)                          # not a tensor
    _refused(text, "reward", good.float(), F64, (2, 3, 4), CPU)                          # dtype
    _refused(text, "reward", torch.zeros(2, 3, 5, dtype=F64), F64, (2, 3, 4), CPU)       # shape
    _refused(text, "reward", torch.zeros(4, 3, 2, dtype=F64).permute(2, 1, 0), F64, (2, 3, 4), CPU)   # strides
    _refused(text, "reward", torch.zeros(2, 3, 4, dtype=F64, device=META), F64, (2, 3, 4), CPU)       # device
    _refused("reward must be a contiguous torch.float64 tensor of shape (2, 3, 4) on cuda:1", "reward", good, F64, (2, 3, 4),
             torch.device("cuda", 1))
    # a torch.Size is accepted for the shape and printed as a tuple (masked_moments' valid against x.shape)
    _refused("valid must be a contiguous torch.uint8 tensor of shape (2, 3, 4) on cpu", "valid", good, U8, good.shape, CPU,
             optional=True)
    _refused("out.stats must be a contiguous torch.float32 tensor of shape (8,) on cpu", "out.stats", torch.zeros(4), F32, (8,), CPU)


def test_any_leading_shape():
    text = "logits must be a contiguous torch.float32 tensor of shape [..., 5] on cpu"
    for lead in ((), (0,), (7,), (2, 3)):
        _require("logits", torch.zeros(lead + (5,)), F32, (..., 5), CPU, align=16)
    _refused(text, "logits", [[0.0] * 5], F32, (..., 5), CPU)
    _refused(text, "logits", torch.zeros(3, 5, dtype=torch.float16), F32, (..., 5), CPU)
    _refused(text, "logits", torch.zeros(3, 4), F32, (..., 5), CPU)
    _refused(text, "logits", torch.zeros(()), F32, (..., 5), CPU)                        # 0-dim
    _refused(text, "logits", torch.zeros(3, 10)[:, ::2], F32, (..., 5), CPU)
    _refused(text, "logits", torch.zeros(3, 5, device=META), F32, (..., 5), CPU)
    _refused(text, "logits", None, F32, (..., 5), CPU)
    _refused("x must be a contiguous torch.float32 tensor of shape [..., 38] on cpu", "x", torch.zeros(2, 37), F32, (..., 38), CPU,
             align=16)


def test_any_shape():
    text = "x must be a contiguous torch.float32 tensor on cpu"
    _require("x", torch.zeros(3, 2, 7), F32, None, CPU)
    _require("x", torch.zeros(()), F32, None, CPU)
    _refused(text, "x", 1.0, F32, None, CPU)
    _refused(text, "x", torch.zeros(3, dtype=F64), F32, None, CPU)
    _refused(text, "x", torch.zeros(3, 4).t(), F32, None, CPU)
    _refused(text, "x", torch.zeros(3, device=META), F32, None, CPU)
    _refused(text, "x", None, F32, None, CPU)


def test_hint_and_verb():
    _refused("actions must be a contiguous torch.uint8 tensor of shape (3, 4) on cpu (cast stored actions to torch.uint8 first)",
             "actions", torch.zeros(3, 4, dtype=torch.int64), U8, (3, 4), CPU, hint=" (cast stored actions to torch.uint8 first)")
    text = "w1t must stay a contiguous torch.float32 tensor of shape (38, 64) on cpu"
    _require("w1t", torch.nn.Parameter(torch.zeros(38, 64)), F32, (38, 64), CPU, verb="stay")
    _refused(text, "w1t", torch.nn.Parameter(torch.zeros(64, 38)), F32, (38, 64), CPU, verb="stay")
    _refused(text, "w1t", torch.zeros(64, 38).t(), F32, (38, 64), CPU, verb="stay")
    _refused(text, "w1t", torch.zeros(38, 64, dtype=F64), F32, (38, 64), CPU, verb="stay")
    _refused(text, "w1t", torch.zeros(38, 64, device=META), F32, (38, 64), CPU, verb="stay")


def test_alignment_comes_last():
    t = _misaligned((3, 4, 5))
    _require("logits", t, F32, (3, 4, 5), CPU)
    _require("logits", t, F32, (3, 4, 5), CPU, align=4)
    for name in ("logits", "obs", "out", "grad_logits", "x"):
        _refused(f"{name} must be 16-byte aligned (a view at an odd offset of its storage is not)", name, t, F32, (..., 5), CPU,
                 align=16)
    # a tensor that is wrong otherwise is refused for that, whatever its address
    _refused("logits must be a contiguous torch.float32 tensor of shape (3, 4, 6) on cpu", "logits", t, F32, (3, 4, 6), CPU, align=16)


def test_a_table_is_checked_in_order_and_aligned_afterwards():
    good, odd = torch.zeros(2, 3, 5), _misaligned((2, 3, 5))
    masks = torch.zeros(2, 3, dtype=U8)
    opt = {"optional": True}
    _require_all(CPU, ("logits", good, F32, (2, 3, 5), {"align": 16}), ("masks", None, U8, (2, 3), opt),
                 ("out.actions", masks, U8, (2, 3)))
    with pytest.raises(ValueError) as e:                                 # the first bad row speaks
        _require_all(CPU, ("logits", good, F32, (2, 3, 5), {"align": 16}), ("masks", masks.long(), U8, (2, 3), opt),
                     ("out.actions", None, U8, (2, 3)))
    assert str(e.value) == "masks must be a contiguous torch.uint8 tensor of shape (2, 3) on cpu"
    with pytest.raises(ValueError) as e:                                 # a misaligned first row waits for the later rows
        _require_all(CPU, ("logits", odd, F32, (2, 3, 5), {"align": 16}), ("masks", masks, U8, (2, 3), opt),
                     ("out.actions", None, U8, (2, 3)))
    assert str(e.value) == "out.actions must be a contiguous torch.uint8 tensor of shape (2, 3) on cpu"
    with pytest.raises(ValueError) as e:
        _require_all(CPU, ("logits", odd, F32, (..., 5), {"align": 16}),
                     ("actions", masks, U8, (2, 3), {"hint": " (cast stored actions to torch.uint8 first)"}),
                     ("out", odd, F32, (2, 3, 5), {"align": 16}))
    assert str(e.value) == "logits must be 16-byte aligned (a view at an odd offset of its storage is not)"
    with pytest.raises(ValueError) as e:
        _require_all(CPU, ("grad_logits", None, F32, (2, 3, 5), {"optional": True, "align": 16}),
                     ("out", odd, F32, (2, 3, 5), {"align": 16}))
    assert str(e.value) == "out must be 16-byte aligned (a view at an odd offset of its storage is not)"


def test_out_is_none_or_the_result_class():
    z = torch.zeros(1)
    for cls, alloc, text in ((GaeResult, "alloc_gae", "out must be a GaeResult (alloc_gae)"),
                             (SampleResult, "alloc_sample", "out must be a SampleResult (alloc_sample)"),
                             (EvalResult, "alloc_evaluate", "out must be an EvalResult (alloc_evaluate)"),
                             (PpoLossResult, "alloc_ppo_loss", "out must be a PpoLossResult (alloc_ppo_loss)")):
        _require_out(None, cls, alloc)
        for bad in (z, (z, z), 0):
            with pytest.raises(ValueError) as e:
                _require_out(bad, cls, alloc)
            assert str(e.value) == text
    _require_out(GaeResult(z, z, None), GaeResult, "alloc_gae")
    _require_out(EvalResult(z, None), EvalResult, "alloc_evaluate")
    with pytest.raises(ValueError):
        _require_out(EvalResult(z, None), SampleResult, "alloc_sample")
