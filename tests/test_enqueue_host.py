"""``LearnerOps._enqueue`` on the host (needs no GPU): what is handed to the library is what gets ordered, and a call that
has an entry cannot lack its exit.  A stub batch with fake streams that log their waits stands in for the
device; the two helpers are the package's own."""

import ctypes as C

import pytest
import torch

from collectivecrossing_amd import _lib
from collectivecrossing_amd.batched import BatchedCollectiveCrossing
from collectivecrossing_amd.learner import LearnerOps


class FakeStream:
    def __init__(self, name, log):
        self.name, self.log = name, log

    def wait_stream(self, other):
        self.log.append(f"{self.name} waits for {other.name}")


class Stub(LearnerOps):
    _order_after_current_stream = BatchedCollectiveCrossing._order_after_current_stream

    def __init__(self, other_current: bool, status: int = 0):
        self.log = []
        self._h = object()
        self._stream = FakeStream("handle", self.log)
        self._current = FakeStream("current", self.log) if other_current else None
        self.status = status

    def _other_stream(self):
        return self._current

    def fn(self, *args):
        self.log.append("call")
        self.got = args
        return self.status


def _args():
    x, y, w = torch.zeros(3), torch.zeros(2, dtype=torch.uint8), torch.nn.Parameter(torch.zeros(4))
    table = (C.c_int64 * 2)(5, 6)
    return (7, x, None, 0.25, table, y, w), (x, y, w), table


def test_the_library_sees_the_handle_then_pointers_and_the_rest_in_place():
    b = Stub(other_current=False)
    args, (x, y, w), table = _args()
    assert b._enqueue(b.fn, *args) is None
    assert b.got[0] is b._h
    assert b.got[1:] == (7, x.data_ptr(), None, 0.25, table, y.data_ptr(), w.data_ptr())
    assert b.got[5] is table and type(b.got[2]) is int and type(b.got[4]) is float


def test_another_stream_current_entry_call_exit():
    b = Stub(other_current=True)
    b._enqueue(b.fn, *_args()[0])
    assert b.log == ["handle waits for current", "call", "current waits for handle"]


def test_same_stream_no_wait():
    b = Stub(other_current=False)
    b._enqueue(b.fn, *_args()[0])
    assert b.log == ["call"]


def test_a_failed_call_raises_through_check_and_has_no_exit(monkeypatch):
    class Lib:
        @staticmethod
        def ccx_last_error():
            return b"the stub said no"

    monkeypatch.setattr(_lib, "load", lambda: Lib)
    b = Stub(other_current=True, status=3)
    with pytest.raises(_lib.CcxError, match="the stub said no") as e:
        b._enqueue(b.fn, *_args()[0])
    assert e.value.status == 3
    assert b.log == ["handle waits for current", "call"]


def test_what_is_passed_is_what_is_ordered(monkeypatch):
    seen = []
    inner = Stub._order_after_current_stream

    def spy(self, *tensors, **kw):
        seen.append(tensors)
        return inner(self, *tensors, **kw)

    monkeypatch.setattr(Stub, "_order_after_current_stream", spy)
    b = Stub(other_current=True)
    args, tensors, _ = _args()
    p, g = torch.zeros(5), torch.zeros(5)
    b._enqueue(b.fn, *args, also=[p, g])
    (got,) = seen
    assert len(got) == 5 and all(a is t for a, t in zip(got, (*tensors, p, g)))
    assert p.data_ptr() not in b.got and g.data_ptr() not in b.got      # (their pointers travel in a table, not as arguments)


def test_switching_the_two_helpers_off_switches_the_order_off(monkeypatch):
    """What the negative controls of the GPU suites rely on."""
    monkeypatch.setattr(Stub, "_order_after_current_stream", lambda self, *a, **k: None)
    monkeypatch.setattr(LearnerOps, "_current_stream_waits", lambda self, *a, **k: None)
    b = Stub(other_current=True)
    b._enqueue(b.fn, *_args()[0])
    assert b.log == ["call"]
