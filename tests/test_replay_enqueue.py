"""replay.py reaches the library through ``_enqueue`` only (the walk of tests/test_stream_order_table.py's third test, on the
new module): a library function is named only as the first argument of ``_enqueue(``, which orders every tensor it passes
-- the ring's own arrays included, since they travel as arguments.  And the public surface: the lazy exports, the ABI table.
No GPU."""

import inspect
import re
from pathlib import Path

import collectivecrossing_amd
from collectivecrossing_amd import _abi


def test_replay_reaches_the_library_through_enqueue_only():
    named = re.compile(r"_lib\.(ccx_\w+)")
    enqueued = re.compile(r"\b_enqueue\(\s*\w+\._lib\.(ccx_\w+)\s*[,)]")
    text = (Path(collectivecrossing_amd.__file__).parent / "replay.py").read_text()
    ok = {m.start(1) for m in enqueued.finditer(text)}
    stray = [m.group(1) for m in named.finditer(text) if m.start(1) not in ok]
    assert not stray, f"replay.py: {stray} must go through _enqueue"
    assert sorted(m.group(1) for m in enqueued.finditer(text)) == ["ccx_replay_fetch", "ccx_replay_push", "ccx_replay_sample"]


def test_the_ring_travels_as_arguments():
    """Every ``_enqueue`` of replay.py passes ``*self._ring_args()``, and that is the seven arrays and the state."""
    from collectivecrossing_amd.replay import _ARRAYS, ReplayRing

    text = inspect.getsource(ReplayRing)
    calls = re.findall(r"_enqueue\(\s*\w+\._lib\.ccx_\w+,\s*([^,]+),", text)
    assert len(calls) == 3 and all(c.strip() == "*self._ring_args()" for c in calls), calls
    assert "also=" not in text
    assert _ARRAYS == ("obs_c", "next_c", "actions", "reward", "done", "valid", "masks_next")
    src = inspect.getsource(ReplayRing._ring_args)
    assert "self._arrays()" in src and "self.state" in src and "self.steps" in src


def test_exports_and_prototypes():
    from collectivecrossing_amd import ReplayBatch, ReplayRing
    from collectivecrossing_amd.replay import ReplayBatch as RB
    from collectivecrossing_amd.replay import ReplayRing as RR

    assert ReplayRing is RR and ReplayBatch is RB
    assert {"ReplayRing", "ReplayBatch"} <= set(collectivecrossing_amd.__all__)
    for name, pointers in (("ccx_replay_push", 16), ("ccx_replay_sample", 16), ("ccx_replay_fetch", 17)):
        restype, args = _abi.PROTOTYPES[name]
        assert len(args) == 1 + 1 + 8 + 1 + (pointers - 8), name             # handle, S, the ring, K or B, the call's arrays
    assert [f for f in ReplayBatch.__dataclass_fields__] == ["obs", "next_obs", "actions", "reward", "done", "valid", "masks_next",
                                                             "index"]
