"""The stream-order contract of every enqueueing method, on the GPU: each case of the table in
tests/_stream_order.py with torch's current stream another one than the handle's, in both directions, against the same call
on a twin batch with the handle's stream current throughout -- bit patterns; the negative control: with the two ordering
helpers switched off the harness does observe the difference, so it can fail."""

import numpy as np
import pytest
import _stream_order as so

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def rig():
    import torch

    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    main, other = torch.cuda.Stream(), torch.cuda.Stream()
    blocker = so.Blocker()
    blocker.warm(main, other)
    yield main, other, blocker
    torch.cuda.synchronize()


def _play(case, direction, rig, block=True):
    main, other, blocker = rig
    return so.run(case, direction, main, other, blocker, block=block, seed=so.seed_of(case, direction))


def _names(case, n):
    return [f"{case.name} output {i}" for i in range(n)]


@pytest.mark.parametrize("direction", ["before", "after"])
@pytest.mark.parametrize("case", so.CASES, ids=lambda c: c.name)
def test_order(case, direction, rig):
    want = _play(case, direction, rig, block=False)                      # the twin: the handle's stream is current
    got = _play(case, direction, rig)
    print(f"{case.name} {direction}: host {got.host_ms:.3f} ms, {len(got.got)} outputs, {sum(map(len, got.got))} bytes")
    assert got.open, "blocker too short: it had ended before the last piece was enqueued, the run proves nothing"
    assert len(got.got) == len(want.got) and got.got
    for name, g, w in zip(_names(case, len(got.got)), got.got, want.got):
        np.testing.assert_array_equal(g, w, err_msg=f"{name} ({direction}): "
                                      + ("the launch did not wait for its inputs" if direction == "before"
                                         else "the consumer did not wait for the launch"))
    if direction == "before":                                            # write after read: the snapshot holds the old bytes
        assert len(got.snaps) == len(got.pre)
        for name, s, p in zip(_names(case, len(got.snaps)), got.snaps, got.pre):
            np.testing.assert_array_equal(s, p, err_msg=f"{name}: overwritten while the current stream still read it")
    assert any(so.differs([g], [p]) for g, p in zip(want.got, want.pre)) or not want.pre, "the call changed no output"


@pytest.mark.parametrize("name", ["rollout", "ppo_loss_out"])
def test_negative_control(name, rig, monkeypatch):
    """With both helpers doing nothing the harness sees a stale result and an overwritten snapshot (before) and the
    prefill in the clones (after).  Every access stays inside buffers the case owns."""
    from collectivecrossing_amd.batched import BatchedCollectiveCrossing
    from collectivecrossing_amd.learner import LearnerOps

    case = next(c for c in so.CASES if c.name == name)
    want = {d: _play(case, d, rig, block=False) for d in ("before", "after")}
    monkeypatch.setattr(BatchedCollectiveCrossing, "_order_after_current_stream", lambda self, *a, **k: None)
    monkeypatch.setattr(LearnerOps, "_current_stream_waits", lambda self, *a, **k: None)
    before, after = _play(case, "before", rig), _play(case, "after", rig)
    assert before.open and after.open, "blocker too short"
    assert so.differs(before.got, want["before"].got), "before: the unordered launch was not seen to read the stale inputs"
    assert so.differs(before.snaps, before.pre), "before: the unordered launch was not seen to overwrite the outputs"
    assert so.differs(after.got, want["after"].got), "after: the unordered consumer was not seen to run early"
    # the clones of the outputs that existed before the call hold the prefill
    n = len(after.pre)
    assert n and not so.differs(after.got[:n], after.pre), "after: the early clones do not hold the prefill"
