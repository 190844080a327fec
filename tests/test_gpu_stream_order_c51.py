"""The stream-order contract of every enqueueing method of ``CategoricalQ``, with the harness of
tests/_stream_order.py (imported, not edited; its table stays the table of the batch's own classes): ``q_values(out=)``,
``loss(out=)``, ``loss_backward(out=)`` and the autograd path, each with torch's current stream another one than the handle's,
in both directions, against the same call on a twin batch with the handle's stream current throughout -- bit patterns; and the
negative control: with the two ordering helpers switched off the harness does see the difference."""

import numpy as np
import pytest
import _stream_order as so
from _stream_order import E, N, Plan, fill_bytes, inp, normal

pytestmark = pytest.mark.gpu

LEAD = (4, E, N)                                 # leading shape of the cases: 2048 rows, eight blocks of the tree
A = 51


def _loss_inputs(rng):
    """The ten arrays of a loss call as (stale buffer, real value) pairs; the stale actions are 255 (no row counts)."""
    rows = int(np.prod(LEAD))
    acts = rng.integers(0, 5, size=LEAD).astype(np.uint8)
    acts.reshape(-1)[rng.random(rows) < 0.1] = 255
    return dict(logits=inp(normal(rng, *LEAD, 5, A)), actions=inp(acts, 255), reward=inp(rng.standard_normal(LEAD)),
                done=inp((rng.random(LEAD) < 0.2).astype(np.uint8), 1), next_target=inp(normal(rng, *LEAD, 5, A)),
                next_online=inp(normal(rng, *LEAD, 5, A)), masks_next=inp(rng.integers(0, 32, size=LEAD).astype(np.uint8), 0x10),
                valid=inp((rng.random(LEAD) < 0.8).astype(np.uint8)), weights=inp(rng.uniform(0.5, 1.5, LEAD).astype(np.float32)),
                discount=inp(rng.uniform(0.9, 1.0, LEAD).astype(np.float32)))


def _q_values(w, rng):
    import torch
    from collectivecrossing_amd import CategoricalQ

    cq = CategoricalQ(w.batch, atoms=A)
    logits = inp(normal(rng, *LEAD, 5, A))
    out = torch.empty(LEAD + (5,), device="cuda")
    fill_bytes(out)
    return Plan([logits], lambda: [cq.q_values(logits[0], out=out)], [out])


def _loss(w, rng):
    from collectivecrossing_amd import CategoricalQ

    cq = CategoricalQ(w.batch, atoms=A)
    d = _loss_inputs(rng)
    out = cq.alloc_loss(LEAD, want_row_loss=True)
    fill_bytes(out.stats, out.row_loss, out.proj)

    def call():
        r = cq.loss(*(d[k][0] for k in list(d)[:9]), discount=d["discount"][0], out=out)
        return [r.stats, r.row_loss, r.proj]
    return Plan(list(d.values()), call, [out.stats, out.row_loss, out.proj])


def _backward(w, rng):
    import torch
    from collectivecrossing_amd import CategoricalQ

    cq = CategoricalQ(w.batch, atoms=A)
    d = _loss_inputs(rng)
    real = cq.loss(*(d[k][1] for k in list(d)[:9]), discount=d["discount"][1])
    stats, proj = inp(real.stats, torch.zeros_like(real.stats)), inp(real.proj)
    gloss = inp(np.array([-1.75], np.float32), 1.0)
    out = cq.alloc_loss(LEAD)
    fill_bytes(out.grad_logits)
    ins = [d[k] for k in ("logits", "actions", "valid", "weights")] + [stats, proj, gloss]
    return Plan(ins, lambda: [cq.loss_backward(d["logits"][0], d["actions"][0], proj[0], d["valid"][0], d["weights"][0], stats=stats[0],
                                               grad_loss=gloss[0], out=out)], [out.grad_logits])


def _autograd(w, rng):
    import torch
    from collectivecrossing_amd import CategoricalQ

    cq = CategoricalQ(w.batch, atoms=A)
    d = _loss_inputs(rng)

    def call():
        with torch.enable_grad():
            x = d["logits"][0].detach().requires_grad_()
            r = cq.loss(x, *(d[k][0] for k in list(d)[1:9]), discount=d["discount"][0], want_row_loss=True)
            (r.loss * 3.0).backward()
        return [r.stats, r.row_loss, r.proj, x.grad]
    return Plan(list(d.values()), call)


CASES = [so.Case("c51_q_values", "sim", ("CategoricalQ.q_values",), _q_values),
         so.Case("c51_loss_out", "sim", ("CategoricalQ.loss",), _loss),
         so.Case("c51_loss_backward_out", "sim", ("CategoricalQ.loss_backward",), _backward),
         so.Case("c51_loss_autograd", "sim", ("CategoricalQ.loss",), _autograd)]


@pytest.fixture(scope="module")
def rig():
    import torch

    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    main, blocker = torch.cuda.Stream(), so.Blocker()
    for _ in range(8):                                                   # (torch hands out pool streams round robin)
        other = torch.cuda.Stream()
        blocker.warm(main, other)
        if _run_side_by_side(main, other, blocker):
            break
    else:
        pytest.fail("no pair of streams that the device runs side by side: the harness could observe nothing")
    yield main, other, blocker
    torch.cuda.synchronize()


def _run_side_by_side(main, other, blocker) -> bool:
    """Does work on ``main`` finish while the blocker keeps ``other`` busy?  Streams outnumber the hardware queues of a
    process; two streams that share a queue run one after the other whatever the library does, and the negative control
    (like every ``before`` / ``after`` run) would then see an order that nobody made."""
    import torch

    busy = blocker.run(other)
    with torch.cuda.stream(main):
        torch.zeros(1, device="cuda")
        done = torch.cuda.Event()
        done.record(main)
    done.synchronize()
    apart = not busy.query()
    torch.cuda.synchronize()
    return apart


def _play(case, direction, rig, block=True):
    main, other, blocker = rig
    seed = 960_000 + 1000 * CASES.index(case) + (direction == "after")   # (beyond every seed of the harness's own table)
    return so.run(case, direction, main, other, blocker, block=block, seed=seed)


@pytest.mark.parametrize("direction", ["before", "after"])
@pytest.mark.parametrize("case", CASES, ids=lambda c: c.name)
def test_order(case, direction, rig):
    want = _play(case, direction, rig, block=False)                      # the twin: the handle's stream is current
    got = _play(case, direction, rig)
    print(f"{case.name} {direction}: host {got.host_ms:.3f} ms, {len(got.got)} outputs, {sum(map(len, got.got))} bytes")
    assert got.open, "blocker too short: it had ended before the last piece was enqueued, the run proves nothing"
    assert len(got.got) == len(want.got) and got.got
    for i, (g, w) in enumerate(zip(got.got, want.got)):
        np.testing.assert_array_equal(g, w, err_msg=f"{case.name} output {i} ({direction}): "
                                      + ("the launch did not wait for its inputs" if direction == "before"
                                         else "the consumer did not wait for the launch"))
    if direction == "before":                                            # write after read: the snapshot holds the old bytes
        assert len(got.snaps) == len(got.pre)
        for i, (s, p) in enumerate(zip(got.snaps, got.pre)):
            np.testing.assert_array_equal(s, p, err_msg=f"{case.name} output {i}: overwritten while the current stream still read it")
    assert any(so.differs([g], [p]) for g, p in zip(want.got, want.pre)) or not want.pre, "the call changed no output"


@pytest.mark.parametrize("name", ["c51_q_values", "c51_loss_out"])
def test_negative_control(name, rig, monkeypatch):
    """With both helpers doing nothing the harness sees a stale result and an overwritten snapshot (before) and the prefill
    in the clones (after).  Every access stays inside buffers the case owns."""
    from collectivecrossing_amd.batched import BatchedCollectiveCrossing
    from collectivecrossing_amd.learner import LearnerOps

    case = next(c for c in CASES if c.name == name)
    want = {d: _play(case, d, rig, block=False) for d in ("before", "after")}
    monkeypatch.setattr(BatchedCollectiveCrossing, "_order_after_current_stream", lambda self, *a, **k: None)
    monkeypatch.setattr(LearnerOps, "_current_stream_waits", lambda self, *a, **k: None)
    before, after = _play(case, "before", rig), _play(case, "after", rig)
    assert before.open and after.open, "blocker too short"
    assert so.differs(before.got, want["before"].got), "before: the unordered launch was not seen to read the stale inputs"
    assert so.differs(before.snaps, before.pre), "before: the unordered launch was not seen to overwrite the outputs"
    assert so.differs(after.got, want["after"].got), "after: the unordered consumer was not seen to run early"


def test_the_harness_table_is_unchanged():
    """This file adds nothing to the table tests/test_stream_order_table.py walks."""
    assert not any(c.name.startswith("c51_") for c in so.CASES)
