"""The stream-order contract of every enqueueing method of ``QLearning``, with the harness of
tests/_stream_order.py (imported, not edited; its table stays the table of the batch's own classes): ``q_actions``,
``td_loss(out=)``, ``td_loss_backward(out=)`` and the autograd path, each with torch's current stream another one than the
handle's, in both directions, against the same call on a twin batch with the handle's stream current throughout -- bit
patterns; and the negative control: with the two ordering helpers switched off the harness does see the difference."""

import numpy as np
import pytest
import _stream_order as so
from _stream_order import E, N, Plan, fill_bytes, inp, normal

pytestmark = pytest.mark.gpu

LEAD = (4, E, N)                                 # leading shape of the learner-side cases: 2048 rows, eight blocks of the tree


def _td_inputs(rng):
    """The nine arrays of a TD-loss call as (stale buffer, real value) pairs; the stale actions are 255 (no row counts)."""
    rows = int(np.prod(LEAD))
    acts = rng.integers(0, 5, size=LEAD).astype(np.uint8)
    acts.reshape(-1)[rng.random(rows) < 0.1] = 255
    return dict(q=inp(normal(rng, *LEAD, 5)), actions=inp(acts, 255), reward=inp(rng.standard_normal(LEAD)),
                done=inp((rng.random(LEAD) < 0.2).astype(np.uint8), 1), q_next_target=inp(normal(rng, *LEAD, 5)),
                q_next_online=inp(normal(rng, *LEAD, 5)), masks_next=inp(rng.integers(0, 32, size=LEAD).astype(np.uint8), 0x10),
                valid=inp((rng.random(LEAD) < 0.8).astype(np.uint8)), weights=inp(rng.uniform(0.5, 1.5, LEAD).astype(np.float32)))


def _q_actions(w, rng):
    import torch
    from collectivecrossing_amd import QLearning

    b = w.batch
    ql = QLearning(b, epsilon=0.5)
    q, masks = inp(normal(rng, E, N, 5)), inp(b.action_masks(), 0x10)
    eps = (ql.epsilon_dev, torch.full((1,), 0.5, device="cuda"))
    ql.epsilon_dev.fill_(0.0)                                            # the stale rate: nothing explores
    out = ql.alloc_q_actions(want_explored=True)
    fill_bytes(out.actions, out.explored)

    def sanity(got):
        acts, expl = got[0].reshape(E, N), got[1].reshape(E, N)
        assert (acts < 4).any() and (acts[acts != 255] <= 4).all() and expl.any() and not expl.all()
    return Plan([q, masks, eps], lambda: so.tensors(ql.q_actions(q[0], masks[0], out=out)), [out.actions, out.explored], sanity)


def _td_loss(w, rng):
    from collectivecrossing_amd import QLearning

    ql = QLearning(w.batch)
    d = _td_inputs(rng)
    out = ql.alloc_td_loss(LEAD, want_td_error=True)
    fill_bytes(out.stats, out.td_error)

    def call():
        r = ql.td_loss(*(d[k][0] for k in d), gamma=0.97, out=out)
        return [r.stats, r.td_error]
    return Plan(list(d.values()), call, [out.stats, out.td_error])


def _td_backward(w, rng):
    import torch
    from collectivecrossing_amd import QLearning

    ql = QLearning(w.batch)
    d = _td_inputs(rng)
    real = ql.td_loss(*(d[k][1] for k in d), gamma=0.97).stats
    stats, gloss = inp(real, torch.zeros_like(real)), inp(np.array([-1.75], np.float32), 1.0)
    out = ql.alloc_td_loss(LEAD)
    fill_bytes(out.grad_q)
    return Plan(list(d.values()) + [stats, gloss],
                lambda: [ql.td_loss_backward(*(d[k][0] for k in d), gamma=0.97, stats=stats[0], grad_loss=gloss[0], out=out)],
                [out.grad_q])


def _autograd(w, rng):
    import torch
    from collectivecrossing_amd import QLearning

    ql = QLearning(w.batch)
    d = _td_inputs(rng)

    def call():
        with torch.enable_grad():
            q = d["q"][0].detach().requires_grad_()
            r = ql.td_loss(q, *(d[k][0] for k in list(d)[1:]), gamma=0.97, want_td_error=True)
            (r.loss * 3.0).backward()
        return [r.stats, r.td_error, q.grad]
    return Plan(list(d.values()), call)


CASES = [so.Case("qlearn_q_actions", "sim", ("QLearning.q_actions",), _q_actions),
         so.Case("qlearn_td_loss_out", "sim", ("QLearning.td_loss",), _td_loss),
         so.Case("qlearn_td_loss_backward_out", "sim", ("QLearning.td_loss_backward",), _td_backward),
         so.Case("qlearn_td_loss_autograd", "sim", ("QLearning.td_loss",), _autograd)]


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
    seed = 950_000 + 1000 * CASES.index(case) + (direction == "after")   # (beyond every seed of the harness's own table)
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


@pytest.mark.parametrize("name", ["qlearn_q_actions", "qlearn_td_loss_out"])
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
    assert not any(c.name.startswith("qlearn_") for c in so.CASES)
