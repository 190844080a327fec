"""The stream-order contract of every enqueueing method of ``WideMlpHead``, with the harness of
tests/_stream_order.py (imported, not edited; its table stays the table of the batch's own classes): ``head(out=)``,
``param_grads(out=)`` and the autograd path with either backward, each with torch's current stream another one than the
handle's, in both directions, against the same call on a twin batch with the handle's stream current throughout -- bit
patterns; and the negative control: with the two ordering helpers switched off the harness does see the difference."""

import numpy as np
import pytest
import _stream_order as so
from _stream_order import H, ROWS, Plan, dev, fill_bytes, inp, normal, prefilled

pytestmark = pytest.mark.gpu

A = 51
O = 5 * A


def _wide(batch, backward="torch"):
    from collectivecrossing_amd import WideMlpHead

    return WideMlpHead(batch, H, O, backward=backward, out_shape=(5, A))


def _param_inputs(batch, head) -> list:
    """The head's parameters as inputs (tests/_stream_order.param_inputs for a wide head): they hold a SECOND seeded
    initialisation until the real one is copied in."""
    import torch

    other = _wide(batch)
    pairs = []
    with torch.no_grad():
        for p, q in zip(head.parameters(), other.parameters()):
            real = p.detach().clone()
            p.copy_(q)
            pairs.append((p, real))
    return pairs


def _forward(w, rng):
    import torch

    head = _wide(w.batch)
    x = inp(normal(rng, ROWS, head.L))
    y, hidden = prefilled((ROWS, 5, A), torch.float32), prefilled((ROWS, H), torch.float32)

    def call():
        with torch.no_grad():
            return [head(x[0], out=y, hidden_out=hidden), hidden]
    return Plan([x] + _param_inputs(w.batch, head), call, [y, hidden])


def _param_grads(w, rng):
    import torch

    head = _wide(w.batch)
    xr = dev(normal(rng, ROWS, head.L))
    hid = torch.empty((ROWS, H), dtype=torch.float32, device="cuda")
    head(xr, hidden_out=hid)
    x, hidden, gy = inp(xr), inp(hid), inp(normal(rng, ROWS, 5, A))
    out = head.alloc_param_grads((ROWS,), want_grad_a=True)
    grads = [out.w1t, out.b1, out.w2, out.b2, out.grad_a]
    fill_bytes(*grads)

    def call():
        head.param_grads(x[0], hidden[0], gy[0], out=out)
        return grads
    return Plan([x, hidden, gy] + _param_inputs(w.batch, head), call, grads)


def _autograd(backward):
    def setup(w, rng):
        import torch

        head = _wide(w.batch, backward)
        x, gy = inp(normal(rng, ROWS, head.L)), inp(normal(rng, ROWS, 5, A))
        x[0].requires_grad_(True)

        def call():
            with torch.enable_grad():
                y = head(x[0])
                y.backward(gy[0])
            return [y, x[0].grad, *(p.grad for p in head.parameters())]
        return Plan([x, gy] + _param_inputs(w.batch, head), call)
    return setup


CASES = [so.Case("wide_head_out", "sim", ("WideMlpHead.forward",), _forward),
         so.Case("wide_param_grads_out", "sim", ("WideMlpHead.param_grads",), _param_grads),
         so.Case("wide_head_grad_torch_backward", "sim", ("WideMlpHead.forward",), _autograd("torch")),
         so.Case("wide_head_grad_device_backward", "sim", ("WideMlpHead.forward", "WideMlpHead.param_grads"), _autograd("device"))]


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
    process; two streams that share a queue run one after the other whatever the library does, and every ``before`` /
    ``after`` run would then see an order that nobody made."""
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
    seed = 980_000 + 1000 * CASES.index(case) + (direction == "after")   # (beyond every seed of the harness's own table)
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


@pytest.mark.parametrize("name", ["wide_head_out", "wide_param_grads_out"])
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
