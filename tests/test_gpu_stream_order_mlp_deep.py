"""The stream-order contract of every enqueueing method of ``DeepMlpHead``, with the harness of
tests/_stream_order.py (imported, not edited; its table stays the table of the batch's own classes): ``head(out=)``,
``param_grads(out=)``, the autograd path with either backward, ``sample_actions`` and ``q_actions``, each with torch's
current stream another one than the handle's, in both directions, against the same call on a twin batch with the handle's
stream current throughout -- bit patterns; and the negative control: with the two ordering helpers switched off the harness
does see the difference."""

import numpy as np
import pytest
import _stream_order as so
from _stream_order import E, H, N, ROWS, Plan, dev, fill_bytes, inp, normal, prefilled, tensors

pytestmark = pytest.mark.gpu

H2 = 32


def _deep(batch, backward="torch", O=5):
    from collectivecrossing_amd import DeepMlpHead

    return DeepMlpHead(batch, H, H2, O, backward=backward)


def _param_inputs(batch, head) -> list:
    """The head's parameters as inputs (tests/_stream_order.param_inputs for a deep head): they hold a SECOND seeded
    initialisation until the real one is copied in."""
    import torch

    other = _deep(batch, O=head.O)
    pairs = []
    with torch.no_grad():
        for p, q in zip(head.parameters(), other.parameters()):
            real = p.detach().clone()
            p.copy_(q)
            pairs.append((p, real))
    return pairs


def _forward(w, rng):
    import torch

    head = _deep(w.batch)
    x = inp(normal(rng, ROWS, head.L))
    y, h1, h2 = (prefilled((ROWS, k), torch.float32) for k in (5, H, H2))

    def call():
        with torch.no_grad():
            return [head(x[0], out=y, hidden1_out=h1, hidden2_out=h2), h1, h2]
    return Plan([x] + _param_inputs(w.batch, head), call, [y, h1, h2])


def _param_grads(w, rng):
    import torch

    head = _deep(w.batch)
    xr = dev(normal(rng, ROWS, head.L))
    a, b = (torch.empty((ROWS, k), dtype=torch.float32, device="cuda") for k in (H, H2))
    head(xr, hidden1_out=a, hidden2_out=b)
    x, h1, h2, gy = inp(xr), inp(a), inp(b), inp(normal(rng, ROWS, 5))
    out = head.alloc_param_grads((ROWS,), want_grad_a=True)
    grads = [*out.grads(), out.grad_a1, out.grad_a2]
    fill_bytes(*grads)

    def call():
        head.param_grads(x[0], h1[0], h2[0], gy[0], out=out)
        return grads
    return Plan([x, h1, h2, gy] + _param_inputs(w.batch, head), call, grads)


def _autograd(backward):
    def setup(w, rng):
        import torch

        head = _deep(w.batch, backward)
        x, gy = inp(normal(rng, ROWS, head.L)), inp(normal(rng, ROWS, 5))
        x[0].requires_grad_(True)

        def call():
            with torch.enable_grad():
                y = head(x[0])
                y.backward(gy[0])
            return [y, x[0].grad, *(p.grad for p in head.parameters())]
        return Plan([x, gy] + _param_inputs(w.batch, head), call)
    return setup


def _sample(w, rng):
    import torch

    b = w.batch
    head = _deep(b)
    obs, masks = inp(b.observe(), 0.0), inp(b.action_masks(), 0x1F)
    out = b.alloc_sample(True, True)
    logits = prefilled((E, N, 5), torch.float32)
    fill_bytes(*tensors(out))
    return Plan([obs, masks] + _param_inputs(b, head),
                lambda: tensors(head.sample_actions(obs[0], masks[0], logits_out=logits, out=out)) + [logits], tensors(out) + [logits])


def _q_actions(w, rng):
    import torch

    from collectivecrossing_amd import QLearning

    b = w.batch
    head = _deep(b, O=6)
    ql = QLearning(b, epsilon=0.25)
    obs, masks = inp(b.observe(), 0.0), inp(b.action_masks(), 0x1F)
    out = ql.alloc_q_actions(want_explored=True)
    q = prefilled((E, N, 5), torch.float32)
    fill_bytes(*tensors(out))
    return Plan([obs, masks] + _param_inputs(b, head),
                lambda: tensors(head.q_actions(ql, obs[0], masks[0], q_out=q, out=out)) + [q], tensors(out) + [q])


CASES = [so.Case("deep_head_out", "sim", ("DeepMlpHead.forward",), _forward),
         so.Case("deep_param_grads_out", "sim", ("DeepMlpHead.param_grads",), _param_grads),
         so.Case("deep_head_grad_torch_backward", "sim", ("DeepMlpHead.forward",), _autograd("torch")),
         so.Case("deep_head_grad_device_backward", "sim", ("DeepMlpHead.forward", "DeepMlpHead.param_grads"), _autograd("device")),
         so.Case("deep_sample_actions", "sim", ("DeepMlpHead.sample_actions",), _sample),
         so.Case("deep_q_actions", "sim", ("DeepMlpHead.q_actions",), _q_actions)]


def test_every_enqueueing_method_of_the_class_has_a_case():
    """The public methods of ``DeepMlpHead`` whose source reaches ``_enqueue`` (directly or through a private method of the
    class) are exactly the ones the cases cover."""
    import inspect
    import re

    from collectivecrossing_amd import DeepMlpHead

    src = {n: inspect.getsource(f) for n, f in vars(DeepMlpHead).items() if inspect.isfunction(f)}

    def reaches(name, seen=()):
        text = src[name]
        return "._enqueue(" in text or "_DeepForward.apply(" in text or any(
            reaches(n, seen + (name,)) for n in set(re.findall(r"\bself\.(\w+)\(", text)) if n in src and n not in seen and n != name)

    public = {f"DeepMlpHead.{n}" for n in src if not n.startswith("_") and reaches(n)}
    assert public == {m for c in CASES for m in c.covers}, public


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
    seed = 990_000 + 1000 * CASES.index(case) + (direction == "after")   # (beyond every seed of the harness's own table)
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


@pytest.mark.parametrize("name", ["deep_head_out", "deep_param_grads_out", "deep_sample_actions"])
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
