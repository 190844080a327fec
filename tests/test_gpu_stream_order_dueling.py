"""The stream-order contract of the CCX_DUELING methods of ``QLearning``, with the harness of
tests/_stream_order.py (imported, not edited; its table stays the table of the batch's own classes): ``dueling(out=)``,
``dueling_into`` of three pairs, ``dueling_backward(out=)``, the autograd path, ``mlp_q_actions`` and ``sides_q_actions``, each
with torch's current stream another one than the handle's, in both directions, against the same call on a twin batch with
the handle's stream current throughout -- bit patterns; and the negative control: with the two ordering helpers switched off
the harness does see the difference."""

import numpy as np
import pytest
import _stream_order as so
from _stream_order import E, H, N, Plan, fill_bytes, inp, normal, param_inputs, prefilled, tensors

pytestmark = pytest.mark.gpu

LEAD = (4, E, N)                                 # leading shape of the row-wise cases: 2048 rows, 32 waves


def _dueling(w, rng):
    import torch
    from collectivecrossing_amd import QLearning

    ql = QLearning(w.batch)
    va = inp(normal(rng, *LEAD, 6))
    q = prefilled(LEAD + (5,), torch.float32)
    return Plan([va], lambda: [ql.dueling(va[0], out=q)], [q])


def _dueling_into(w, rng):
    import torch
    from collectivecrossing_amd import QLearning

    ql = QLearning(w.batch)
    vas = [inp(normal(rng, *LEAD, 6)) for _ in range(3)]
    qs = tuple(prefilled(LEAD + (5,), torch.float32) for _ in range(3))
    return Plan(vas, lambda: list(ql.dueling_into(tuple(v[0] for v in vas), qs)), list(qs))


def _dueling_backward(w, rng):
    import torch
    from collectivecrossing_amd import QLearning

    ql = QLearning(w.batch)
    gq = inp(normal(rng, *LEAD, 5))
    gva = prefilled(LEAD + (6,), torch.float32)
    return Plan([gq], lambda: [ql.dueling_backward(gq[0], out=gva)], [gva])


def _autograd(w, rng):
    import torch
    from collectivecrossing_amd import QLearning

    ql = QLearning(w.batch)
    va, gq = inp(normal(rng, *LEAD, 6)), inp(normal(rng, *LEAD, 5))

    def call():
        with torch.enable_grad():
            x = va[0].detach().requires_grad_()
            q = ql.dueling(x)
            q.backward(gq[0])
        return [q, x.grad]
    return Plan([va, gq], call)


def _fused_inputs(b, ql):
    import torch

    obs, masks = inp(b.observe(), 0.0), inp(b.action_masks(), 0x10)
    eps = (ql.epsilon_dev, torch.full((1,), 0.5, device="cuda"))
    ql.epsilon_dev.fill_(0.0)                                            # the stale rate: nothing explores
    out = ql.alloc_q_actions(want_explored=True)
    q_out = prefilled((E, N, 5), torch.float32)
    fill_bytes(out.actions, out.explored)
    return obs, masks, eps, out, q_out


def _mlp_q_actions(w, rng):
    from collectivecrossing_amd import QLearning

    b = w.batch
    ql = QLearning(b, epsilon=0.5)
    head = b.mlp_head(H, O=6)
    obs, masks, eps, out, q_out = _fused_inputs(b, ql)

    def sanity(got):
        acts, expl = got[0].reshape(E, N), got[1].reshape(E, N)
        assert (acts < 4).any() and (acts[acts != 255] <= 4).all() and expl.any() and not expl.all()
    return Plan([obs, masks, eps] + param_inputs(b, head),
                lambda: tensors(ql.mlp_q_actions(head, obs[0], masks[0], q_out=q_out, out=out)) + [q_out],
                [out.actions, out.explored, q_out], sanity)


def _sides_q_actions(w, rng):
    from collectivecrossing_amd import QLearning, SideHeads

    b = w.batch
    ql = QLearning(b, epsilon=0.5)
    sides = SideHeads(b, {"boarding": b.mlp_head(H, O=6)})              # the exiting slots are unowned: 255 / 0 / untouched
    params = [pair for _, head in sides.groups for pair in param_inputs(b, head)]
    obs, masks, eps, out, q_out = _fused_inputs(b, ql)

    def sanity(got):
        acts, expl = got[0].reshape(E, N), got[1].reshape(E, N)
        assert (acts[:, 5:] == 255).all() and (acts[:, :5] < 5).any() and expl[:, :5].any() and not expl[:, 5:].any()
    return Plan([obs, masks, eps] + params,
                lambda: tensors(ql.sides_q_actions(sides, obs[0], masks[0], q_out=q_out, out=out)) + [q_out],
                [out.actions, out.explored, q_out], sanity)


CASES = [so.Case("dueling_out", "sim", ("QLearning.dueling",), _dueling),
         so.Case("dueling_into_three", "sim", ("QLearning.dueling_into",), _dueling_into),
         so.Case("dueling_backward_out", "sim", ("QLearning.dueling_backward",), _dueling_backward),
         so.Case("dueling_autograd", "sim", ("QLearning.dueling",), _autograd),
         so.Case("dueling_mlp_q_actions", "sim", ("QLearning.mlp_q_actions",), _mlp_q_actions),
         so.Case("dueling_sides_q_actions", "sim", ("QLearning.sides_q_actions",), _sides_q_actions)]


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
    """Does work on ``main`` finish while the blocker keeps ``other`` busy?  (Two streams that share a hardware queue run one
    after the other whatever the library does.)"""
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
    seed = 970_000 + 1000 * CASES.index(case) + (direction == "after")   # (beyond every seed of the harness's own table)
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


@pytest.mark.parametrize("name", ["dueling_into_three", "dueling_mlp_q_actions"])
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
    assert not any(c.name.startswith("dueling_") for c in so.CASES)
