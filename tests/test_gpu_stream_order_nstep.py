"""The stream-order contract of every enqueueing method of ``NStepReplay``, with the harness of
tests/_stream_order.py (imported, not edited; its table stays the table of the batch's own classes): ``push``, ``mark_cut``,
``sample(out=)`` and ``fetch(out=)``, each with torch's current stream another one than the handle's, in both directions,
against the same call on a twin batch with the handle's stream current throughout -- bit patterns; and the negative control:
with the two ordering helpers switched off the harness does see the difference.  Every access stays inside buffers the case
owns whatever the order: a stale ring is the EMPTY one with head 0 (no successor exists), a stale index is -1 (nothing is
read), and every slot is reduced mod S."""

import numpy as np
import pytest
import _stream_order as so
from _stream_order import E, K, Plan, fill_bytes, inp
from test_gpu_stream_order_replay import _block, _ring_tensors, _run_side_by_side

pytestmark = pytest.mark.gpu

S = 8                                            # ring steps: R = 512 records
B = 2048                                         # a minibatch of several workgroups


def _new(w):
    from collectivecrossing_amd import NStepReplay, ReplayRing

    return NStepReplay(ReplayRing(w.batch, steps=S), n=3, gamma=0.99)


def _batch_tensors(mb) -> list:
    return so.tensors(mb.batch) + [mb.discount, mb.span]


def _push(w, rng):
    """The block's arrays are inputs; the stale env flags are zeros (no cut), the real ones end episodes."""
    ns = _new(w)
    ns.cut.fill_(9)
    d = _block(w, rng)
    outs = _ring_tensors(ns.ring) + [ns.cut]

    def call():
        ns.push(d["obs0"][0], d["actions"][0], tuple(d[k][0] for k in ("reward", "agent_flags", "env_flags", "obs_compact", "final_compact")),
                masks_next=d["masks_next"][0])
        return outs

    def sanity(got):
        cut = got[8]
        assert set(np.unique(cut[:K * E])) <= {0, 1} and (cut[K * E:] == 9).all() and got[7].view(np.int64).tolist() == [K, 0, 0, 0]
    return Plan(list(d.values()), call, outs, sanity)


def _filled(w, rng):
    """An n-step ring whose arrays and cut bytes are inputs: they hold the EMPTY ring and no cut until the real ones (two
    pushed blocks) are copied in."""
    import torch

    ns, real = _new(w), _new(w)
    d = _block(w, rng)
    for _ in range(2):
        real.push(d["obs0"][1], d["actions"][1], tuple(d[k][1] for k in ("reward", "agent_flags", "env_flags", "obs_compact", "final_compact")),
                  masks_next=d["masks_next"][1])
    torch.cuda.synchronize()
    pairs = [(t, r.clone()) for t, r in zip(_ring_tensors(ns.ring), _ring_tensors(real.ring))] + [(ns.cut, real.cut.clone())]
    return ns, pairs


def _mark(w, rng):
    """``env_mask`` and the ring's ``state`` are inputs: the stale head is 0 (nothing is marked), the stale mask zeros."""
    import torch

    ns = _new(w)
    mask = inp((np.arange(E) % 2).astype(np.uint8), 0)
    state = torch.tensor([S + 3, 0, 0, 0], dtype=torch.int64, device="cuda")
    outs = [ns.cut]

    def call():
        ns.mark_cut(mask[0])
        return outs

    def sanity(got):
        cut = got[0].reshape(S, E)
        assert (cut[2] == np.arange(E) % 2).all() and cut.sum() == E // 2
    torch.cuda.synchronize()
    return Plan([mask, (ns.ring.state, state)], call, outs, sanity)


def _sample(w, rng):
    ns, pairs = _filled(w, rng)
    out = ns.alloc_batch(B)
    outs = _batch_tensors(out)
    fill_bytes(*outs)

    def sanity(got):
        index = got[7].view(np.int64)
        assert index.min() >= 0 and index.max() < 2 * K * E and (got[2] != 255).any()      # (not the -1 of the stale, empty ring)
        assert (got[9] > 1).any() and got[10].view(np.int64).tolist() == [2 * K, 1, 0, 0]   # windows of several steps
    # (the ring's state is read AND written: it is an input here, so it is returned but not snapshotted as an output)
    return Plan(pairs, lambda: _batch_tensors(ns.sample(B, out=out)) + [ns.ring.state], outs, sanity)


def _fetch(w, rng):
    ns, pairs = _filled(w, rng)
    index = inp(rng.integers(0, 2 * K * E, size=(B,)).astype(np.int64), -1)
    out = ns.alloc_batch(B)
    outs = _batch_tensors(out)
    fill_bytes(*outs)
    return Plan(pairs + [index], lambda: _batch_tensors(ns.fetch(index[0], out=out)), outs, lambda got: (got[9] > 1).any() or pytest.fail("no window of several steps"))


CASES = [so.Case("nstep_push", "sim", ("NStepReplay.push",), _push),
         so.Case("nstep_mark_cut", "sim", ("NStepReplay.mark_cut",), _mark),
         so.Case("nstep_sample_out", "sim", ("NStepReplay.sample",), _sample),
         so.Case("nstep_fetch_out", "sim", ("NStepReplay.fetch",), _fetch)]


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
    assert any(so.differs([g], [p]) for g, p in zip(want.got, want.pre)), "the call changed no output"


@pytest.mark.parametrize("name", ["nstep_push", "nstep_sample_out"])
def test_negative_control(name, rig, monkeypatch):
    """With both helpers doing nothing the harness sees a stale result and an overwritten snapshot (before) and the old
    bytes in the clones (after)."""
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
    assert not any(c.name.startswith("nstep_") for c in so.CASES)
