"""The stream-order contract of every enqueueing method of ``PrioritizedReplay``, with the harness of
tests/_stream_order.py (imported, not edited; its table stays the table of the batch's own classes): ``push``,
``update_priorities`` and ``sample(out=)``, each with torch's current stream another one than the handle's, in both
directions, against the same call on a twin batch with the handle's stream current throughout -- bit patterns; and the
negative control: with the two ordering helpers switched off the harness does see the difference.  Every access stays inside
buffers the case owns whatever the order: stale leaves are zeros (nothing is drawable, index -1 reads nothing), a stale
index is -1 (the update changes nothing)."""

import numpy as np
import pytest
import _stream_order as so
from _stream_order import E, K, N, Plan, fill_bytes, inp
from test_gpu_stream_order_replay import _block, _push_into, _ring_tensors, _run_side_by_side

pytestmark = pytest.mark.gpu

S = 8                                            # ring steps: R = 512 records, two tree workgroups
B = 2048                                         # a minibatch of several workgroups
MAX_LEAF = 3 * 65536


def _new(w):
    from collectivecrossing_amd import PrioritizedReplay, ReplayRing

    return PrioritizedReplay(ReplayRing(w.batch, steps=S))


def _push(w, rng):
    """The block's arrays AND ``pstate`` are inputs: the stale max_leaf is the initial 65536, the real one three times that."""
    pr = _new(w)
    d = _block(w, rng)
    real = pr.pstate.clone()
    real[0] = MAX_LEAF
    outs = _ring_tensors(pr.ring) + [pr.leaf]

    def call():
        pr.push(d["obs0"][0], d["actions"][0], tuple(d[k][0] for k in ("reward", "agent_flags", "env_flags", "obs_compact", "final_compact")),
                masks_next=d["masks_next"][0])
        return outs

    def sanity(got):
        leaf = got[8].view(np.int32)
        assert (leaf[:K * E] == MAX_LEAF).all() and not leaf[K * E:].any() and got[7].view(np.int64).tolist() == [K, 0, 0, 0]
    return Plan(list(d.values()) + [(pr.pstate, real)], call, outs, sanity)


def _filled(w, rng):
    """A prioritised ring whose arrays and leaves are inputs: they hold the EMPTY ring and zero leaves until the real ones
    (two pushed blocks, leaves of mixed sizes) are copied in."""
    import torch

    pr, real = _new(w), _new(w)
    d = _block(w, rng)
    for _ in range(2):
        _push_into(real.ring, d, 1)
    leaf = torch.zeros_like(real.leaf)
    leaf[:2 * K * E] = so.dev(rng.integers(1, 1 << 24, size=2 * K * E).astype(np.int32))
    torch.cuda.synchronize()
    pairs = [(t, r.clone()) for t, r in zip(_ring_tensors(pr.ring), _ring_tensors(real.ring))] + [(pr.leaf, leaf)]
    return pr, pairs


def _sample(w, rng):
    pr, pairs = _filled(w, rng)
    out = pr.alloc_batch(B)
    outs = so.tensors(out.batch) + [out.weights, out.leaf_drawn]
    fill_bytes(*outs)

    def call():
        got = pr.sample(B, out=out)
        return so.tensors(got.batch) + [got.weights, got.leaf_drawn, pr.pstate]

    def sanity(got):
        index = got[7].view(np.int64)
        assert index.min() >= 0 and index.max() < 2 * K * E and (got[2] != 255).any()      # (not the -1 of the stale zero leaves)
        assert (got[8].view(np.float32) > 0).all() and got[10].view(np.int64).tolist()[1] == 1
    # (pstate is read AND written: returned, not snapshotted as an output)
    return Plan(pairs, call, outs, sanity)


def _update(w, rng):
    import torch

    pr = _new(w)
    pr.leaf.fill_(65536)
    index = inp(rng.integers(0, S * E, size=(B,)).astype(np.int64), -1)
    tds = [inp((rng.standard_normal((B, N)) * 10).astype(np.float32), 0.0) for _ in range(2)]
    outs = [pr.leaf, pr.pstate]

    def call():
        pr.update_priorities(index[0], (tds[0][0], tds[1][0]))
        return outs

    def sanity(got):
        leaf = got[0].view(np.int32)
        assert (leaf != 65536).sum() > S * E // 2 and leaf.min() > 0 and got[1].view(np.int64)[0] == leaf.max()
    torch.cuda.synchronize()
    return Plan([index] + tds, call, outs, sanity)


CASES = [so.Case("prio_push", "sim", ("PrioritizedReplay.push",), _push),
         so.Case("prio_sample_out", "sim", ("PrioritizedReplay.sample",), _sample),
         so.Case("prio_update", "sim", ("PrioritizedReplay.update_priorities",), _update)]


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
    assert any(so.differs([g], [p]) for g, p in zip(want.got, want.pre)), "the call changed no output"


@pytest.mark.parametrize("name", ["prio_push", "prio_sample_out"])
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
    assert not any(c.name.startswith("prio_") for c in so.CASES)
