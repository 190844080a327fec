"""The stream-order contract of every enqueueing method of ``RolloutMinibatches``, with the harness of
tests/_stream_order.py (imported, not edited; its table stays the table of the batch's own classes): ``next(out=)``,
``fetch(out=)``, ``permutation(out=)`` and ``rewind``, each with torch's current stream another one than the handle's, in both
directions, against the same call on a twin batch with the handle's stream current throughout -- bit patterns; and the negative
control: with the two ordering helpers switched off the harness does see the difference.  Every access stays inside buffers
the case owns whatever the order: the stale state is zeros, which names positions in range, and the stale index is -1."""

import numpy as np
import pytest
import _stream_order as so
from _stream_order import E, K, N, Plan, fill_bytes, inp

pytestmark = pytest.mark.gpu

M = K * E                                        # 256 records
B_NEXT = 192                                     # a minibatch of several workgroups; the second draw of an epoch is padded
B_FETCH = 2048


def _sources(w, rng, form):
    """The rollout's arrays as (stale buffer, real value) pairs; the stale ones are legal inputs of another rollout."""
    L = w.batch.obs_len
    W = 4 if form == "compact" else L
    acts = rng.integers(0, 5, (K, E, N)).astype(np.uint8)
    return dict(obs0=inp(rng.integers(0, 9, (E, N, W)).astype(np.float32), 0.0),
                obs=inp(rng.integers(0, 9, (K, E, N, W)).astype(np.float32), 0.0),
                actions=inp(acts, 4), logp=inp(-rng.random((K, E, N)).astype(np.float32), 0.0),
                advantages=inp(so.normal(rng, K, E, N), 0.0), returns=inp(so.normal(rng, K, E, N), 0.0),
                masks=inp((rng.integers(0, 32, (K, E, N)) | 0x10).astype(np.uint8), 0x1F),
                valid=inp(((rng.random((K, E, N)) < 0.8) * 4).astype(np.uint8), 4))


def _minibatches(w, rng, form, B):
    from collectivecrossing_amd import RolloutMinibatches

    mb = RolloutMinibatches(w.batch, num_steps=K, batch_size=B)
    d = _sources(w, rng, form)
    mb.set_source(**{k: v[0] for k, v in d.items()})
    return mb, list(d.values())


def _next(form):
    def setup(w, rng):
        import torch

        mb, pairs = _minibatches(w, rng, form, B_NEXT)
        state = (mb.state, torch.tensor([3, B_NEXT, 0, 0], dtype=torch.int64, device="cuda"))   # stale: zeros, the first draw of epoch 0
        out = mb.alloc()
        outs = so.tensors(out)
        fill_bytes(*outs)

        def sanity(got):
            index = got[7].view(np.int64)
            assert (index[:M - B_NEXT] >= 0).all() and (index[M - B_NEXT:] == -1).all() and (got[1] != 255).any()
            assert got[8].view(np.int64).tolist() == [4, 0, 0, 0]
        # (the state is read AND written: it is an input here, so it is returned but not snapshotted as an output)
        return Plan(pairs + [state], lambda: so.tensors(mb.next(out=out)) + [mb.state], outs, sanity)
    return setup


def _fetch(w, rng):
    mb, pairs = _minibatches(w, rng, "rows", 4)
    index = inp(rng.integers(0, M, size=(B_FETCH,)).astype(np.int64), -1)
    out = mb.alloc(B_FETCH)
    outs = so.tensors(out)
    fill_bytes(*outs)
    return Plan(pairs + [index], lambda: so.tensors(mb.fetch(index[0], out=out)), outs)


def _permutation(w, rng):
    import torch
    from collectivecrossing_amd import RolloutMinibatches

    mb = RolloutMinibatches(w.batch, num_steps=K, batch_size=4)
    out = so.prefilled((M,), torch.int64)

    def sanity(got):
        assert sorted(got[0].view(np.int64).tolist()) == list(range(M))
    return Plan([], lambda: [mb.permutation(5, out=out)], [out], sanity)


def _rewind(w, rng):
    from collectivecrossing_amd import RolloutMinibatches

    mb = RolloutMinibatches(w.batch, num_steps=K, batch_size=4)
    fill_bytes(mb.state)

    def call():
        mb.rewind(6)
        return [mb.state]

    def sanity(got):
        assert got[0].view(np.int64).tolist() == [6, 0, 0, 0]
    return Plan([], call, [mb.state], sanity)


CASES = [so.Case("minibatch_next_rows_out", "sim", ("RolloutMinibatches.next",), _next("rows")),
         so.Case("minibatch_next_compact_out", "sim", ("RolloutMinibatches.next",), _next("compact")),
         so.Case("minibatch_fetch_out", "sim", ("RolloutMinibatches.fetch",), _fetch),
         so.Case("minibatch_permutation_out", "sim", ("RolloutMinibatches.permutation",), _permutation),
         so.Case("minibatch_rewind", "sim", ("RolloutMinibatches.rewind",), _rewind)]


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
    """Does work on ``main`` finish while the blocker keeps ``other`` busy?  (tests/test_gpu_stream_order_qlearn.py)"""
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


@pytest.mark.parametrize("name", ["minibatch_next_rows_out", "minibatch_fetch_out"])
def test_negative_control(name, rig, monkeypatch):
    """With both helpers doing nothing the harness sees a stale result and an overwritten snapshot (before) and the prefill
    in the clones (after).  Every access stays inside buffers the case owns: the stale state is zeros -- the first draw of
    epoch 0, positions in range --, and a stale index is -1, which reads nothing."""
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
    assert not any(c.name.startswith("minibatch_") for c in so.CASES)
