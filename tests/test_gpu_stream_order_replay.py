"""The stream-order contract of every enqueueing method of ``ReplayRing``, with the harness of
tests/_stream_order.py (imported, not edited; its table stays the table of the batch's own classes): ``push``,
``sample(out=)`` and ``fetch(out=)``, each with torch's current stream another one than the handle's, in both directions,
against the same call on a twin batch with the handle's stream current throughout -- bit patterns; and the negative control:
with the two ordering helpers switched off the harness does see the difference."""

import numpy as np
import pytest
import _stream_order as so
from _stream_order import E, K, N, Plan, fill_bytes, inp

pytestmark = pytest.mark.gpu

S = 8                                            # ring steps: R = 512 records
B = 2048                                         # a minibatch of several workgroups


def _block(w, rng):
    """A real K-step block of the world's batch as (stale buffer, real value) pairs: the stale flags are legal bytes, the
    stale compact records those of an earlier state."""
    import torch

    b = w.batch
    acts = so.dev(so.actions(rng, K))
    traj = b.alloc_rollout(K, want_obs=False, want_compact=True, want_final=True)
    b.rollout(acts, auto_reset=True, reset_obs="next", out=traj, want_obs=False, want_compact=True)
    obs0 = traj.obs_compact[K - 1].clone()
    acts2 = so.dev(so.actions(rng, K))
    traj2 = b.alloc_rollout(K, want_obs=False, want_compact=True, want_final=True)
    b.rollout(acts2, auto_reset=True, reset_obs="next", out=traj2, want_obs=False, want_compact=True)
    masks = rng.integers(0, 32, size=(K, E, N)).astype(np.uint8) | 0x10
    return dict(obs0=inp(obs0, traj.obs_compact[0]), actions=inp(acts2, 4), reward=inp(traj2.reward, 0.0),
                agent_flags=inp(traj2.agent_flags, so.STALE_FLAGS), env_flags=inp(traj2.env_flags, 0),
                obs_compact=inp(traj2.obs_compact, traj.obs_compact), final_compact=inp(traj2.final_compact, torch.zeros_like(traj2.final_compact)),
                masks_next=inp(masks, 0x1F))


def _ring_tensors(ring) -> list:
    return [ring.obs_c, ring.next_c, ring.actions, ring.reward, ring.done, ring.valid, ring.masks_next, ring.state]


def _push_into(ring, d, which):
    ring.push(d["obs0"][which], d["actions"][which],
              tuple(d[k][which] for k in ("reward", "agent_flags", "env_flags", "obs_compact", "final_compact")),
              masks_next=d["masks_next"][which])


def _push(w, rng):
    from collectivecrossing_amd import ReplayRing

    ring = ReplayRing(w.batch, steps=S)
    d = _block(w, rng)
    outs = _ring_tensors(ring)

    def call():
        _push_into(ring, d, 0)
        return outs

    def sanity(got):
        acts = got[2].reshape(S * E, N)
        assert (acts[:K * E] != 255).any() and (acts[K * E:] == 255).all() and got[7].view(np.int64).tolist() == [K, 0, 0, 0]
    return Plan(list(d.values()), call, outs, sanity)


def _filled_ring(w, rng):
    """The ring's arrays as inputs of a sample / fetch: they hold the EMPTY ring until the real records are copied in."""
    import torch
    from collectivecrossing_amd import ReplayRing

    ring, real = ReplayRing(w.batch, steps=S), ReplayRing(w.batch, steps=S)
    d = _block(w, rng)
    for _ in range(2):
        _push_into(real, d, 1)
    torch.cuda.synchronize()
    return ring, [(t, r.clone()) for t, r in zip(_ring_tensors(ring), _ring_tensors(real))]


def _sample(w, rng):
    ring, pairs = _filled_ring(w, rng)
    out = ring.alloc_batch(B)
    outs = so.tensors(out)
    fill_bytes(*outs)

    def sanity(got):
        index = got[7].view(np.int64)
        assert index.min() >= 0 and index.max() < 2 * K * E and (got[2] != 255).any()      # (not the -1 of the stale, empty ring)
        assert got[8].view(np.int64).tolist() == [2 * K, 1, 0, 0]
    # (the ring's state is read AND written: it is an input here, so it is returned but not snapshotted as an output)
    return Plan(pairs, lambda: so.tensors(ring.sample(B, out=out)) + [ring.state], outs, sanity)


def _fetch(w, rng):
    ring, pairs = _filled_ring(w, rng)
    index = inp(rng.integers(0, 2 * K * E, size=(B,)).astype(np.int64), -1)
    out = ring.alloc_batch(B)
    outs = so.tensors(out)
    fill_bytes(*outs)
    return Plan(pairs + [index], lambda: so.tensors(ring.fetch(index[0], out=out)), outs)


CASES = [so.Case("replay_push", "sim", ("ReplayRing.push",), _push),
         so.Case("replay_sample_out", "sim", ("ReplayRing.sample",), _sample),
         so.Case("replay_fetch_out", "sim", ("ReplayRing.fetch",), _fetch)]


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


@pytest.mark.parametrize("name", ["replay_push", "replay_sample_out"])
def test_negative_control(name, rig, monkeypatch):
    """With both helpers doing nothing the harness sees a stale result and an overwritten snapshot (before) and the prefill
    in the clones (after).  Every access stays inside buffers the case owns: the stale ring is the EMPTY one, whose draws are
    -1 and read nothing, and a stale index is -1."""
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
    assert not any(c.name.startswith("replay_") for c in so.CASES)
