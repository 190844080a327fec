"""``PrioritizedReplay`` over an ``NStepReplay`` (include/ccx.h CCX_PRIO, CCX_NSTEP) through push, sample and update, against
a twin ``PrioritizedReplay`` over a plain ring at equal state: ``index``, ``weights``, ``leaf_drawn`` and every leaf are the
twin's, the cut bytes are those of ``NStepReplay.push``, and the batch is ``NStepReplay.fetch`` of that index, bit for bit."""

import numpy as np
import pytest
from _reset_obs_spec import make_config

pytestmark = pytest.mark.gpu

SEED = 0x0123_4567_89AB_CDEF
E, N, S, B = 24, 8, 6, 150
BLOCKS = (1, 3, 2, 4)


def _same(a, b, msg):
    import torch

    assert a.dtype == b.dtype and a.shape == b.shape, msg
    assert torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8)), msg


def test_push_sample_and_update_through_the_nstep_ring():
    import torch

    from collectivecrossing_amd import NStepBatch, NStepReplay, PrioritizedReplay, ReplayBatch, ReplayRing
    from collectivecrossing_amd.batched import BatchedCollectiveCrossing

    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    b = BatchedCollectiveCrossing(make_config(N, max_steps=4), E)
    try:
        b.make_reset_pool(seed0=5, size=64)
        b.reset_from_pool()
        b.set_rng_seed(SEED)
        rng = np.random.default_rng(8)
        ns = NStepReplay(ReplayRing(b, steps=S), n=3, gamma=0.99)
        alone = NStepReplay(ReplayRing(b, steps=S), n=3, gamma=0.99)
        pn, pr = PrioritizedReplay(ns, alpha=0.6, beta=0.4), PrioritizedReplay(ReplayRing(b, steps=S), alpha=0.6, beta=0.4)
        assert pn.ring is ns.ring and pn.nstep is ns and pr.nstep is None
        first = b.rollout(rng.integers(0, 5, size=(1, E, N), dtype=np.uint8), auto_reset=True, want_compact=True, reset_obs="next")
        obs0 = first.obs_compact[0].clone()
        for K in BLOCKS:
            acts = torch.from_numpy(rng.integers(0, 5, size=(K, E, N), dtype=np.uint8)).cuda()
            traj = b.alloc_rollout(K, True, True, want_final=True)
            b.rollout(acts, auto_reset=True, out=traj, reset_obs="next")
            for target in (pn, pr, alone):
                target.push(obs0, acts, traj)
            obs0 = traj.obs_compact[K - 1].clone()
            for rnd in range(2):
                got, want = pn.sample(B, stratified=bool(rnd)), pr.sample(B, stratified=bool(rnd))
                assert isinstance(got.batch, NStepBatch) and isinstance(want.batch, ReplayBatch)
                tag = f"K {K} round {rnd}"
                _same(got.batch.index, want.batch.index, tag + ": index")
                _same(got.weights, want.weights, tag + ": weights")
                _same(got.leaf_drawn, want.leaf_drawn, tag + ": leaf_drawn")
                ref = alone.fetch(want.batch.index)
                for k in ("obs", "next_obs", "actions", "reward", "done", "valid", "masks_next", "index"):
                    _same(getattr(got.batch.batch, k), getattr(ref.batch, k), f"{tag}: {k}")
                _same(got.batch.discount, ref.discount, tag + ": discount")
                _same(got.batch.span, ref.span, tag + ": span")
                td = torch.from_numpy((rng.standard_normal((B, N)) * 3).astype(np.float32)).cuda()
                pn.update_priorities(got.batch.index, td)
                pr.update_priorities(want.batch.index, td)
                _same(pn.leaf, pr.leaf, tag + ": leaf")
                _same(pn.pstate, pr.pstate, tag + ": pstate")
            _same(ns.cut, alone.cut, f"K {K}: cut")
        assert ns.cut.any() and (got.batch.span > 1).any() and int(pn.ring.state[0]) == sum(BLOCKS) > S
        out = pn.alloc_batch(B)
        assert pn.sample(B, out=out) is out and isinstance(out.batch, NStepBatch)
        with pytest.raises(ValueError):
            pn.sample(B, out=pr.alloc_batch(B))                          # a plain batch where the n-step one is due
        with pytest.raises(ValueError):
            pr.sample(B, out=out)
        with pytest.raises(ValueError):
            PrioritizedReplay(object())
        sd = pn.state_dict()
        other = PrioritizedReplay(NStepReplay(ReplayRing(b, steps=S), n=2, gamma=0.5))
        other.load_state_dict(sd)
        _same(other.nstep.cut, ns.cut, "loaded cut")
        _same(other.leaf, pn.leaf, "loaded leaf")
        assert other.nstep.n == 3
        pn.clear()
        assert not ns.cut.any() and not pn.leaf.any() and ns.ring.state.tolist() == [0, 0, 0, 0]
    finally:
        b.close()


def test_the_examples_loop_twice():
    import importlib.util
    from pathlib import Path

    import torch

    spec = importlib.util.spec_from_file_location("dqn_nstep", Path(__file__).resolve().parent.parent / "examples" / "dqn_nstep.py")
    example = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(example)
    kw = dict(num_envs=64, updates=20, ring_steps=16, batch=256, warmup_steps=8, target_every=5, anneal_updates=10, hidden=16,
              log_every=0)
    first, counts, stats, (leaf, pstate), spans = example.train(**kw)
    second, counts2, _, (leaf2, pstate2), spans2 = example.train(**kw)
    assert counts == counts2 == (20, 0) and spans == spans2
    assert all(torch.isfinite(p).all() for p in first) and all(np.isfinite(s).all() and s[6] > 0 for s in map(np.array, stats))
    assert example.same_bits(first, second), "two runs from the same seeds must end with the same parameter bits"
    assert torch.equal(leaf, leaf2) and torch.equal(pstate, pstate2), "and with the same leaves"
    assert spans[0] == 0 and spans[1] > 0 and spans[3] > spans[1], spans          # most windows run their three steps
