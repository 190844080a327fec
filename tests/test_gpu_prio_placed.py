"""Every entry point of CCX_PRIO with each pointer at the weakest address include/ccx.h allows -- +8 for the int64 arrays
(``pstate``, the tree, ``index``, the ring's ``state``), +4 for int32 and f32 (``leaf``, ``beta``, ``weights``, ``leaf_drawn``,
``td_error``) --, between guard bands (tests/_placed.py, imported): a push, an update and a sample on a twin with ordinary
tensors give the expected bits; asserted are bit-equal results, 4096 untouched sentinel bytes on either side of every
array, and unchanged input bytes."""

import numpy as np
import pytest
from _placed import PlacedCall
from _reset_obs_spec import make_config

pytestmark = pytest.mark.gpu

SEED = 0x0123_4567_89AB_CDEF
K, S = 3, 4


@pytest.mark.parametrize("E,N,B", [(5, 3, 65), (13, 8, 300), (70, 3, 257)])     # R = 20, 52, 280 (more than one tree workgroup)
def test_push_update_and_sample_on_placed_arrays(E, N, B):
    import torch

    from collectivecrossing_amd import PrioritizedBatch, PrioritizedReplay, ReplayRing
    from collectivecrossing_amd.batched import BatchedCollectiveCrossing

    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    b = BatchedCollectiveCrossing(make_config(N, max_steps=12), E)
    try:
        b.make_reset_pool(seed0=5, size=64)
        b.reset_from_pool()
        b.set_rng_seed(SEED)
        rng = np.random.default_rng(E)
        first = b.rollout(rng.integers(0, 5, size=(1, E, N), dtype=np.uint8), auto_reset=True, want_compact=True, reset_obs="next")
        obs0_c = first.obs_compact[0].clone()
        acts = torch.from_numpy(rng.integers(0, 5, size=(K, E, N), dtype=np.uint8)).cuda()
        traj = b.alloc_rollout(K, True, True, want_final=True)
        b.rollout(acts, auto_reset=True, out=traj, reset_obs="next")
        block = (obs0_c, acts, (traj.reward, traj.agent_flags, traj.env_flags, traj.obs_compact, traj.final_compact))
        R = S * E
        index = rng.integers(-2, R + 2, size=B).astype(np.int64)
        index[:64] = 3                                                   # one slot, a whole wave
        tds = [(rng.standard_normal((B, N)) * 50).astype(np.float32) for _ in range(2)]
        tds[0][7, 0] = np.nan

        p = PlacedCall(f"PrioritizedReplay E={E} N={N} B={B}")
        pa, pb = PrioritizedReplay(ReplayRing(b, steps=S)), PrioritizedReplay(ReplayRing(b, steps=S))
        # the class's own arrays, moved: each is read AND written, so each is an output that starts from the class's value
        for name, dtype, off in (("leaf", torch.int32, 4), ("pstate", torch.int64, 8), ("beta_dev", torch.float32, 4), ("tree", torch.int64, 8)):
            old = getattr(pb, name)
            view = p.out(name, old.shape, dtype, off, off)
            view.copy_(old)
            setattr(pb, name, view)
        state = p.out("ring.state", (4,), torch.int64, 8, 8)
        state.copy_(pb.ring.state)
        pb.ring.state = state
        out = PrioritizedBatch(pb.ring.alloc_batch(B), p.out("weights", (B, N), torch.float32, 4, 4), p.out("leaf_drawn", (B,), torch.int32, 4, 4))
        out.batch.index = p.out("index", (B,), torch.int64, 8, 8)

        want = None
        for pr, placed in ((pa, False), (pb, True)):
            pr.push(*block)
            pr.push(*block)                                              # head = 6: the second block wraps
            if placed:
                pr.update_priorities(p.inp("update.index", index, 8, 8), tuple(p.inp(f"td[{a}]", t, 4, 4) for a, t in enumerate(tds)))
                pr.sample(B, out=out)
            else:
                pr.update_priorities(torch.from_numpy(index).cuda(), tuple(torch.from_numpy(t).cuda() for t in tds))
                want = pr.sample(B)
        torch.cuda.synchronize()
        assert pa.pstate.tolist()[1:3] == [1, int(pa.leaf.sum())] and int(pa.pstate[0]) > 65536 and (pa.leaf > 0).sum() == R
        p.check({"leaf": pa.leaf, "pstate": pa.pstate, "beta_dev": pa.beta_dev, "tree": pa.tree, "ring.state": pa.ring.state,
                 "weights": want.weights, "leaf_drawn": want.leaf_drawn, "index": want.batch.index})
        for k in ("obs", "next_obs", "actions", "reward", "done", "valid", "masks_next"):
            assert torch.equal(getattr(out.batch, k).view(torch.uint8), getattr(want.batch, k).view(torch.uint8)), k
    finally:
        b.close()
