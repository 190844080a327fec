"""Every entry point of CCX_NSTEP with each pointer at the weakest address include/ccx.h allows -- +16 for the compact arrays,
the row outputs and the Q arrays, +8 for f64 / int64 (``reward``, ``index``, the ring's ``state``, the workspace), +4 for f32
(``discount``, ``weights``, ``stats``, ``td_error``) and +1 for the byte arrays (``cut``, ``env_flags``, ``env_mask``,
``span`` and the ring's small fields) --, between guard bands (tests/_placed.py, imported): a push, a manual cut, a fetch, a
sample and the discounted TD loss with its backward on a twin with ordinary tensors give the expected bits; asserted are
bit-equal results, 4096 untouched sentinel bytes on either side of every array, and unchanged input bytes."""

import numpy as np
import pytest
from _placed import PlacedCall
from _qlearn_spec import make_td_case, td_args
from _reset_obs_spec import make_config

pytestmark = pytest.mark.gpu

SEED = 0x0123_4567_89AB_CDEF
K, S = 3, 4
RING = (("obs_c", 16), ("next_c", 16), ("actions", 1), ("reward", 8), ("done", 1), ("valid", 1), ("masks_next", 1), ("state", 8))
OUTS = (("obs", 16), ("next_obs", 16), ("actions", 1), ("reward", 8), ("done", 1), ("valid", 1), ("masks_next", 1), ("index", 8))


@pytest.mark.parametrize("E,N,B", [(5, 3, 65), (13, 8, 300)])
def test_push_mark_fetch_and_sample_on_placed_arrays(E, N, B):
    import torch

    from collectivecrossing_amd import NStepBatch, NStepReplay, ReplayBatch, ReplayRing
    from collectivecrossing_amd.batched import BatchedCollectiveCrossing

    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    b = BatchedCollectiveCrossing(make_config(N, max_steps=4), E)
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
        R = S * E
        index = rng.integers(-2, R + 2, size=B).astype(np.int64)
        mask = (np.arange(E) % 2).astype(np.uint8)

        p = PlacedCall(f"NStepReplay E={E} N={N} B={B}")
        na, nb = NStepReplay(ReplayRing(b, steps=S), n=3, gamma=0.99), NStepReplay(ReplayRing(b, steps=S), n=3, gamma=0.99)
        # the ring's arrays and the cut bytes, moved: each is read AND written, so each is an output that starts from the class's value
        for name, off in RING:
            old = getattr(nb.ring, name)
            view = p.out("ring." + name, old.shape, old.dtype, off, off)
            view.copy_(old)
            setattr(nb.ring, name, view)
        view = p.out("cut", nb.cut.shape, torch.uint8, 1, 1)
        view.copy_(nb.cut)
        nb.cut = view
        flags = p.inp("env_flags", traj.env_flags, 1, 1)
        like = na.ring.alloc_batch(B)
        fetched = NStepBatch(ReplayBatch(*(p.out("fetch." + k, getattr(like, k).shape, getattr(like, k).dtype, off, off) for k, off in OUTS)),
                             p.out("fetch.discount", (B, N), torch.float32, 4, 4), p.out("fetch.span", (B, N), torch.uint8, 1, 1))
        drawn = NStepBatch(ReplayBatch(*(p.out("sample." + k, getattr(like, k).shape, getattr(like, k).dtype, off, off) for k, off in OUTS)),
                           p.out("sample.discount", (B, N), torch.float32, 4, 4), p.out("sample.span", (B, N), torch.uint8, 1, 1))
        want = {}
        for ns, placed in ((na, False), (nb, True)):
            block = (obs0_c, acts, (traj.reward, traj.agent_flags, flags if placed else traj.env_flags, traj.obs_compact, traj.final_compact))
            ns.push(*block)
            ns.push(*block)                                              # head = 6: the second block wraps
            if placed:
                ns.mark_cut(p.inp("env_mask", mask, 1, 1))
                ns.fetch(p.inp("index_in", index, 8, 8), out=fetched)
                ns.sample(B, out=drawn)
            else:
                ns.mark_cut(torch.from_numpy(mask).cuda())
                want["fetch"] = ns.fetch(torch.from_numpy(index).cuda())
                want["sample"] = ns.sample(B)
        torch.cuda.synchronize()
        assert na.ring.state.tolist() == [2 * K, 1, 0, 0] and na.cut.any() and (want["fetch"].span > 1).any()
        expected = {"cut": na.cut, **{"ring." + k: getattr(na.ring, k) for k, _ in RING}}
        for which in ("fetch", "sample"):
            expected.update({f"{which}.{k}": getattr(want[which].batch, k) for k, _ in OUTS})
            expected.update({which + ".discount": want[which].discount, which + ".span": want[which].span})
        p.check(expected)
    finally:
        b.close()


@pytest.mark.parametrize("M,double", [(65, True), (300, False)])
def test_discounted_td_loss_on_placed_arrays(M, double):
    import torch

    from collectivecrossing_amd import QLearning, TdLossResult
    from collectivecrossing_amd.batched import BatchedCollectiveCrossing

    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    b = BatchedCollectiveCrossing(make_config(8, max_steps=12), 4)
    try:
        ql = QLearning(b)
        kw = td_args(make_td_case(M, seed=M), True, double, True, True)
        rng = np.random.default_rng(M)
        disc = rng.choice(np.array([0.0, 0.97, 0.9409, 1.0], np.float32), M)
        gloss = np.array([-1.75], np.float32)
        offs = dict(q=16, actions=1, reward=8, done=1, q_next_target=16, q_next_online=16, masks_next=1, valid=1, weights=4)
        keys = tuple(offs)
        d = {k: None if v is None else torch.from_numpy(v).cuda() for k, v in kw.items()}
        want = ql.td_loss(*(d[k] for k in keys), discount=torch.from_numpy(disc).cuda(), want_td_error=True)
        want_g = ql.td_loss_backward(*(d[k] for k in keys), discount=torch.from_numpy(disc).cuda(), stats=want.stats,
                                     grad_loss=torch.from_numpy(gloss).cuda())
        p = PlacedCall(f"td_loss(discount=) M={M} double={double}")
        args = [p.inp(k, kw[k], offs[k], offs[k]) for k in keys]
        dd = p.inp("discount", disc, 4, 4)
        stats = p.out("stats", (8,), torch.float32, 4, 4)
        ws = p.scratch("workspace", int(b._lib.ccx_td_workspace_bytes(M)), 8, 8)
        out = TdLossResult(stats[0], stats, p.out("td_error", (M,), torch.float32, 4, 4), ws, p.out("grad_q", (M, 5), torch.float32, 16, 16))
        ql.td_loss(*args, discount=dd, out=out)
        ql.td_loss_backward(*args, discount=dd, stats=stats, grad_loss=p.inp("grad_loss", gloss, 4, 4), out=out)
        p.check({"stats": want.stats, "td_error": want.td_error, "grad_q": want_g})
        assert float(want.stats[6]) > 0
    finally:
        b.close()
