"""Prioritised replay on the device (include/ccx.h: CCX_PRIO) against the spec (tests/_prio_spec.py: Python-integer cumulative
sums and ``bisect_right``, NumPy f32), bit for bit: the draw over leaf arrays whose sizes sit on every boundary of the sum
tree (256 leaves to a workgroup, 65 536 to a second-level one) with equal, single, sparse and saturated leaves; minibatch
sizes around a wave and a workgroup, stratified and not; the update with duplicates inside a wave and across workgroups,
out-of-range indices, slots never pushed, NaN and inf, on a ring filled from real rollouts; the push; a captured round
replayed against eager rounds with ``beta`` changed in between; consistency with the ring's own fetch; checkpoints and
refusals."""

import numpy as np
import pytest
from _prio_spec import LEAF_MAX, ONE_FIXED, new_pstate, push_leaf_spec, sample_spec, update_spec
from _reset_obs_spec import make_config
from test_gpu_replay import BLOCKS, OUT_KEYS, World, batch_np, same
from test_gpu_replay import E, S, SEED

pytestmark = pytest.mark.gpu

SIZES = [1, 2, 255, 256, 257, 65_535, 65_536, 65_537, 65_536 + 257]
BATCHES = [1, 63, 64, 65, 256, 257]


def prio_np(mb) -> dict:
    return dict(index=mb.batch.index.cpu().numpy(), weights=mb.weights.cpu().numpy(), leaf_drawn=mb.leaf_drawn.cpu().numpy())


def check_sample(pr, leaf, pstate, B, stratified, beta, tag):
    """One sample launch against the spec; ``pstate`` (the spec's) advances with it."""
    mb = pr.sample(B, stratified=stratified)
    got = prio_np(mb)
    want = sample_spec(leaf, pstate, SEED, B, pr.batch.num_agents, beta, stratified)
    for k in ("index", "leaf_drawn", "weights"):
        same(got[k], want[k], f"{tag}: {k}")
    same(pr.pstate.cpu().numpy(), pstate, f"{tag}: pstate")
    return mb, got


# ------------------------------------------------------------------------------------------------- 1. the tree's boundaries
@pytest.fixture(scope="module")
def one_env():
    import torch

    from collectivecrossing_amd.batched import BatchedCollectiveCrossing

    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    b = BatchedCollectiveCrossing(make_config(3, max_steps=8), 1)
    b.set_rng_seed(SEED)
    yield b
    b.close()


def _patterns(R, rng):
    yield "all equal", np.full(R, 3 * ONE_FIXED, np.int32)
    one = np.zeros(R, np.int32)
    one[(2 * R) // 3] = 12345
    yield "one non-zero", one
    sparse = rng.integers(1, 1 << 24, R).astype(np.int32)
    sparse[rng.random(R) < 0.4] = 0
    for a in range(256, R, 1024):                                        # whole empty workgroups, and an empty second-level stretch
        sparse[a:a + 256] = 0
    sparse[4096:8192] = 0
    if not sparse.any():
        sparse[0] = 5
    yield "random with empty blocks", sparse
    yield "all 2^31 - 1", np.full(R, LEAF_MAX, np.int32)


@pytest.mark.parametrize("R", SIZES)
def test_draw_at_the_tree_boundaries(one_env, R):
    import torch

    from collectivecrossing_amd import PrioritizedReplay, ReplayRing

    pr = PrioritizedReplay(ReplayRing(one_env, steps=R), beta=0.4)
    assert pr.leaf.shape == (R,) and pr.tree.numel() == one_env._lib.ccx_prio_tree_words(R) and pr.pstate.tolist() == [ONE_FIXED, 0, 0, 0]
    rng = np.random.default_rng(R)
    pstate = new_pstate()
    for what, leaf in _patterns(R, rng):
        pr.leaf.copy_(torch.from_numpy(leaf))
        pr.tree.fill_(-0x0123456789)                                     # the refresh rewrites what the draw reads
        for B, strat in ((257, True), (65, False)):
            _, got = check_sample(pr, leaf, pstate, B, strat, 0.4, f"R {R} {what} B {B} stratified {strat}")
            assert (leaf[got["index"]] > 0).all()
        if what == "all equal":                                          # the uniform draw of the same words
            assert got["index"].min() >= 0 and got["index"].max() < R and (got["weights"] == 1.0).all()
    assert int(pstate[1]) == 8


@pytest.mark.parametrize("R", [257, 65_536 + 257])
def test_minibatch_sizes_stratified_and_not(one_env, R):
    import torch

    from collectivecrossing_amd import PrioritizedReplay, ReplayRing

    pr = PrioritizedReplay(ReplayRing(one_env, steps=R), beta=1.0)
    rng = np.random.default_rng(R + 1)
    leaf = rng.integers(0, 1 << 20, R).astype(np.int32)
    pr.leaf.copy_(torch.from_numpy(leaf))
    pstate = new_pstate()
    for n, B in enumerate(BATCHES):
        for strat in (True, False):
            pr.beta = beta = (0.0, 0.4, 1.0)[n % 3]
            mb, got = check_sample(pr, leaf, pstate, B, strat, beta, f"R {R} B {B} stratified {strat}")
            if strat:
                assert (np.diff(got["index"]) >= 0).all()                 # one draw per stratum, in order
            fetched = batch_np(pr.ring.fetch(mb.batch.index))            # consistency with the ring
            for k in OUT_KEYS:
                same(batch_np(mb.batch)[k], fetched[k], f"B {B}: batch.{k}")


def test_nothing_drawable(one_env):
    from collectivecrossing_amd import PrioritizedReplay, ReplayRing

    pr = PrioritizedReplay(ReplayRing(one_env, steps=300))
    mb = pr.sample(65)
    got = prio_np(mb)
    assert (got["index"] == -1).all() and not got["leaf_drawn"].any() and not got["weights"].view(np.uint32).any()
    assert pr.pstate.tolist() == [ONE_FIXED, 1, 0, 0] and (mb.batch.actions == 255).all()


# ------------------------------------------------------------------------------------------------- 2. push and update
@pytest.fixture(scope="module", params=[8, 3], ids=["N8", "N3"])
def world(request):
    import torch

    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    w = World(request.param, False)
    yield w
    w.close()


def _td(rng, B, N, count):
    tds = []
    for a in range(count):
        td = (rng.standard_normal((B, N)) * np.exp2(rng.integers(-24, 11, (B, 1)))).astype(np.float32)
        td[rng.random((B, N)) < 0.05] = np.nan
        td[rng.random((B, N)) < 0.2] = 0.0
        td[[20 + a, B - 40 + a], [0, N - 1]] = np.inf * (1 - 2 * a)         # (few: the maximum over duplicates must not saturate everywhere)
        tds.append(td)
    tds[0][5] = np.nan                                                   # a record of NaNs only
    return tds


def _indices(rng, B, R):
    """int64 [B >= 600]: duplicates everywhere, one slot 64 times in one wave, one slot in three workgroups, indices outside."""
    idx = rng.integers(0, R, B).astype(np.int64)
    idx[64:128] = 5
    idx[[0, 256 + 3, 599]] = 7
    idx[[10, 300, 301, 302]] = [-1, R, 1 << 40, -(1 << 62)]
    return idx


def test_push_and_update_equal_the_spec(world):
    """The four blocks (a partly filled ring, a block that wraps inside itself, K == S) pushed through the class, with an
    update behind every block: the next push overwrites updated leaves with the max_leaf the updates have raised."""
    import torch

    from collectivecrossing_amd import PrioritizedReplay, ReplayRing

    b, N, R = world.batch, world.N, S * E
    pr = PrioritizedReplay(ReplayRing(b, steps=S))
    leaf, pstate = np.zeros(R, np.int64), new_pstate()
    rng = np.random.default_rng(40 + N)
    head = 0
    cases = [(1, 0.6), (2, 1.0), (3, 0.0), (2, 0.6)]
    for n, ((obs0, acts, traj, masks), K, (count, alpha)) in enumerate(zip(world.dev_blocks, BLOCKS, cases)):
        pr.push(obs0, acts, traj, masks_next=masks)
        push_leaf_spec(leaf, pstate, head, K, S, E)
        head += K
        same(pr.leaf.cpu().numpy().astype(np.int64), leaf, f"leaves after block {n}")
        same(pr.pstate.cpu().numpy(), pstate, f"pstate after block {n}")
        assert pr.ring.state.tolist()[0] == head and (n > 0 or (leaf[E:] == 0).all())      # (block 0: slots never pushed)
        B = 600
        idx, tds = _indices(rng, B, R), _td(rng, B, N, count)
        dev = tuple(torch.from_numpy(t).cuda() for t in tds)
        pr.update_priorities(torch.from_numpy(idx).cuda(), dev[0] if count == 1 else dev, alpha=alpha)
        update_spec(leaf, pstate, idx, tds, alpha, pr.eps)
        same(pr.leaf.cpu().numpy().astype(np.int64), leaf, f"leaves after update {n} ({count} arrays, alpha {alpha})")
        same(pr.pstate.cpu().numpy(), pstate, f"pstate after update {n}")
        assert leaf.min() >= 0 and (alpha == 0.0 or pstate[0] > ONE_FIXED)
    assert (leaf > 0).all() and len(set(leaf.tolist())) > 50
    # the ring's records are the ring's own push
    for k, v in world.after[-1][1].items():
        if k != "state":
            same(getattr(pr.ring, k).cpu().numpy(), v, f"ring.{k}")
    # and a draw over these leaves, fetched
    mb, got = check_sample(pr, leaf, pstate, 300, True, pr.beta, "after the pushes")
    fetched = batch_np(pr.ring.fetch(mb.batch.index))
    for k in OUT_KEYS:
        same(batch_np(mb.batch)[k], fetched[k], f"batch.{k}")
    assert got["weights"].max() == 1.0 or int(pstate[3]) not in got["leaf_drawn"]


# ------------------------------------------------------------------------------------------------- 3. captured
def test_a_captured_round_equals_eager_rounds(world):
    import torch

    from collectivecrossing_amd import PrioritizedReplay, ReplayRing
    from collectivecrossing_amd.batched import RolloutResult

    b, N, K, B = world.batch, world.N, 2, 257
    rng = np.random.default_rng(77)
    betas = (0.4, 0.7, 1.0)
    side = torch.cuda.Stream()
    b.use_stream(side)
    torch.cuda.synchronize()
    try:
        with torch.cuda.stream(side):
            feeds = []
            for obs0, acts, traj, masks in world.dev_blocks[1:]:
                feeds.append((obs0, acts[:K].contiguous(), traj.reward[:K].contiguous(), traj.agent_flags[:K].contiguous(),
                              traj.env_flags[:K].contiguous(), traj.obs_compact[:K].contiguous(), traj.final_compact[:K].contiguous(),
                              masks[:K].contiguous(), torch.from_numpy(_td(rng, B, N, 2)[0]).cuda(), torch.from_numpy(_td(rng, B, N, 2)[1]).cuda()))
            twin, eager = PrioritizedReplay(ReplayRing(b, steps=S)), []
            for f, beta in zip(feeds, betas):
                twin.beta = beta
                twin.push(f[0], f[1], tuple(f[2:7]), masks_next=f[7])
                mb = twin.sample(B)
                twin.update_priorities(mb.batch.index, (f[8], f[9]))
                side.synchronize()
                eager.append({**batch_np(mb.batch), **prio_np(mb), "leaf": twin.leaf.cpu().numpy(), "pstate": twin.pstate.cpu().numpy()})
            pr = PrioritizedReplay(ReplayRing(b, steps=S))
            static = [torch.empty_like(t) for t in feeds[0]]
            out = pr.alloc_batch(B)
            traj = RolloutResult(None, static[2], static[3], static[4], obs_compact=static[5], final_compact=static[6])
            side.synchronize()
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph, stream=side):
                pr.push(static[0], static[1], traj, masks_next=static[7])
                pr.sample(B, out=out)
                pr.update_priorities(out.batch.index, (static[8], static[9]))
            side.synchronize()
            assert pr.pstate.tolist() == [ONE_FIXED, 0, 0, 0] and not pr.leaf.any()       # capturing ran nothing
            for n, (f, beta) in enumerate(zip(feeds, betas)):
                for dst, src in zip(static, f):
                    dst.copy_(src)
                pr.beta = beta                                           # between replays: the device scalar
                graph.replay()
                side.synchronize()
                got = {**batch_np(out.batch), **prio_np(out), "leaf": pr.leaf.cpu().numpy(), "pstate": pr.pstate.cpu().numpy()}
                for k, v in eager[n].items():
                    same(got[k], v, f"replay {n}: {k}")
                assert pr.pstate.tolist()[1] == n + 1 and pr.ring.state.tolist()[0] == K * (n + 1)
            assert len({tuple(e["index"].tolist()) for e in eager}) == 3
            assert not np.array_equal(eager[1]["weights"], eager[2]["weights"])
    finally:
        torch.cuda.synchronize()
        b.use_stream(None)


# ------------------------------------------------------------------------------------------------- 4. checkpoints, clear, refusals
def test_state_dict_clear_and_refusals(world):
    import torch

    from collectivecrossing_amd import PrioritizedBatch, PrioritizedReplay, ReplayRing

    b, N = world.batch, world.N
    pr = PrioritizedReplay(ReplayRing(b, steps=S), alpha=0.5, beta=0.25, eps=1e-3)
    obs0, acts, traj, masks = world.dev_blocks[1]
    pr.push(obs0, acts, traj, masks_next=masks)
    mb = pr.sample(64)
    pr.update_priorities(mb.batch.index, torch.rand((64, N), device="cuda"))
    sd = pr.state_dict()
    assert set(sd) == {"leaf", "pstate", "beta", "alpha", "eps", "ring"} and sd["beta"] == 0.25
    other = PrioritizedReplay(ReplayRing(b, steps=S))
    other.load_state_dict(sd)
    assert (other.alpha, other.beta, other.eps) == (pr.alpha, pr.beta, pr.eps) and float(other.beta_dev) == 0.25
    same(other.leaf.cpu().numpy(), pr.leaf.cpu().numpy())
    same(other.pstate.cpu().numpy(), pr.pstate.cpu().numpy())
    same(other.ring.reward.cpu().numpy(), pr.ring.reward.cpu().numpy())
    a, c = prio_np(pr.sample(65)), prio_np(other.sample(65))
    for k in a:
        same(a[k], c[k], f"after load_state_dict: {k}")
    pr.clear()
    assert not pr.leaf.any() and pr.pstate.tolist() == [ONE_FIXED, 0, 0, 0] and pr.ring.state.tolist() == [0, 0, 0, 0]
    assert (pr.ring.actions == 255).all()
    idx, td = torch.zeros(4, dtype=torch.int64, device="cuda"), torch.zeros((4, N), device="cuda")
    for bad in (dict(alpha=-0.1), dict(alpha=1.5), dict(alpha=float("nan")), dict(eps=0.0), dict(eps=-1.0), dict(eps=float("inf"))):
        with pytest.raises(ValueError):
            pr.update_priorities(idx, td, **bad)
        with pytest.raises(ValueError):
            PrioritizedReplay(pr.ring, **bad)
    for bad_idx, bad_td in ((idx.int(), td), (idx, td.double()), (idx, td[:3]), (idx, ()), (idx, (td,) * 9), (idx[:0], td[:0]),
                            (idx, td.cpu()), (idx, td.T.contiguous().T if N > 1 else td[:, :0])):
        with pytest.raises(ValueError):
            pr.update_priorities(bad_idx, bad_td)
    with pytest.raises(ValueError):
        pr.beta = 1.5
    with pytest.raises(ValueError):
        PrioritizedReplay(b)
    out = pr.alloc_batch(8)
    for bad_out in (pr.ring.alloc_batch(8), PrioritizedBatch(out.batch, out.weights[:4], out.leaf_drawn),
                    PrioritizedBatch(out.batch, out.weights, out.leaf_drawn.long())):
        with pytest.raises(ValueError):
            pr.sample(8, out=bad_out)
    for bad_B in (0, -1, 2.5):
        with pytest.raises(ValueError):
            pr.sample(bad_B)
    assert not pr.leaf.any() and pr.pstate.tolist() == [ONE_FIXED, 0, 0, 0]               # a refused call enqueues nothing
    # the library's own refusals, before any launch
    lib, h = b._lib, b._h
    from collectivecrossing_amd import _abi
    assert lib.ccx_prio_push(h, S, pr.ring.state.data_ptr(), S + 1, pr.leaf.data_ptr(), pr.pstate.data_ptr()) == _abi.EINVAL
    assert lib.ccx_prio_push(h, S, pr.ring.state.data_ptr(), 1, pr.leaf.data_ptr() + 2, pr.pstate.data_ptr()) == _abi.EINVAL
    assert lib.ccx_prio_sample(h, S, pr.leaf.data_ptr(), pr.pstate.data_ptr() + 4, pr.beta_dev.data_ptr(), pr.tree.data_ptr(), 8, 1,
                               out.batch.index.data_ptr(), out.weights.data_ptr(), out.leaf_drawn.data_ptr()) == _abi.EINVAL
    assert b"pstate must be 8-byte aligned" in lib.ccx_last_error()
    assert lib.ccx_prio_tree_words(0) == 0 and lib.ccx_prio_tree_words(1 << 31) == 0 and lib.ccx_prio_tree_words(256) == 2 * (16 + 1 + 1)
    torch.cuda.synchronize()
    assert not pr.leaf.any() and pr.pstate.tolist() == [ONE_FIXED, 0, 0, 0]


# ------------------------------------------------------------------------------------------------- 5. the example's loop, twice
def test_the_examples_loop_twice():
    import importlib.util
    from pathlib import Path

    import torch

    spec = importlib.util.spec_from_file_location("dqn_prioritized", Path(__file__).resolve().parent.parent / "examples" / "dqn_prioritized.py")
    example = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(example)
    kw = dict(num_envs=64, updates=20, ring_steps=16, batch=256, warmup_steps=8, target_every=5, anneal_updates=10, hidden=16,
              log_every=0)
    first, counts, stats, (leaf, pstate) = example.train(**kw)
    second, counts2, _, (leaf2, pstate2) = example.train(**kw)
    assert counts == counts2 == (20, 0)
    assert all(torch.isfinite(p).all() for p in first) and all(np.isfinite(s).all() and s[6] > 0 for s in map(np.array, stats))
    assert example.same_bits(first, second), "two runs from the same seeds must end with the same parameter bits"
    assert torch.equal(leaf, leaf2) and torch.equal(pstate, pstate2), "and with the same leaves"
    assert pstate[1].item() == 20 and (leaf > 0).all() and leaf.unique().numel() > 50 and pstate[0].item() >= leaf.max().item()
