"""N-step targets on the device (include/ccx.h: CCX_NSTEP) against the spec (tests/_nstep_spec.py), bit for bit, at the shapes
of tests/test_gpu_replay.py: 24 envs, 8 agents (16-byte row stores) and 3 agents (8-byte ones), each on the launch shape the
library picks for 24 envs (one record to a wave) and on full waves of 8 / 16 records; a ring of 6 steps filled from real
auto-resetting rollouts of the scripted policy in blocks of 1, 3, 2 and 4 steps, so that it wraps and is rewritten, with
episodes that end inside windows and agents that finish at different steps.  After every block every record is fetched once,
plus -1, R and duplicates, for n in {1, 2, 3, 5, 6} and gamma in {0.99, 1.0, 0.0}."""

import numpy as np
import pytest
from _nstep_cases import BLOCKS, CAUSES, E, EPSILON, GAMMAS, NS, POOL, S, config, count_causes, stagger, synthetic, synthetic_states
from _nstep_spec import cut_push_spec, mark_cut_spec, new_cut, nstep_fetch_spec
from _replay_spec import ARRAYS, draw_spec, filled_spec, new_ring, push_spec
from test_gpu_replay import batch_np, compact_of_rows, ring_np, same

pytestmark = pytest.mark.gpu

SEED = 0x0123_4567_89AB_CDEF
R = S * E
OUT_KEYS = ("obs", "next_obs", "actions", "reward", "done", "valid", "masks_next", "index")
INDEX = np.concatenate([np.arange(R), [-1, R, 5, 5, R - 1, 1 << 40]]).astype(np.int64)      # 150 records: no multiple of 8 or 16


def nbatch_np(mb) -> dict:
    return {**batch_np(mb.batch), "discount": mb.discount.cpu().numpy(), "span": mb.span.cpu().numpy()}


def check(got: dict, want: dict, tag=""):
    for k in OUT_KEYS + ("discount", "span"):
        if got[k] is not None:
            same(got[k], want[k], f"{tag} {k}")


class World:
    """One batch, the blocks of real rollouts, an NStepReplay with all of them pushed and a plain twin ring pushed alongside;
    after every block the device's ring and cut bytes, the spec's, and the fetches of every (n, gamma) are kept."""

    def __init__(self, N, shaped):
        import torch

        from collectivecrossing_amd import NStepReplay, ReplayRing
        from collectivecrossing_amd.batched import BatchedCollectiveCrossing
        from collectivecrossing_amd.reset import build_reset_pool

        self.N = N
        cfg = config(N)
        b = self.batch = BatchedCollectiveCrossing(cfg, E)
        if shaped:
            b.set_launch_shape(lanes_per_wave=64, waves_per_block=2)
        ls = b.launch_shape()
        self.per_wave = ls["lanes_per_wave"] // ls["group_lanes"]
        assert (self.per_wave > 1 and ls["waves_per_block"] == 2) if shaped else self.per_wave >= 1
        b.set_reset_pool(build_reset_pool(cfg, POOL["seed0"], POOL["size"]))
        b.reset_from_pool()
        b.set_state(step_count=stagger(E))
        b.set_rng_seed(SEED)
        b.set_policy_epsilon(EPSILON)
        self.consts = tuple(float(x) for x in b.observe()[0, 0, 2:6].cpu())
        rng = np.random.default_rng(200 + N)
        self.ns = NStepReplay(ReplayRing(b, steps=S), n=3, gamma=0.99)
        self.plain = ReplayRing(b, steps=S)
        self.spec, self.cut = new_ring(S, E, N), new_cut(S, E)
        self.after, self.dev_blocks, self.fetched = [], [], []
        index = torch.from_numpy(INDEX).cuda()
        for K in BLOCKS:
            obs0 = compact_of_rows(b.observe().clone())
            state = b.get_state()
            _, acts = b.rollout_greedy(K, auto_reset=True, want_obs=False)       # the scripted policy's actions, by a dry run
            b.set_state(**state)
            traj = b.alloc_rollout(K, want_obs=True, want_compact=True, want_final=True)
            masks_last = torch.empty((E, N), dtype=torch.uint8, device="cuda")
            b.rollout(acts, auto_reset=True, reset_obs="next", out=traj, want_compact=True, masks_out=masks_last)
            masks = torch.from_numpy(rng.integers(0, 32, size=(K, E, N), dtype=np.uint8) | 0x10).cuda()
            masks[K - 1] = masks_last
            self.ns.push(obs0, acts, traj, masks_next=masks)
            self.plain.push(obs0, acts, traj, masks_next=masks)
            blk = dict(obs0_compact=obs0.cpu().numpy(), actions=acts.cpu().numpy(), reward=traj.reward.cpu().numpy(),
                       agent_flags=traj.agent_flags.cpu().numpy(), env_flags=traj.env_flags.cpu().numpy(),
                       obs_compact=traj.obs_compact.cpu().numpy(), final_compact=traj.final_compact.cpu().numpy(),
                       masks_next=masks.cpu().numpy())
            push_spec(self.spec, **blk)
            cut_push_spec(self.cut, int(self.spec["state"][0]), S, E, blk["env_flags"])
            self.dev_blocks.append((obs0, acts, traj, masks))
            snap = {k: np.copy(v) for k, v in self.spec.items() if k in ARRAYS + ("state",)}
            self.after.append((ring_np(self.ns.ring), self.ns.cut.cpu().numpy(), {**snap, "S": S, "E": E, "N": N}, self.cut.copy()))
            got = {}
            for n in NS:
                for gamma in GAMMAS:
                    self.ns.n, self.ns.gamma = n, gamma
                    got[n, gamma] = (nbatch_np(self.ns.fetch(index)), nbatch_np(self.ns.fetch(index[77:78].contiguous())))
            got["plain"] = batch_np(self.plain.fetch(index))
            self.fetched.append(got)
        self.ns.n, self.ns.gamma = 3, 0.99
        torch.cuda.synchronize()

    def close(self):
        self.batch.set_policy_epsilon(0.0)
        self.batch.close()


@pytest.fixture(scope="module", params=[(8, False), (8, True), (3, False), (3, True)],
                ids=["N8_even", "N8_even_full_waves", "N3_odd", "N3_odd_full_waves"])
def world(request):
    import torch

    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    w = World(*request.param)
    yield w
    w.close()


# ------------------------------------------------------------------------------------------------- the test's own inputs
def test_inputs_hold_every_ending(world):
    total = dict.fromkeys(CAUSES, 0)
    for _ring, _cut, spec, cut in world.after:
        for k, v in count_causes(spec, cut, INDEX, 3).items():
            total[k] += v
    print(f"N = {world.N}: a wave takes {world.per_wave} records; windows of n = 3 ended by {total}")
    for k in CAUSES:
        assert total[k] > 0, (k, total)
    assert len(INDEX) % world.per_wave or world.per_wave == 1


# ------------------------------------------------------------------------------------------------- (a) the cut bytes
def test_push_marks_the_cuts_after_every_block(world):
    for n, (ring, cut, spec, want) in enumerate(world.after):
        same(cut, want, f"after block {n}: cut")
        for k in ARRAYS + ("state",):
            same(ring[k], spec[k], f"after block {n}: {k}")
    assert world.after[-1][3].any() and not world.after[-1][3].all()


# ------------------------------------------------------------------------------------------------- (b) fetch
def test_fetch_equals_the_spec_after_every_block(world):
    for blk, (_ring, _cut, spec, cut) in enumerate(world.after):
        for n in NS:
            for gamma in GAMMAS:
                full, one = world.fetched[blk][n, gamma]
                check(full, nstep_fetch_spec(spec, cut, INDEX, n, gamma, world.consts), f"block {blk} n {n} gamma {gamma}:")
                check(one, nstep_fetch_spec(spec, cut, INDEX[77:78], n, gamma, world.consts), f"block {blk} n {n} gamma {gamma} B = 1:")


def test_n1_has_the_bits_of_the_rings_own_fetch(world):
    for blk, got in enumerate(world.fetched):
        for gamma in GAMMAS:
            full, _ = got[1, gamma]
            for k in OUT_KEYS:
                same(full[k], got["plain"][k], f"block {blk} gamma {gamma}: {k}")
            assert (full["span"] == 1).all() and (full["discount"] == np.float32(gamma)).all()


# ------------------------------------------------------------------------------------------------- (c) sample
def test_sample_names_the_records_the_ring_names(world):
    ns, plain = world.ns, world.plain
    _ring, _cut, spec, cut = world.after[-1]
    for B in (1, 65, 150):
        d = int(ns.ring.state[1])
        assert int(plain.state[1]) == d
        a, p = ns.sample(B), plain.sample(B)
        got = nbatch_np(a)
        same(got["index"], p.index.cpu().numpy(), f"B {B}: index against ReplayRing.sample")
        same(got["index"], draw_spec(SEED, filled_spec(int(spec["state"][0]), S, E), d, B), f"B {B}: index against the spec")
        check(got, nstep_fetch_spec(spec, cut, got["index"], 3, 0.99, world.consts), f"sample B {B}:")
        assert ns.ring.state.tolist() == [int(spec["state"][0]), d + 1, 0, 0]


def test_absent_row_outputs_leave_the_other_arrays_their_bits(world):
    """Every array still present has the bits of the full fetch, whichever of the two row outputs is left out: a lone record
    in a wave (B = 1), and several waves with a one-record tail (B = 65 = 4 * 16 + 1 = 8 * 8 + 1), records outside the ring
    among them."""
    import torch

    ns = world.ns
    assert len(INDEX[-65:]) == 65 and (65 % world.per_wave == 1 or world.per_wave == 1)
    for idx in (INDEX[77:78], INDEX[-65:]):
        index = torch.from_numpy(idx).cuda()
        full = nbatch_np(ns.fetch(index))
        assert full["obs"] is not None and full["next_obs"] is not None
        for want_obs, want_next in ((False, True), (True, False), (False, False)):
            mb = ns.fetch(index, want_obs=want_obs, want_next_obs=want_next)
            assert (mb.batch.obs is None) == (not want_obs) and (mb.batch.next_obs is None) == (not want_next)
            check(nbatch_np(mb), full, f"B {len(idx)} want_obs {want_obs} want_next_obs {want_next}:")


# ------------------------------------------------------------------------------------------------- (d) a manual cut
def test_mark_cut_equals_the_spec(world):
    import torch

    from collectivecrossing_amd import NStepReplay, ReplayRing

    b = world.batch
    ns = NStepReplay(ReplayRing(b, steps=S), n=3, gamma=0.99)
    want = new_cut(S, E)
    ns.mark_cut()                                                        # an empty ring: nothing
    same(ns.cut.cpu().numpy(), want)
    mask = (np.arange(E) % 3 == 0).astype(np.uint8) * 7
    head = 0
    for (obs0, acts, traj, masks), m in zip(world.dev_blocks, (mask, None, mask[::-1].copy(), None)):
        ns.push(obs0, acts, traj, masks_next=masks)
        head += acts.shape[0]
        cut_push_spec(want, head, S, E, traj.env_flags.cpu().numpy())
        ns.mark_cut(None if m is None else torch.from_numpy(m).cuda())
        mark_cut_spec(want, head, S, E, m)
        same(ns.cut.cpu().numpy(), want, f"head {head}")
    spec = world.after[-1][2]
    check(nbatch_np(ns.fetch(torch.from_numpy(INDEX).cuda())), nstep_fetch_spec(spec, want, INDEX, 3, 0.99, world.consts), "after mark_cut:")
    sd = ns.state_dict()
    other = NStepReplay(ReplayRing(b, steps=S), n=2, gamma=0.5)
    other.load_state_dict(sd)
    assert (other.n, other.gamma) == (3, ns.gamma)
    check(nbatch_np(other.fetch(torch.from_numpy(INDEX).cuda())), nstep_fetch_spec(spec, want, INDEX, 3, 0.99, world.consts), "loaded:")
    other.clear()
    assert not other.cut.any() and other.ring.state.tolist() == [0, 0, 0, 0]


# ------------------------------------------------------------------------------------------------- (e) the synthetic ring
def test_synthetic_ring_on_the_device():
    import torch

    from collectivecrossing_amd import NStepReplay, ReplayRing
    from collectivecrossing_amd.batched import BatchedCollectiveCrossing

    spec, cut, where = synthetic(N=3)
    b = BatchedCollectiveCrossing(config(3), spec["E"])
    try:
        consts = tuple(float(x) for x in b.observe()[0, 0, 2:6].cpu())
        ns = NStepReplay(ReplayRing(b, steps=spec["S"]), n=3, gamma=0.5)
        for k in ARRAYS:
            getattr(ns.ring, k).copy_(torch.from_numpy(spec[k]))
        ns.cut.copy_(torch.from_numpy(cut))
        Rs = spec["S"] * spec["E"]
        idx = np.array([-1, Rs] + list(range(Rs)) + [where["dropped"]], np.int64)
        for head, what in synthetic_states():
            spec["state"][0] = head
            ns.ring.state.copy_(torch.from_numpy(spec["state"]))
            for n in (1, 2, 3, 5):
                ns.n = n
                check(nbatch_np(ns.fetch(torch.from_numpy(idx).cuda())), nstep_fetch_spec(spec, cut, idx, n, 0.5, consts), f"{what} n {n}:")
        spec["state"][0] = 7
        ns.ring.state.copy_(torch.from_numpy(spec["state"]))
        ns.n = 3
        got = nbatch_np(ns.fetch(torch.tensor([where["agent_early"], where["nan_just_beyond"]], device="cuda")))
        assert got["span"][0].tolist() == [1, 1, 3] and got["valid"][0].tolist() == [4, 0, 4] and np.isnan(got["reward"][0, 2])
        assert not np.isnan(got["reward"][1]).any()
    finally:
        b.close()


# ------------------------------------------------------------------------------------------------- (e2) the longest window
def test_the_longest_window_on_the_device():
    """n = 16 (CCX_NSTEP_MAX) and the sizes between 8 and 16 on a ring of 32 steps: the upper half of the unrolled window."""
    import torch

    from collectivecrossing_amd import NStepReplay, ReplayRing
    from collectivecrossing_amd.batched import BatchedCollectiveCrossing

    S_, E_, N = 32, 5, 3
    b = BatchedCollectiveCrossing(config(N), E_)
    try:
        consts = tuple(float(x) for x in b.observe()[0, 0, 2:6].cpu())
        rng = np.random.default_rng(16)
        spec, R_ = new_ring(S_, E_, N), S_ * E_
        spec["reward"][:] = rng.standard_normal((R_, N))
        spec["actions"][:] = rng.integers(0, 5, (R_, N), dtype=np.uint8)
        spec["done"][:] = rng.random((R_, N)) < 0.03
        spec["valid"][:] = (rng.random((R_, N)) < 0.97) * 4
        spec["masks_next"][:] = rng.integers(0, 16, (R_, N), dtype=np.uint8) | 0x10
        spec["obs_c"][:] = rng.standard_normal((R_, N, 4)).astype(np.float32)
        spec["next_c"][:] = rng.standard_normal((R_, N, 4)).astype(np.float32)
        cut = ((rng.random(R_) < 0.04) * rng.integers(1, 256, R_)).astype(np.uint8)
        ns = NStepReplay(ReplayRing(b, steps=S_), n=16, gamma=0.99)
        for k in ARRAYS:
            getattr(ns.ring, k).copy_(torch.from_numpy(spec[k]))
        ns.cut.copy_(torch.from_numpy(cut))
        idx = np.concatenate([np.arange(R_), [-1, R_, 7]]).astype(np.int64)
        longest = 0
        for head in (S_ + 11, S_, 20):
            spec["state"][0] = head
            ns.ring.state.copy_(torch.from_numpy(spec["state"]))
            for n in (16, 15, 12, 9):
                ns.n = n
                want = nstep_fetch_spec(spec, cut, idx, n, 0.99, consts)
                check(nbatch_np(ns.fetch(torch.from_numpy(idx).cuda())), want, f"head {head} n {n}:")
                longest = max(longest, int(want["span"].max()))
        assert longest == 16                                             # a window of all sixteen steps occurs
    finally:
        b.close()


# ------------------------------------------------------------------------------------------------- (f) captured
def test_captured_push_and_sample_advance_with_every_replay(world):
    import torch

    from collectivecrossing_amd import NStepReplay, ReplayRing
    from collectivecrossing_amd.batched import RolloutResult

    b, K, B = world.batch, 2, 65
    side = torch.cuda.Stream()
    b.use_stream(side)
    torch.cuda.synchronize()
    try:
        with torch.cuda.stream(side):
            feeds = []
            for obs0, acts, traj, masks in world.dev_blocks[1:]:        # blocks of 3, 2 and 4 steps: their first two
                feeds.append((obs0, acts[:K].contiguous(), traj.reward[:K].contiguous(), traj.agent_flags[:K].contiguous(),
                              traj.env_flags[:K].contiguous(), traj.obs_compact[:K].contiguous(), traj.final_compact[:K].contiguous(),
                              masks[:K].contiguous()))
            twin, eager = NStepReplay(ReplayRing(b, steps=S), n=3, gamma=0.99), []
            for f in feeds:
                twin.push(f[0], f[1], tuple(f[2:7]), masks_next=f[7])
                eager.append(nbatch_np(twin.sample(B)))
            ns = NStepReplay(ReplayRing(b, steps=S), n=3, gamma=0.99)
            static = [torch.empty_like(t) for t in feeds[0]]
            out = ns.alloc_batch(B)
            traj = RolloutResult(None, static[2], static[3], static[4], obs_compact=static[5], final_compact=static[6])
            side.synchronize()
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph, stream=side):
                ns.push(static[0], static[1], traj, masks_next=static[7])
                ns.sample(B, out=out)
            side.synchronize()
            assert ns.ring.state.tolist() == [0, 0, 0, 0] and not ns.cut.any()     # capturing ran nothing
            for n, f in enumerate(feeds):
                for dst, src in zip(static, f):
                    dst.copy_(src)
                graph.replay()
                side.synchronize()
                check(nbatch_np(out), eager[n], f"replay {n}:")
                assert ns.ring.state.tolist() == [K * (n + 1), n + 1, 0, 0]
            same(ns.cut.cpu().numpy(), twin.cut.cpu().numpy(), "cut after three replays")
            assert (eager[-1]["span"] > 1).any() and len({tuple(e["index"].tolist()) for e in eager}) == 3
    finally:
        torch.cuda.synchronize()
        b.use_stream(None)


# ------------------------------------------------------------------------------------------------- the refusals
def test_refusals(world):
    import torch

    from collectivecrossing_amd import NStepReplay, ReplayRing

    b, ns, N = world.batch, world.ns, world.N
    index = torch.from_numpy(INDEX).cuda()
    before = ns.cut.clone()
    bad = [lambda: NStepReplay(object()), lambda: NStepReplay(ns.ring, n=0), lambda: NStepReplay(ns.ring, n=S + 1),
           lambda: NStepReplay(ReplayRing(b, steps=32), n=17), lambda: NStepReplay(ns.ring, n=2.5),
           lambda: NStepReplay(ns.ring, gamma=1.5), lambda: NStepReplay(ns.ring, gamma=float("nan")), lambda: NStepReplay(ns.ring, gamma="x"),
           lambda: ns.fetch(index.to(torch.int32)), lambda: ns.fetch(index[:0]), lambda: ns.fetch(index.cpu()),
           lambda: ns.fetch(index, out=ns.alloc_batch(5)), lambda: ns.fetch(index, out=ns.ring.alloc_batch(len(INDEX))),
           lambda: ns.sample(0), lambda: ns.sample(64, out=ns.alloc_batch(65)), lambda: ns.sample((1 << 31) // N + 1),
           lambda: ns.mark_cut(torch.zeros(E + 1, dtype=torch.uint8, device="cuda")),
           lambda: ns.mark_cut(torch.zeros(E, dtype=torch.int32, device="cuda")),
           lambda: ns.push(world.dev_blocks[1][0], world.dev_blocks[1][1].to(torch.int64), world.dev_blocks[1][2]),
           lambda: ns.load_state_dict({"cut": ns.cut})]
    for n, call in enumerate(bad):
        with pytest.raises(ValueError):
            call()
            pytest.fail(f"refusal {n} did not raise")
    out = ns.alloc_batch(len(INDEX))
    out.discount = out.discount.double()
    with pytest.raises(ValueError):
        ns.fetch(index, out=out)
    assert NStepReplay(ReplayRing(b, steps=32), n=16).n == 16
    torch.cuda.synchronize()
    same(ns.cut.cpu().numpy(), before.cpu().numpy(), "a refused call changed cut")
