"""The replay ring on the device (include/ccx.h: CCX_REPLAY) against the spec (tests/_replay_spec.py) and against the library's
own rows, at the smallest shapes at which it can go wrong: 24 envs, 8 agents (16-byte row stores) and 3 agents (8-byte ones),
each on the launch shape the library picks for 24 envs (one record to a wave) and on full waves of 8 / 16 records, two waves
to a workgroup; a ring of 4 steps filled from real auto-resetting rollouts in blocks of 1, 3, 2 and 4 steps (a partly filled
ring, a block that wraps inside itself, K == S); minibatch sizes around a wave's and a workgroup's share, so that tail waves
and tail workgroups occur.  Every comparison is bit for bit."""

import numpy as np
import pytest
from _replay_spec import (AF_LIVE, AF_TERMINATED, ARRAYS, EF_RESET, draw_spec, fetch_spec, filled_spec, new_ring, push_spec, rows_spec,
                          slot_spec)
from _reset_obs_spec import make_config

pytestmark = pytest.mark.gpu

SEED = 0x0123_4567_89AB_CDEF
E, S = 24, 4
MAX_STEPS = 8                                    # of the 10 steps pushed: every env is truncated and restarted inside them
BLOCKS = (1, 3, 2, 4)
OUT_KEYS = ("obs", "next_obs", "actions", "reward", "done", "valid", "masks_next", "index")


def _bits(a) -> np.ndarray:
    a = np.ascontiguousarray(a)
    return a.view(np.uint8).reshape(a.shape + (a.itemsize,)) if a.dtype.itemsize > 1 else a


def same(got, want, msg=""):
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, (msg, got.dtype, want.dtype, got.shape, want.shape)
    np.testing.assert_array_equal(_bits(got), _bits(want), err_msg=msg)


def compact_of_rows(rows):
    """Compact records [..., N, 4] of DefaultObservation rows [..., N, L] (N >= 2): slot j >= 1 from row 0, slot 0 from row 1."""
    import torch

    N = rows.shape[-2]
    return torch.stack([rows[..., 1, 6:10]] + [rows[..., 0, 6 + 4 * j:10 + 4 * j] for j in range(1, N)], dim=-2).contiguous()


def ring_np(ring) -> dict:
    return {**{k: getattr(ring, k).cpu().numpy() for k in ARRAYS}, "state": ring.state.cpu().numpy()}


def batch_np(mb) -> dict:
    return {k: None if getattr(mb, k) is None else getattr(mb, k).cpu().numpy() for k in OUT_KEYS}


class World:
    """One batch, the blocks of real rollouts, and a ring with all of them pushed; the ring after every block is kept next
    to the spec's, and the rollouts' own ROW arrays are kept by slot (the example's ring, on the host)."""

    def __init__(self, N, shaped):
        import torch

        from collectivecrossing_amd import ReplayRing
        from collectivecrossing_amd.batched import BatchedCollectiveCrossing

        self.N = N
        b = self.batch = BatchedCollectiveCrossing(make_config(N, max_steps=MAX_STEPS), E)
        assert b.num_agents == N
        if shaped:                                                       # full waves of several records, two waves to a workgroup
            b.set_launch_shape(lanes_per_wave=64, waves_per_block=2)
        ls = b.launch_shape()
        self.per_wave = ls["lanes_per_wave"] // ls["group_lanes"]
        assert (self.per_wave > 1 and ls["waves_per_block"] == 2) if shaped else self.per_wave >= 1
        b.make_reset_pool(seed0=7, size=64)
        b.reset_from_pool()
        b.set_rng_seed(SEED)
        self.L = b.obs_len
        self.consts = tuple(float(x) for x in b.observe()[0, 0, 2:6].cpu())
        rng = np.random.default_rng(100 + N)
        self.ring = ReplayRing(b, steps=S)
        self.spec = new_ring(S, E, N)
        same(ring_np(self.ring)["actions"], self.spec["actions"])
        self.rows = dict(obs=np.zeros((S * E, N, self.L), np.float32), next_obs=np.zeros((S * E, N, self.L), np.float32))
        self.blocks, self.dev_blocks, self.after = [], [], []
        self.partial = None
        for K in BLOCKS:
            rows0 = b.observe().clone()
            obs0 = compact_of_rows(rows0)
            if self.blocks:                                              # reset_obs="next": the last compact record IS the state's
                same(obs0.cpu().numpy(), self.blocks[-1]["obs_compact"][-1], "the compact record of the current state")
            acts = self._actions(rng, K)
            traj = b.alloc_rollout(K, want_obs=True, want_compact=True, want_final=True)
            masks_last = torch.empty((E, N), dtype=torch.uint8, device="cuda")
            b.rollout(acts, auto_reset=True, reset_obs="next", out=traj, want_compact=True, masks_out=masks_last)
            # the legal set behind every step: only the last one is the rollout's own; the others are arbitrary legal bytes
            masks = torch.from_numpy(rng.integers(0, 32, size=(K, E, N), dtype=np.uint8) | 0x10).cuda()
            masks[K - 1] = masks_last
            head = int(self.spec["state"][0])
            self.ring.push(obs0, acts, traj, masks_next=masks)
            blk = dict(obs0_compact=obs0.cpu().numpy(), actions=acts.cpu().numpy(), reward=traj.reward.cpu().numpy(),
                       agent_flags=traj.agent_flags.cpu().numpy(), env_flags=traj.env_flags.cpu().numpy(),
                       obs_compact=traj.obs_compact.cpu().numpy(), final_compact=traj.final_compact.cpu().numpy(),
                       masks_next=masks.cpu().numpy())
            push_spec(self.spec, **blk)
            self.blocks.append(blk)
            self.dev_blocks.append((obs0, acts, traj, masks))
            self.after.append((ring_np(self.ring), {k: np.copy(v) for k, v in self.spec.items() if k in ARRAYS + ("state",)}))
            obs, fin, r0 = traj.obs.cpu().numpy(), traj.final_obs.cpu().numpy(), rows0.cpu().numpy()
            for s in range(K):
                for e in range(E):
                    at = slot_spec(head, s, S, E, e)
                    self.rows["obs"][at] = r0[e] if s == 0 else obs[s - 1, e]
                    self.rows["next_obs"][at] = fin[s, e] if blk["env_flags"][s, e] & EF_RESET else obs[s, e]
            if self.partial is None:                                     # head = 1: a quarter of the ring is filled
                d = int(self.ring.state[1])
                mb = self.ring.sample(300)
                self.partial = (d, batch_np(mb), {k: np.copy(v) for k, v in self.spec.items() if k in ARRAYS}, int(self.ring.state[1]))
                self.spec["state"][1] = 1                                  # (the spec's ring keeps the launch counter too)
        torch.cuda.synchronize()

    def _actions(self, rng, K):
        """u8 [K, E, N] for the next K steps: the greedy policy's action with probability 0.9, else a random one, found by a
        dry run from the current state (which is then put back) -- agents arrive and terminate inside the few steps."""
        import torch

        b = self.batch
        state = b.get_state()
        acts = torch.empty((K, E, N := self.N), dtype=torch.uint8, device="cuda")
        for s in range(K):
            rand = torch.from_numpy(rng.integers(0, 5, size=(E, N), dtype=np.uint8)).cuda()
            pick = torch.from_numpy(rng.random((E, N)) < 0.9).cuda()
            greedy = b.greedy_actions()
            acts[s] = torch.where(pick & (greedy != 255), greedy, rand)
            b.rollout(acts[s:s + 1], auto_reset=True, want_traj=False)
        b.set_state(**state)
        return acts

    def spec_ring(self, arrays=None) -> dict:
        return {**(arrays or {k: self.spec[k] for k in ARRAYS}), "S": S, "E": E, "N": self.N}

    def close(self):
        self.batch.close()


@pytest.fixture(scope="module", params=[(8, False), (8, True), (3, False), (3, True)],
                ids=["N8_even", "N8_even_full_waves", "N3_odd", "N3_odd_full_waves"])
def world(request):
    import torch

    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    w = World(*request.param)
    yield w
    w.close()


def check_batch(w, got: dict, index, spec_arrays=None, tag=""):
    want = fetch_spec(w.spec_ring(spec_arrays), index, w.consts)
    for k in OUT_KEYS:
        if got[k] is not None:
            same(got[k], want[k], f"{tag} {k}")


# ------------------------------------------------------------------------------------------------- the test's own inputs
def test_inputs_exercise_resets_dead_agents_and_terminations(world):
    ef = np.concatenate([b["env_flags"].reshape(-1) for b in world.blocks])
    af = np.concatenate([b["agent_flags"].reshape(-1) for b in world.blocks])
    assert (ef & EF_RESET).any() and not (ef & EF_RESET).all(), "no pushed (s, e) carries EF_RESET"
    assert ((af & AF_LIVE) == 0).any(), "every agent-step is live"
    assert (af & AF_TERMINATED).any(), "no agent-step is terminated"
    assert (E * world.N) % 256, "a step's (env, agent) lanes fill whole workgroups: the push has no tail"
    for b in world.blocks:                                               # final_compact differs from obs_compact where it matters
        r = (b["env_flags"] & EF_RESET) != 0
        if r.any():
            assert (b["final_compact"][r] != b["obs_compact"][r]).any()


# ------------------------------------------------------------------------------------------------- (a) push
def test_push_equals_the_spec_after_every_block(world):
    heads = np.cumsum(BLOCKS)
    for n, (got, want) in enumerate(world.after):
        for k in ARRAYS + ("state",):
            same(got[k], want[k], f"after block {n} (K = {BLOCKS[n]}): {k}")
        assert got["state"].tolist()[0] == heads[n] and got["state"].tolist()[2:] == [0, 0]
    first = world.after[0][0]
    assert (first["actions"][E:] == 255).all() and (first["masks_next"][E:] == 0x10).all() and not first["obs_c"][E:].any()


# ------------------------------------------------------------------------------------------------- (b) sample
def _share(batch) -> int:
    ls = batch.launch_shape()
    return (ls["lanes_per_wave"] // ls["group_lanes"]) * ls["waves_per_block"]


def test_sample_equals_the_spec(world):
    ring = world.ring
    share = _share(world.batch)
    F = filled_spec(int(world.spec["state"][0]), S, E)
    assert F == S * E
    sizes = sorted({1, 63, 64, 65, 300, share - 1, share, share + 1} - {0})
    print(f"N = {world.N}: a wave takes {world.per_wave} records, a workgroup {share}; B in {sizes}")
    for B in sizes:
        d = int(ring.state[1])
        mb = ring.sample(B)
        got = batch_np(mb)
        same(got["index"], draw_spec(SEED, F, d, B), f"B {B}: index")
        assert got["index"].min() >= 0 and got["index"].max() < F
        check_batch(world, got, got["index"], tag=f"B {B}:")
        assert ring.state.tolist() == [int(world.spec["state"][0]), d + 1, 0, 0]
        for k in ("obs", "next_obs"):
            assert got[k].shape == (B, world.N, world.L)


def test_sample_of_a_partly_filled_ring(world):
    d, got, arrays, draws_after = world.partial
    assert d == 0 and draws_after == 1
    same(got["index"], draw_spec(SEED, E, 0, 300), "index over F = E records")
    assert got["index"].max() < E and len(set(got["index"].tolist())) > E // 2
    check_batch(world, got, got["index"], spec_arrays=arrays, tag="partly filled:")


# ------------------------------------------------------------------------------------------------- (c) rows, by the library
def test_rows_equal_the_librarys_own(world):
    import torch

    ring, b = world.ring, world.batch
    index = torch.arange(S * E, dtype=torch.int64, device="cuda").flip(0).contiguous()
    mb = ring.fetch(index)
    same(mb.obs.cpu().numpy(), b.expand_observations(ring.obs_c[index]).cpu().numpy(), "obs against expand_observations")
    same(mb.next_obs.cpu().numpy(), b.expand_observations(ring.next_c[index]).cpu().numpy(), "next_obs against expand_observations")
    at = index.cpu().numpy()
    same(mb.obs.cpu().numpy(), world.rows["obs"][at], "obs against the rows the rollouts wrote")
    same(mb.next_obs.cpu().numpy(), world.rows["next_obs"][at], "next_obs against where(reset, final_obs, obs)")
    same(mb.obs.cpu().numpy(), rows_spec(world.spec["obs_c"][at], world.consts), "obs against the restated layout")
    same(mb.index.cpu().numpy(), at)
    d = int(ring.state[1])
    drawn = ring.sample(65)
    same(drawn.obs.cpu().numpy(), b.expand_observations(ring.obs_c[drawn.index]).cpu().numpy())
    same(drawn.next_obs.cpu().numpy(), world.rows["next_obs"][drawn.index.cpu().numpy()])
    assert int(ring.state[1]) == d + 1


# ------------------------------------------------------------------------------------------------- (d) the empty record
def _prefilled(ring, B, **kw):
    import torch

    out = ring.alloc_batch(B, **kw)
    for k in OUT_KEYS:
        if getattr(out, k) is not None:
            getattr(out, k).view(torch.uint8).fill_(0xCD)
    return out


def test_indices_outside_the_ring_and_empty_slots(world):
    import torch

    from collectivecrossing_amd import ReplayRing

    b = world.batch
    ring = ReplayRing(b, steps=S)
    empty = fetch_spec(world.spec_ring(new_ring(S, E, world.N)), np.array([0], np.int64), world.consts)
    # an empty ring: every draw is -1
    out = _prefilled(ring, 65)
    mb = ring.sample(65, out=out)
    got = batch_np(mb)
    assert mb is out and (got["index"] == -1).all() and ring.state.tolist() == [0, 1, 0, 0]
    for k in OUT_KEYS[:-1]:
        same(got[k], np.broadcast_to(empty[k], got[k].shape), f"empty ring: {k}")
    assert (got["actions"] == 255).all() and (got["masks_next"] == 0x10).all() and not got["valid"].any()
    assert not _bits(got["reward"]).any()                                # +0.0
    same(got["obs"][0], rows_spec(np.zeros((world.N, 4), np.float32), world.consts))
    # one block of one step: F = E of R = 4 E records
    obs0, acts, traj, masks = world.dev_blocks[0]
    ring.push(obs0, acts, traj, masks_next=masks)
    R, F = S * E, E
    idx = np.array([-1, R, 1 << 40, F + 5, 3, R - 1, -(1 << 62), F, F - 1], np.int64)
    out = _prefilled(ring, len(idx))
    mb = ring.fetch(torch.from_numpy(idx).cuda(), out=out)
    got = batch_np(mb)
    assert ring.state.tolist() == [1, 1, 0, 0]                           # fetch leaves draws alone
    check_batch(world, got, idx, spec_arrays=world.after[0][1], tag="fetch:")
    for n in (0, 1, 2, 3, 5, 6, 7):
        for k in OUT_KEYS[:-1]:
            same(got[k][n], empty[k][0], f"index {idx[n]}: {k}")
    assert (got["actions"][4] != 255).any() and (got["actions"][8] != 255).any()
    same(got["index"], idx)


# ------------------------------------------------------------------------------------------------- (e) optional rows
def test_absent_row_outputs(world):
    ring = world.ring
    index = ring.sample(64).index
    full = batch_np(ring.fetch(index))
    for want_obs, want_next in ((False, True), (True, False), (False, False)):
        mb = ring.fetch(index, want_obs=want_obs, want_next_obs=want_next)
        assert (mb.obs is None) == (not want_obs) and (mb.next_obs is None) == (not want_next)
        got = batch_np(mb)
        for k in OUT_KEYS:
            if got[k] is not None:
                same(got[k], full[k], f"want_obs {want_obs} want_next_obs {want_next}: {k}")
        d = int(ring.state[1])
        drawn = ring.sample(64, out=_prefilled(ring, 64, want_obs=want_obs, want_next_obs=want_next))
        assert (drawn.obs is None) == (not want_obs) and (drawn.next_obs is None) == (not want_next)
        check_batch(world, batch_np(drawn), draw_spec(SEED, S * E, d, 64), tag="sample with absent rows:")


# ------------------------------------------------------------------------------------------------- (f) captured
def test_captured_push_and_sample_advance_with_every_replay(world):
    import torch

    from collectivecrossing_amd import ReplayRing
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
            twin, eager = ReplayRing(b, steps=S), []
            for f in feeds:
                twin.push(f[0], f[1], tuple(f[2:7]), masks_next=f[7])
                eager.append(batch_np(twin.sample(B)))
            ring = ReplayRing(b, steps=S)
            static = [torch.empty_like(t) for t in feeds[0]]
            out = ring.alloc_batch(B)
            traj = RolloutResult(None, static[2], static[3], static[4], obs_compact=static[5], final_compact=static[6])
            side.synchronize()
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph, stream=side):
                ring.push(static[0], static[1], traj, masks_next=static[7])
                ring.sample(B, out=out)
            side.synchronize()
            assert ring.state.tolist() == [0, 0, 0, 0]                    # capturing ran nothing
            for n, f in enumerate(feeds):
                for dst, src in zip(static, f):
                    dst.copy_(src)
                graph.replay()
                side.synchronize()
                got = batch_np(out)
                for k in OUT_KEYS:
                    same(got[k], eager[n][k], f"replay {n}: {k}")
                assert ring.state.tolist() == [K * (n + 1), n + 1, 0, 0]
            want, got = ring_np(twin), ring_np(ring)
            for k in ARRAYS + ("state",):
                same(got[k], want[k], f"ring after three replays: {k}")
            assert len({tuple(e["index"].tolist()) for e in eager}) == 3
    finally:
        torch.cuda.synchronize()
        b.use_stream(None)


# ------------------------------------------------------------------------------------------------- (g) checkpoints
def test_state_dict_round_trip(world):
    from collectivecrossing_amd import ReplayRing

    ring = world.ring
    sd = ring.state_dict()
    assert sd["geometry"] == (S, E, world.N) and sd["state"].tolist() == ring.state.tolist()
    other = ReplayRing(world.batch, steps=S)
    other.load_state_dict(sd)
    a, b = batch_np(ring.sample(300)), batch_np(other.sample(300))
    for k in OUT_KEYS:
        same(a[k], b[k], k)
    assert other.state.tolist() == ring.state.tolist()
    with pytest.raises(ValueError):
        ReplayRing(world.batch, steps=S + 1).load_state_dict(sd)
    with pytest.raises(ValueError):
        other.load_state_dict({k: v for k, v in sd.items() if k != "reward"})
    other.clear()
    fresh = ring_np(ReplayRing(world.batch, steps=S))
    for k, v in ring_np(other).items():
        same(v, fresh[k], f"clear: {k}")


# ------------------------------------------------------------------------------------------------- (h) into the TD loss
def test_minibatch_drops_into_td_loss(world):
    import torch

    from collectivecrossing_amd import QLearning

    B, N = 64, world.N
    mb = world.ring.sample(B)
    ql = QLearning(world.batch)
    g = torch.Generator(device="cuda").manual_seed(1)
    q, qt = (torch.randn((B, N, 5), device="cuda", generator=g) for _ in range(2))
    r = ql.td_loss(q, mb.actions, mb.reward, mb.done, qt, None, mb.masks_next, valid=mb.valid, want_td_error=True)
    stats = r.stats.tolist()
    counts = ((mb.valid != 0) & (mb.actions <= 4)).sum().item()
    assert stats[6] == counts > 0 and stats[7] == 0 and np.isfinite(stats).all()


# ------------------------------------------------------------------------------------------------- the refusals
def test_refusals(world):
    import torch

    from collectivecrossing_amd import ReplayRing

    b, ring, N = world.batch, world.ring, world.N
    obs0, acts, traj, masks = world.dev_blocks[1]                        # K = 3
    before = ring_np(ring)
    bad = [lambda: ReplayRing(b, steps=0), lambda: ReplayRing(object(), steps=4), lambda: ReplayRing(b, steps=(1 << 31) // E + 1),
           lambda: ring.push(obs0, torch.cat([acts, acts]), traj),                        # K = 6 > S
           lambda: ring.push(obs0, acts.to(torch.int64), traj),
           lambda: ring.push(obs0.cpu(), acts, traj),
           lambda: ring.push(torch.empty(E * N * 4 + 1, device="cuda")[1:].view(E, N, 4), acts, traj),   # not 16-byte aligned
           lambda: ring.push(obs0, acts, (traj.reward, traj.agent_flags, traj.env_flags)),
           lambda: ring.push(obs0, acts, (traj.reward.float(), traj.agent_flags, traj.env_flags, traj.obs_compact)),
           lambda: ring.push(obs0, acts, traj, masks_next=masks[:2]),
           lambda: ring.push(obs0, acts.transpose(1, 2).contiguous().transpose(1, 2), traj),
           lambda: ring.sample(0), lambda: ring.sample(64, out=ring.alloc_batch(65)), lambda: ring.sample(64, out=object()),
           lambda: ring.sample((1 << 31) // N + 1),
           lambda: ring.fetch(torch.zeros(4, dtype=torch.int32, device="cuda")),
           lambda: ring.fetch(torch.zeros((4, 1), dtype=torch.int64, device="cuda")),
           lambda: ring.fetch(torch.zeros(0, dtype=torch.int64, device="cuda")),
           lambda: ring.fetch(torch.zeros(4, dtype=torch.int64, device="cuda"), out=ring.alloc_batch(5))]
    for n, call in enumerate(bad):
        with pytest.raises(ValueError):
            call()
            pytest.fail(f"refusal {n} did not raise")
    torch.cuda.synchronize()
    for k, v in ring_np(ring).items():
        same(v, before[k], f"a refused call changed {k}")
