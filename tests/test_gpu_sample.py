"""Masked categorical sampling on the device (include/ccx.h: CCX_SAMPLE) against the NumPy spec (tests/_sample_spec.py):
adversarial cases on shapes that cross every boundary of the kernel's layout, every output element written, the state and
the key (far shards, shard invariance, the seed), a real actor loop eager and captured, and the refusals.  f32 values are
compared as bit patterns throughout."""

import itertools

import numpy as np
import pytest
from _far_shard_cases import EP_ABOVE_2_16, EP_BIG_RESIDUE, EP_LATE
from _reset_obs_spec import make_config
from _sample_spec import bits32, make_sample_case, reference_f64, sample_spec

pytestmark = pytest.mark.gpu

# E x N slots: one slot (a single partial 16-byte piece behind the last whole one), 63 / 64 / 65 slots around one wave, 536
# (eight full waves and a tail of 24), 6500 (5 E N a multiple of 4: no partial piece; 50 agents: envs straddle waves)
SHAPES = ((1, 1), (21, 3), (8, 8), (5, 13), (67, 8), (130, 50))
SEED = 0x0123_4567_89AB_CDEF
MODES = tuple(itertools.product((True, False), (False, True)))          # (masked, deterministic)
SENTINEL = 0xEE


@pytest.fixture(scope="module")
def batches():
    import torch

    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    from collectivecrossing_amd.batched import BatchedCollectiveCrossing

    made = []

    def new(N, E, **kw):
        b = BatchedCollectiveCrossing(make_config(N, max_steps=12), E, **kw)
        assert b.num_agents == N
        made.append(b)
        return b

    yield new
    for b in made:
        b.close()


def _late(case):
    """The generator's case with the late episode counters of tests/_far_shard_cases.py at its first envs."""
    ep = case["episode"].copy()
    late = np.array([EP_LATE, EP_ABOVE_2_16, EP_BIG_RESIDUE, (1 << 31) - 1], np.int64)[: len(ep)]
    ep[: len(late)] = late.astype(np.int32)
    return dict(case, episode=ep)


@pytest.fixture(scope="module")
def cases():
    """A generator case and the spec's answers in the four modes, made once per shape and env_offset."""
    cache = {}

    def get(E, N, env_offset=0):
        if (E, N, env_offset) not in cache:
            case = _late(make_sample_case(E, N, seed=E * 100 + N))
            want = {(masked, det): sample_spec(case["logits_masked"] if masked else case["logits"],
                                               case["masks"] if masked else None, case["terminated"], case["truncated"],
                                               case["step_count"], case["episode"], env_offset=env_offset, seed=SEED,
                                               deterministic=det) for masked, det in MODES}
            cache[E, N, env_offset] = (case, want)
        return cache[E, N, env_offset]

    return get


def _load(batch, case):
    import torch

    batch.set_state(terminated=case["terminated"], truncated=case["truncated"], step_count=case["step_count"],
                    episode=case["episode"])
    batch.set_rng_seed(SEED)
    return {k: torch.from_numpy(np.ascontiguousarray(case[k])).cuda() for k in ("logits", "logits_masked", "masks")}


def _run(batch, d, masked, det, logp=True, entropy=True, prefill=True):
    import torch

    out = batch.alloc_sample(want_logp=logp, want_entropy=entropy)
    if prefill:
        for t in (out.actions, out.logp, out.entropy):
            if t is not None:
                t.view(torch.uint8).fill_(SENTINEL)
        torch.cuda.synchronize()
    got = batch.sample_actions(d["logits_masked"] if masked else d["logits"], d["masks"] if masked else None,
                               deterministic=det, out=out)
    assert got is out
    batch.synchronize()
    return tuple(None if t is None else t.cpu().numpy() for t in (out.actions, out.logp, out.entropy))


def _assert_equal(got, want, tag):
    for g, w, name in zip(got, want, ("actions", "logp", "entropy")):
        if g is not None:
            np.testing.assert_array_equal(bits32(g), bits32(w), err_msg=f"{name} {tag}")


def _expected_change(case):
    """The expected share of slots in which two independent draws of the rule give different actions: 1 - sum_k p_k^2 for a
    live slot, p the f64 softmax over its legal set (a degenerate slot: uniform over that set), and 0 for a dead one.  The
    generator's peaked, single-action and dead slots keep it near 0.2.  The tests ask for half of it: the number of changed
    slots is a sum of independent Bernoulli draws, its standard deviation at most sqrt(E N) / 2 (12 for the 536 slots used
    here against a mean above 100), so half the mean lies more than four standard deviations below the mean."""
    lp, _ = reference_f64(case["logits_masked"], case["masks"])
    legal = (((case["masks"][..., None] | 0x10) >> np.arange(5, dtype=np.uint8)) & 1).astype(bool)
    degenerate = np.isnan(lp).any(-1, keepdims=True)
    p = np.where(degenerate, legal / legal.sum(-1, keepdims=True), np.where(legal, np.exp(lp), 0.0))
    np.testing.assert_allclose(p.sum(-1), 1.0, atol=1e-12)
    live = (case["terminated"] | case["truncated"]) == 0
    return float(np.where(live, 1.0 - (p * p).sum(-1), 0.0).mean())


# ------------------------------------------------------------------------------------------------- 1. bits against the spec
@pytest.mark.parametrize("E,N", SHAPES)
def test_bits_against_the_spec_every_element_written(batches, cases, E, N):
    batch = batches(N, E)
    case, want = cases(E, N)
    d = _load(batch, case)
    for masked, det in MODES:
        for logp, entropy in ((True, True), (True, False), (False, True), (False, False)):
            got = _run(batch, d, masked, det, logp, entropy)                         # outputs prefilled with 0xEE bytes
            assert (got[1] is None) == (not logp) and (got[2] is None) == (not entropy)
            _assert_equal(got, want[masked, det], f"E {E} N {N} masked {masked} det {det} logp {logp} entropy {entropy}")
    dead = (case["terminated"] | case["truncated"]) != 0
    acts, lp, ent = want[True, False]
    assert (acts[dead] == 255).all() and not bits32(lp)[dead].any() and not bits32(ent)[dead].any()
    assert E * N < 64 or (dead.any() and not dead.all())
    assert not np.isnan(lp).any() and not np.isnan(ent).any() and (E * N < 64 or np.isnan(case["logits_masked"]).any())
    # the default call: logp without entropy, fresh tensors
    res = batch.sample_actions(d["logits_masked"], d["masks"])
    batch.synchronize()
    assert res.entropy is None
    _assert_equal((res.actions.cpu().numpy(), res.logp.cpu().numpy(), None), want[True, False], "defaults")


# ------------------------------------------------------------------------------------------------- 2. the state
def test_the_draw_follows_the_state(batches, cases):
    E, N = 67, 8
    batch = batches(N, E)
    case, want = cases(E, N)
    d = _load(batch, case)
    _assert_equal(_run(batch, d, True, False), want[True, False], "start state")
    # other counters in some envs, other dead slots in others: the outputs change there and nowhere else
    moved = dict(case)
    moved["step_count"] = case["step_count"].copy()
    moved["step_count"][10:20] += 1
    moved["episode"] = case["episode"].copy()
    moved["episode"][20:30] = np.array([EP_LATE, EP_ABOVE_2_16, EP_BIG_RESIDUE] * 4, np.int64)[:10].astype(np.int32) + 1
    moved["terminated"] = case["terminated"].copy()
    moved["terminated"][30:40] ^= 1
    moved["truncated"] = case["truncated"].copy()
    moved["truncated"][40:50, ::2] = 1
    spec = sample_spec(moved["logits_masked"], moved["masks"], moved["terminated"], moved["truncated"], moved["step_count"],
                       moved["episode"], seed=SEED)
    batch.set_state(terminated=moved["terminated"], truncated=moved["truncated"], step_count=moved["step_count"],
                    episode=moved["episode"])
    got = _run(batch, d, True, False)
    _assert_equal(got, spec, "moved state")
    changed = (got[0] != want[True, False][0]).any(-1)
    assert not changed[:10].any() and not changed[50:].any()
    assert changed[10:20].sum() >= 5 and changed[20:30].sum() >= 5 and changed[30:40].all() and changed[40:50].sum() >= 5
    # the deterministic mode reads no counter
    det = _run(batch, d, True, True)
    live = ((moved["terminated"] | moved["truncated"] | case["terminated"] | case["truncated"]) == 0)      # in both states
    np.testing.assert_array_equal(det[0][live], want[True, True][0][live])


# ------------------------------------------------------------------------------------------------- 3. the key
def test_env_offset_above_2_32(batches, cases):
    E, N, offset = 67, 8, (1 << 40) + 12_345
    batch = batches(N, E, env_offset=offset, total_envs=(1 << 41))
    case, want = cases(E, N, offset)
    d = _load(batch, case)
    _assert_equal(_run(batch, d, True, False), want[True, False], "env_offset 2^40 + 12345")
    _, base = cases(E, N)
    assert (want[True, False][0] != base[True, False][0]).mean() > _expected_change(case) / 2    # (not offset 0's stream)


def test_shards_draw_what_the_whole_batch_draws(batches, cases):
    import torch

    E, N, offset, cut = 130, 8, (1 << 32) - 29, 67                                  # global env 2^32 lies inside the first shard
    case = _late(make_sample_case(E, N, seed=99))
    whole = batches(N, E, env_offset=offset, total_envs=offset + E)
    d = _load(whole, case)
    got = _run(whole, d, True, False)
    _assert_equal(got, sample_spec(case["logits_masked"], case["masks"], case["terminated"], case["truncated"],
                                   case["step_count"], case["episode"], env_offset=offset, seed=SEED), "whole batch")
    for lo, hi in ((0, cut), (cut, E)):
        part = {k: (v[lo:hi] if isinstance(v, np.ndarray) else v) for k, v in case.items()}
        shard = batches(N, hi - lo, env_offset=offset + lo, total_envs=offset + E)
        dp = _load(shard, part)
        _assert_equal(_run(shard, dp, True, False), tuple(g[lo:hi] for g in got), f"shard {lo}:{hi}")
    assert torch.cuda.is_available()


def test_the_seed_selects_the_stream(batches, cases):
    E, N = 67, 8
    batch = batches(N, E)
    case, want = cases(E, N)
    d = _load(batch, case)
    first = _run(batch, d, True, False)
    _assert_equal(first, want[True, False], "seed")
    for seed in (SEED ^ 1, SEED ^ (1 << 32), 0):
        batch.set_rng_seed(seed)
        other = _run(batch, d, True, False)
        _assert_equal(other, sample_spec(case["logits_masked"], case["masks"], case["terminated"], case["truncated"],
                                         case["step_count"], case["episode"], seed=seed), f"seed {seed:#x}")
        assert (other[0] != first[0]).mean() > _expected_change(case) / 2
    batch.set_rng_seed(SEED)
    _assert_equal(_run(batch, d, True, False), first, "the same seed again")


# ------------------------------------------------------------------------------------------------- 4. a real loop
C1 = np.array([0.37, -0.21, 0.11, 0.29, -0.13], np.float32)
C2 = np.array([0.19, 0.23, -0.31, 0.07, 0.17], np.float32)
LOOP_E, LOOP_N, LOOP_K = 64, 8, 40


def _logits_np(obs):
    """A fixed function of the rows in single f32 operations (two products and a difference per logit)."""
    return obs[..., 0:5] * C1 - obs[..., 5:10] * C2


@pytest.fixture(scope="module")
def loop_reference():
    """The actor loop on the CPU: the oracle's states, tests/_action_masks.spec_masks, the spec's actions."""
    from _action_masks import spec_masks
    from oracle import oracle

    from collectivecrossing_amd.params import lower_config

    params = lower_config(make_config(LOOP_N, max_steps=12))
    ob = oracle.OracleBatch(params, LOOP_E)
    ob.set_reset_pool(oracle.seeded_placements(params, np.arange(5, 5 + 256, dtype=np.uint64)))
    ob.reset_from_pool()
    obs = ob.observe()
    hist = dict(actions=[], logp=[], masks=[], reset=[])
    for _ in range(LOOP_K):
        masks = spec_masks(oracle, params, ob.x, ob.y, ob.active, ob.terminated, ob.truncated)
        acts, logp, _ = sample_spec(_logits_np(obs), masks, ob.terminated, ob.truncated, ob.step_count, ob.episode, seed=SEED)
        step_obs, _, _, ef = ob.rollout(acts[None], auto_reset=True)
        reset = (ef[0] & 0x04) != 0
        obs = np.where(reset[:, None, None], ob.observe(), step_obs[0])            # reset_obs="next"
        for k, v in (("actions", acts), ("logp", logp), ("masks", masks), ("reset", reset)):
            hist[k].append(v)
    return {k: np.stack(v) for k, v in hist.items()}


def test_actor_loop_eager_and_captured(loop_reference):
    import torch

    from collectivecrossing_amd.batched import BatchedCollectiveCrossing, SampleResult

    ref = loop_reference
    assert ref["reset"].any() and (ref["actions"] == 255).any() and len(np.unique(ref["actions"])) == 6
    E, N, K = LOOP_E, LOOP_N, LOOP_K
    env = BatchedCollectiveCrossing(make_config(N, max_steps=12), E)
    env.make_reset_pool(seed0=5, size=256)
    env.reset_from_pool()
    env.set_rng_seed(SEED)
    start = env.get_state()
    c1, c2 = torch.from_numpy(C1).cuda(), torch.from_numpy(C2).cuda()
    side = torch.cuda.Stream()
    env.use_stream(side)
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        obs = env.observe()
        masks = env.action_masks()
        actions = torch.empty((1, E, N), dtype=torch.uint8, device="cuda")
        logp = torch.empty((E, N), dtype=torch.float32, device="cuda")
        sampled = SampleResult(actions[0], logp, None)
        out = env.alloc_rollout(1)
        hist = {k: torch.empty((K,) + tuple(t.shape), dtype=t.dtype, device="cuda")
                for k, t in (("actions", actions[0]), ("logp", logp), ("masks", masks))}

        def body():
            logits = obs[..., 0:5] * c1 - obs[..., 5:10] * c2
            env.sample_actions(logits, masks, out=sampled)
            env.rollout(actions, auto_reset=True, out=out, masks_out=masks, reset_obs="next")
            obs.copy_(out.obs[0])

        def run(step):
            got = {}
            for s in range(K):
                hist["masks"][s].copy_(masks)                                      # the masks the step samples under
                step()
                hist["actions"][s].copy_(actions[0])
                hist["logp"][s].copy_(logp)
            side.synchronize()
            for k, t in hist.items():
                got[k] = t.cpu().numpy()
            return got

        eager = run(body)
        np.testing.assert_array_equal(eager["masks"], ref["masks"])
        np.testing.assert_array_equal(eager["actions"], ref["actions"], err_msg="the action history")
        np.testing.assert_array_equal(bits32(eager["logp"]), bits32(ref["logp"]))
        live = eager["actions"] != 255
        assert ((eager["masks"][live] >> eager["actions"][live]) & 1).all()        # sampled under the mask of its state
        moves = live & (eager["actions"] < 4)
        assert moves.sum() > 1000 and (eager["masks"][live] != 0x1F).any()
        # the same loop from the same start, captured once and replayed
        env.set_state(**start)
        env.observe(out=obs)
        env.action_masks(out=masks)
        side.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            body()
        side.synchronize()
        replayed = run(graph.replay)
        for k in hist:
            np.testing.assert_array_equal(bits32(replayed[k]), bits32(eager[k]), err_msg=f"graph replay: {k}")
    env.use_stream(None)
    env.close()


# ------------------------------------------------------------------------------------------------- 5. refusals
def test_refusals_leave_the_batch_usable(batches, cases):
    import torch

    from collectivecrossing_amd import SampleResult, _abi

    E, N = 21, 3
    batch = batches(N, E)
    case, want = cases(E, N)
    d = _load(batch, case)
    lg, mk = d["logits_masked"], d["masks"]
    shifted = torch.empty(E * N * 5 + 1, dtype=torch.float32, device="cuda")[1:].view(E, N, 5)
    assert shifted.is_contiguous() and shifted.data_ptr() % 16
    bad = [
        dict(logits=lg.double()), dict(logits=lg.half()), dict(logits=lg.bfloat16()),            # the caller casts
        dict(logits=lg[:, :2].contiguous()), dict(logits=lg[:-1]), dict(logits=lg.reshape(E, N * 5)),
        dict(logits=lg.cpu()), dict(logits=lg.transpose(0, 1).contiguous().transpose(0, 1)),     # not contiguous
        dict(logits=shifted), dict(logits=case["logits"]),
        dict(logits=lg, masks=mk.to(torch.int32)), dict(logits=lg, masks=mk[:-1]), dict(logits=lg, masks=mk.cpu()),
        dict(logits=lg, out=(1, 2, 3)), dict(logits=lg, out=SampleResult(torch.empty((E, N + 1), dtype=torch.uint8, device="cuda"), None, None)),
        dict(logits=lg, out=SampleResult(batch.alloc_sample().actions, torch.empty((E, N), dtype=torch.float64, device="cuda"), None)),
    ]
    for kw in bad:
        with pytest.raises(ValueError):
            batch.sample_actions(**kw)
    # the library's own refusals (the wrapper refuses first, so they are reached through the bindings)
    lib, h = batch._lib, batch._h
    out = batch.alloc_sample(True, True)
    o = [out.actions.data_ptr(), out.logp.data_ptr(), out.entropy.data_ptr()]
    for handle, logits, acts, word in ((None, lg.data_ptr(), o[0], "NULL handle"), (h, None, o[0], "NULL"),
                                       (h, lg.data_ptr(), None, "NULL"), (h, shifted.data_ptr(), o[0], "aligned")):
        assert lib.ccx_sample_actions(handle, logits, mk.data_ptr(), 0, acts, o[1], o[2]) == _abi.EINVAL
        assert word in lib.ccx_last_error().decode()
    _assert_equal(_run(batch, d, True, False), want[True, False], "after the refusals")
