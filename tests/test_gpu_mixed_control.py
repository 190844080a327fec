"""Mixed-control steps on the device (ccx_rollout_mixed: csrc/ccx_step.hip's policy instantiations, and the library's
unfused path for grids without LDS tables).  Every comparison is exact: integers, u32 / u64 bit patterns.

(a) every reference-recorded mixed-control episode (tests/golden/mixed/) through step_mixed and rollout_mixed, GARBAGE in
the scripted slots of the tensor; (b) fused == the composition policy_actions -> torch.where -> step on a second handle,
over agent counts x batch sizes x masks x policies x epsilon x move order x outputs x auto-reset; (c) mask "all" ==
rollout_policy; (d) the unfused path; (e) graph capture, no allocation; (f) the documented errors; (g) input checking."""

import numpy as np
import pytest
from _fixtures import assert_step_matches, config_from_dict
from _mixed import MIXED_NPZ, MixedGolden

from collectivecrossing_amd import _abi

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ccx():
    import torch

    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    from collectivecrossing_amd.batched import BatchedCollectiveCrossing

    return BatchedCollectiveCrossing


def _np(t):
    return None if t is None else t.cpu().numpy()


def _bits(t):
    import torch
    return t.view(torch.int64 if t.dtype is torch.float64 else torch.int32)


# ------------------------------------------------------------------------------------------- (a) the reference
def _assert_rollout_matches(g, res, actions_out, state, label):
    K = res.agent_flags.shape[0]
    np.testing.assert_array_equal(_np(actions_out), g["actions"][:K], err_msg=f"actions_out {label}")
    for s in range(K):
        last = s == K - 1
        st = state if last else {k: g[k][s] for k in ("x", "y", "active", "terminated", "truncated", "step_count")}
        assert_step_matches(g, s, _np(res.obs[s]), _np(res.reward[s]), _np(res.agent_flags[s]), _np(res.env_flags[s]), st,
                            label=label)


@pytest.mark.parametrize("name", MIXED_NPZ)
def test_step_mixed_replays_the_reference(ccx, name):
    import torch
    g = MixedGolden(name)
    tensor = torch.from_numpy(g.tensor()).cuda()
    env = ccx(g.config, g.E)
    assert env.step_shape()["ok"] == (0 if g.params.width == 100 else 1)
    env.set_state(**g.init_state())
    ao = torch.empty((g.E, g.N), dtype=torch.uint8, device="cuda")
    for s in range(g.K):
        # (the recorded dict order; an episode recorded in slot order also runs without an order array every other step)
        order = None if (g.identity_order() and s % 2) else g["order"][s]
        r = env.step_mixed(tensor[s], g.mask, g.policy, order=order, actions_out=ao)
        np.testing.assert_array_equal(_np(ao), g["actions"][s], err_msg=f"{name} step {s}: actions_out")
        assert_step_matches(g, s, _np(r.obs), _np(r.reward), _np(r.agent_flags), _np(r.env_flags), env.get_state())
    env.close()


@pytest.mark.parametrize("name", MIXED_NPZ)
@pytest.mark.parametrize("cut", [0, 16])
def test_rollout_mixed_replays_the_reference(ccx, name, cut):
    """One call for the whole episode (the library cuts it into launches of 16), and the caller cutting at 16."""
    import torch
    g = MixedGolden(name)
    tensor = torch.from_numpy(g.tensor()).cuda()
    order = torch.from_numpy(g["order"]).cuda()
    env = ccx(g.config, g.E)
    env.set_state(**g.init_state())
    ao = torch.full((g.K, g.E, g.N), 77, dtype=torch.uint8, device="cuda")
    res = env.alloc_rollout(g.K)
    if cut == 0:
        env.rollout_mixed(tensor, g.mask, g.policy, order=order, out=res, actions_out=ao)
    else:
        from collectivecrossing_amd.batched import RolloutResult
        for k0 in range(0, g.K, cut):
            k1 = min(g.K, k0 + cut)
            part = RolloutResult(res.obs[k0:k1], res.reward[k0:k1], res.agent_flags[k0:k1], res.env_flags[k0:k1])
            if part.obs.data_ptr() % 16:          # (an odd E x N: this slice of the rows is not 16-byte aligned)
                part = None
            got = env.rollout_mixed(tensor[k0:k1], g.mask, g.policy, order=order[k0:k1], out=part, actions_out=ao[k0:k1])
            if part is None:
                for f in ("obs", "reward", "agent_flags", "env_flags"):
                    getattr(res, f)[k0:k1] = getattr(got, f)
    _assert_rollout_matches(g, res, ao, env.get_state(), f"cut={cut}")
    env.close()


# ------------------------------------------------------------------------------------------- (b) fused == composition
def _matrix_cfg(N, max_steps=20):
    short = dict(truncated_config=dict(truncated_function="max_steps", max_steps=max_steps))
    c1 = dict(width=12, height=8, division_y=4, tram_door_left=5, tram_door_right=7, tram_length=9,
              exiting_destination_area_y=0, boarding_destination_area_y=8, **short)
    if N <= 8:
        nb = {1: 1, 3: 2, 5: 3, 8: 5}[N]
        return config_from_dict(dict(c1, num_boarding_agents=nb, num_exiting_agents=N - nb))
    if N == 32:
        return config_from_dict(dict(width=20, height=12, division_y=6, tram_door_left=6, tram_door_right=10, tram_length=16,
                                     num_boarding_agents=16, num_exiting_agents=16, exiting_destination_area_y=0,
                                     boarding_destination_area_y=12,
                                     reward_config=dict(reward_function="simple_distance", distance_penalty_factor=0.1), **short))
    nb = N // 2
    return config_from_dict(dict(width=32, height=16, division_y=8, tram_door_left=10, tram_door_right=16, tram_length=26,
                                 num_boarding_agents=nb, num_exiting_agents=N - nb, exiting_destination_area_y=0,
                                 boarding_destination_area_y=16,
                                 terminated_config=dict(terminated_function="all_at_destination" if N == 64 else
                                                        "individual_at_destination"), _relaxed=N > 50, **short))


def _masks(cfg, N):
    from collectivecrossing_amd.batched import scripted_slot_mask
    return [("none", 0), ("all", scripted_slot_mask(cfg, "all")), ("exiting", scripted_slot_mask(cfg, "exiting")),
            ("boarding", scripted_slot_mask(cfg, "boarding")), ("single", 1 << (N // 2)),
            ("alternating", sum(1 << a for a in range(0, N, 2)))]


STEPS = 32
OUTPUTS = [(True, False), (False, True), (True, True), (False, False)]       # (want_obs, want_compact)
CHUNKS = [(1,), (1, 4, 16), (16, 3), (2, 1)]                                 # launch lengths of the mixed-control side


def _rotation(ei, mi):
    """(policy, epsilon, move order, auto-reset, outputs, launch lengths) of batch size number ei and mask number mi.  The
    strides are chosen so that the 24 runs hold every pair of values of any two axes (batch size and mask included):
    test_the_rotation_covers_every_pair checks that on the CPU side of this file."""
    return (("greedy", "waiting")[(mi + ei // 2) % 2], (0.0, 0.3)[(mi // 2 + ei) % 2], bool((mi // 3 + ei) % 2),
            (mi + ei) % 3 != 0, OUTPUTS[(mi + 3 * ei) % 4], CHUNKS[(mi + ei + 3 * (mi // 2)) % 4])


def test_the_rotation_covers_every_pair():
    import itertools
    rows = [(ei, mi, *_rotation(ei, mi)) for ei in range(4) for mi in range(6)]
    for a, b in itertools.combinations(range(8), 2):
        va, vb = {r[a] for r in rows}, {r[b] for r in rows}
        assert len({(r[a], r[b]) for r in rows}) == len(va) * len(vb), (a, b)
    assert [len({r[k] for r in rows}) for k in range(8)] == [4, 6, 2, 2, 2, 2, 4, 4]


def _run_pair(ccx, cfg, E, N, mask, policy, eps, with_order, auto_reset, want_obs, want_compact, chunks, seen, tag):
    """Handle A: the parent's way, step by step.  Handle B: the mixed-control call, in launches of `chunks` steps."""
    import torch
    gen = torch.Generator(device="cpu").manual_seed(E * 1000 + N * 7 + mask % 997)
    acts = torch.randint(0, 6, (STEPS, E, N), dtype=torch.uint8, generator=gen)
    acts[acts == 5] = 255
    acts = acts.cuda()
    orders = torch.argsort(torch.rand((STEPS, E, N), generator=gen), dim=-1).to(torch.uint8).cuda() if with_order else None
    sel = torch.tensor([(mask >> a) & 1 for a in range(N)], dtype=torch.bool, device="cuda")
    A, B = ccx(cfg, E), ccx(cfg, E)
    for h in (A, B):
        h.make_reset_pool(11, 64)
        h.reset_from_pool()
        h.set_rng_seed(77)
        h.set_policy_epsilon(eps)
    ao = torch.full((STEPS, E, N), 99, dtype=torch.uint8, device="cuda")
    s = 0
    ci = 0
    while s < STEPS:
        K = min(chunks[ci % len(chunks)], STEPS - s)
        ci += 1
        if E * N % 2 and want_obs and s % 2:
            K = 1                                    # (an odd E x N: a multi-step launch's rows must start 16-byte aligned)
        o = None if orders is None else orders[s:s + K]
        if K == 1 and not auto_reset:
            rb = B.step_mixed(acts[s], mask, policy, order=None if o is None else o[0], want_obs=want_obs,
                              want_compact=want_compact, actions_out=ao[s])
            outs_b = [(rb.obs, rb.reward, rb.agent_flags, rb.env_flags, rb.obs_compact)]
        else:
            rb = B.rollout_mixed(acts[s:s + K], mask, policy, order=o, auto_reset=auto_reset, actions_out=ao[s:s + K],
                                 want_obs=want_obs, want_compact=want_compact)
            outs_b = [(None if rb.obs is None else rb.obs[k], rb.reward[k], rb.agent_flags[k], rb.env_flags[k],
                       None if rb.obs_compact is None else rb.obs_compact[k]) for k in range(K)]
        for k in range(K):
            pa = A.policy_actions(policy)
            merged = torch.where(sel, pa, acts[s + k])
            if eps > 0 and mask:                     # (did a draw really change a scripted action?  host-side setting only)
                A.set_policy_epsilon(0.0)
                seen["explored"] |= bool((A.policy_actions(policy) != pa)[:, sel].any())
                A.set_policy_epsilon(eps)
            ok = None if orders is None else orders[s + k]
            if auto_reset:
                ra = A.rollout(merged[None], order=None if ok is None else ok[None], auto_reset=True, want_obs=want_obs,
                               want_compact=want_compact)
                out_a = (None if ra.obs is None else ra.obs[0], ra.reward[0], ra.agent_flags[0], ra.env_flags[0],
                         None if ra.obs_compact is None else ra.obs_compact[0])
            else:
                ra = A.step(merged, ok, want_obs=want_obs, want_compact=want_compact)
                out_a = (ra.obs, ra.reward, ra.agent_flags, ra.env_flags, ra.obs_compact)
            where = f"{tag} step {s + k}"
            assert torch.equal(ao[s + k], merged), f"actions_out {where}"
            for name, x, y in zip(("obs", "reward", "agent_flags", "env_flags", "obs_compact"), out_a, outs_b[k]):
                assert (x is None) == (y is None), f"{name} {where}"
                if x is not None:
                    assert torch.equal(_bits(x) if x.dtype.is_floating_point else x,
                                       _bits(y) if y.dtype.is_floating_point else y), f"{name} {where}"
            af, ef = out_a[2], out_a[3]
            seen["reset"] |= bool((ef & _abi.EF_RESET).any())
            seen["truncated"] |= bool((af & _abi.AF_TRUNCATED).any())
            seen["terminated"] |= bool((af & _abi.AF_TERMINATED).any())
            seen["arrived"] |= bool((af & _abi.AF_AT_DEST).any())
            seen["absent_scripted"] |= bool((merged[:, sel] == 255).any()) if mask else False
        s += K
    sa, sb = A.get_state(), B.get_state()
    for k in sa:
        np.testing.assert_array_equal(sa[k], sb[k], err_msg=f"state {k} {tag}")
    assert A.counters() == B.counters(), tag
    A.close()
    B.close()


@pytest.mark.parametrize("N", [1, 3, 5, 8, 32, 50, 64])
def test_fused_equals_the_composition(ccx, N):
    """policy_actions -> torch.where -> step on one handle, step_mixed / rollout_mixed on a second from the same state,
    32 consecutive steps (max_steps = 20: arrivals, done agents, truncation and -- with auto-reset -- restarts are crossed).
    Batch sizes 1, 3, 4096, 4099 x six masks; policy, epsilon, move order, outputs, auto-reset and the launch lengths
    rotate (_rotation) so that every pair of values of any two of these eight axes meets somewhere in the matrix."""
    import torch
    cfg = _matrix_cfg(N)
    seen = dict(reset=False, truncated=False, terminated=False, arrived=False, absent_scripted=False, explored=False)
    run = 0
    for ei, E in enumerate((1, 3, 4096, 4099)):
        for mi, (mname, mask) in enumerate(_masks(cfg, N)):
            policy, eps, with_order, auto_reset, outs, chunks = _rotation(ei, mi)
            want_obs, want_compact = outs
            tag = f"N={N} E={E} mask={mname} {policy} eps={eps} order={with_order} reset={auto_reset} chunks={chunks}"
            _run_pair(ccx, cfg, E, N, mask, policy, eps, with_order, auto_reset, want_obs, want_compact, chunks, seen, tag)
            run += 1
        torch.cuda.empty_cache()
    assert run == 24
    # (N = 64 runs all_at_destination: 64 agents do not all arrive within 20 steps, so its terminated flag stays down)
    assert all(v for k, v in seen.items() if k != "terminated") and (seen["terminated"] or N == 64), seen


# ------------------------------------------------------------------------------------------- (c) mask "all" == rollout_policy
@pytest.mark.parametrize("eps", [0.0, 0.3])
@pytest.mark.parametrize("policy", ["greedy", "waiting"])
def test_everything_scripted_equals_rollout_policy(ccx, policy, eps):
    import torch
    cfg = _matrix_cfg(8)
    E, K = 1000, 40
    A, B = ccx(cfg, E), ccx(cfg, E)
    for h in (A, B):
        h.make_reset_pool(5, 64)
        h.reset_from_pool()
        h.set_rng_seed(1234)
        h.set_policy_epsilon(eps)
    ra, acts_a = A.rollout_policy(K, policy, auto_reset=True)
    acts_b = torch.empty_like(acts_a)
    rb = B.rollout_mixed(None, "all", policy, auto_reset=True, actions_out=acts_b, num_steps=K)
    assert torch.equal(acts_a, acts_b)
    assert torch.equal(_bits(ra.obs), _bits(rb.obs)) and torch.equal(_bits(ra.reward), _bits(rb.reward))
    assert torch.equal(ra.agent_flags, rb.agent_flags) and torch.equal(ra.env_flags, rb.env_flags)
    assert bool((ra.env_flags & _abi.EF_RESET).any())
    sa, sb = A.get_state(), B.get_state()
    for k in sa:
        np.testing.assert_array_equal(sa[k], sb[k], err_msg=k)
    A.close()
    B.close()


def test_no_slot_scripted_equals_plain_step(ccx):
    import torch
    cfg = _matrix_cfg(8)
    E = 500
    A, B = ccx(cfg, E), ccx(cfg, E)
    for h in (A, B):
        h.make_reset_pool(5, 64)
        h.reset_from_pool()
    acts = torch.randint(0, 5, (25, E, 8), dtype=torch.uint8, device="cuda")
    for s in range(25):
        ra, rb = A.step(acts[s]), B.step_mixed(acts[s], 0)
        assert torch.equal(_bits(ra.obs), _bits(rb.obs)) and torch.equal(_bits(ra.reward), _bits(rb.reward))
        assert torch.equal(ra.agent_flags, rb.agent_flags) and torch.equal(ra.env_flags, rb.env_flags)
    A.close()
    B.close()


# ------------------------------------------------------------------------------------------- (d) the unfused path
def _big_cfg(max_steps=15):
    return config_from_dict(dict(width=100, height=100, division_y=50, tram_door_left=25, tram_door_right=35, tram_length=60,
                                 num_boarding_agents=6, num_exiting_agents=6, exiting_destination_area_y=0,
                                 boarding_destination_area_y=100,
                                 truncated_config=dict(truncated_function="max_steps", max_steps=max_steps)))


@pytest.mark.parametrize("which", ["100x100", "tunable"])
def test_the_unfused_path_gives_the_same_results(ccx, which):
    """A handle whose short launches cannot use the step kernel runs the composition inside the library: equal to the
    composition done by the caller (100 x 100), and -- forced by the tunable on a small grid -- to the fused kernel."""
    import torch
    cfg = _big_cfg() if which == "100x100" else _matrix_cfg(8)
    N = 12 if which == "100x100" else 8
    E = 37
    seen = dict(reset=False, truncated=False, terminated=False, arrived=False, absent_scripted=False, explored=False)
    if which == "100x100":
        probe = ccx(cfg, E)
        assert probe.step_shape()["ok"] == 0
        probe.close()
        for mi, (mname, mask) in enumerate(_masks(cfg, N)):
            _run_pair(ccx, cfg, E, N, mask, ("greedy", "waiting")[mi % 2], (0.0, 0.3)[(mi // 2) % 2], bool(mi % 2), bool(mi % 3),
                      mi % 2 == 0, mi % 3 == 0, [(1,), (5, 1)][mi % 2], seen, f"100x100 mask={mname}")
        assert seen["truncated"] and seen["reset"]
        return
    from collectivecrossing_amd.batched import scripted_slot_mask
    mask = scripted_slot_mask(cfg, "exiting")
    A, B = ccx(cfg, E), ccx(cfg, E)
    B.set_tunable("step_kernel", 0)
    assert A.step_shape()["ok"] == 1 and B.step_shape()["ok"] == 0
    for h in (A, B):
        h.make_reset_pool(2, 32)
        h.reset_from_pool()
        h.set_rng_seed(5)
        h.set_policy_epsilon(0.3)
    acts = torch.randint(0, 5, (24, E, N), dtype=torch.uint8, device="cuda")
    oa, ob = torch.empty_like(acts), torch.empty_like(acts)
    ra = A.rollout_mixed(acts, mask, "waiting", auto_reset=True, actions_out=oa)
    rb = B.rollout_mixed(acts, mask, "waiting", auto_reset=True, actions_out=ob)
    assert torch.equal(oa, ob)
    assert torch.equal(_bits(ra.obs), _bits(rb.obs)) and torch.equal(_bits(ra.reward), _bits(rb.reward))
    assert torch.equal(ra.agent_flags, rb.agent_flags) and torch.equal(ra.env_flags, rb.env_flags)
    A.close()
    B.close()


# ------------------------------------------------------------------------------------------- (e) graphs, allocation
def test_a_graph_of_mixed_steps_replays_bit_exactly_and_allocates_nothing(ccx):
    import torch
    cfg = _matrix_cfg(8, max_steps=1000)
    E, N = 512, 8
    A, B = ccx(cfg, E), ccx(cfg, E)
    seeds = np.arange(E, dtype=np.uint64)
    acts = torch.randint(0, 5, (E, N), dtype=torch.uint8, device="cuda")
    side = torch.cuda.Stream()
    B.use_stream(side)
    A.reset(seeds)
    B.reset(seeds)
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        ao = torch.empty((E, N), dtype=torch.uint8, device="cuda")
        B.step_mixed(acts, "exiting", "greedy", actions_out=ao)            # first call: the output buffers
        side.synchronize()
        before = torch.cuda.memory_allocated()
        B.step_mixed(acts, "exiting", "greedy", actions_out=ao)
        side.synchronize()
        assert torch.cuda.memory_allocated() == before        # (the fused path owns no buffer at all)
        B.reset(seeds)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            rb = B.step_mixed(acts, "exiting", "greedy", actions_out=ao)
        B.reset(seeds)                                                     # (the capture ran nothing)
        side.synchronize()
        for _ in range(50):
            graph.replay()
        side.synchronize()
    sel = torch.tensor([a >= 5 for a in range(N)], device="cuda")
    for _ in range(50):
        merged = torch.where(sel, A.policy_actions("greedy"), acts)
        ra = A.step(merged)
    torch.cuda.synchronize()
    assert torch.equal(ao, merged)
    assert torch.equal(_bits(ra.obs), _bits(rb.obs)) and torch.equal(_bits(ra.reward), _bits(rb.reward))
    assert torch.equal(ra.agent_flags, rb.agent_flags)
    sa, sb = A.get_state(), B.get_state()
    for k in sa:
        np.testing.assert_array_equal(sa[k], sb[k], err_msg=k)
    assert int(sa["step_count"][0]) == 50
    A.close()
    B.close()


@pytest.mark.parametrize("which", ["100x100", "tunable"])
def test_a_graph_of_unfused_mixed_steps_replays_bit_exactly(ccx, which):
    """The unfused path keeps the merged actions in a scratch buffer of the handle (no actions_out here, so it is really
    used).  It is allocated by the first eager call; a capture refuses to allocate and a replay runs with the pointers
    baked in at capture time, so 50 replays equal to 50 eager steps of the composition on a second handle show that the
    buffer neither moves nor is allocated again.  torch's own allocator sees no new memory either."""
    import torch
    cfg = _big_cfg(max_steps=1000) if which == "100x100" else _matrix_cfg(8, max_steps=1000)
    E, N = 96, (12 if which == "100x100" else 8)
    A, B = ccx(cfg, E), ccx(cfg, E)
    if which == "tunable":
        B.set_tunable("step_kernel", 0)
    assert B.step_shape()["ok"] == 0
    seeds = np.arange(E, dtype=np.uint64) + 9
    acts = torch.randint(0, 5, (E, N), dtype=torch.uint8, device="cuda")
    side = torch.cuda.Stream()
    B.use_stream(side)
    A.reset(seeds)
    B.reset(seeds)
    for h in (A, B):
        h.set_rng_seed(31)
        h.set_policy_epsilon(0.3)
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        B.step_mixed(acts, "boarding", "waiting")                          # first call: output buffers, the scratch buffer
        side.synchronize()
        before = torch.cuda.memory_allocated()
        B.step_mixed(acts, "boarding", "waiting")
        side.synchronize()
        assert torch.cuda.memory_allocated() == before
        B.reset(seeds)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            rb = B.step_mixed(acts, "boarding", "waiting")
        B.reset(seeds)                                                     # (the capture ran nothing)
        side.synchronize()
        for _ in range(50):
            graph.replay()
        side.synchronize()
    sel = torch.tensor([a < cfg.num_boarding_agents for a in range(N)], device="cuda")
    for _ in range(50):
        ra = A.step(torch.where(sel, A.policy_actions("waiting"), acts))
    torch.cuda.synchronize()
    assert torch.equal(_bits(ra.obs), _bits(rb.obs)) and torch.equal(_bits(ra.reward), _bits(rb.reward))
    assert torch.equal(ra.agent_flags, rb.agent_flags) and torch.equal(ra.env_flags, rb.env_flags)
    sa, sb = A.get_state(), B.get_state()
    for k in sa:
        np.testing.assert_array_equal(sa[k], sb[k], err_msg=k)
    assert int(sa["step_count"][0]) == 50
    A.close()
    B.close()


def test_an_unfused_mixed_step_refuses_to_allocate_inside_a_capture(ccx):
    """The first unfused call allocates the scratch buffer, so it cannot be the captured one: the documented error, and the
    state untouched."""
    import torch

    from collectivecrossing_amd._lib import CcxError
    E = 8
    env = ccx(_matrix_cfg(8), E)
    env.set_tunable("step_kernel", 0)
    side = torch.cuda.Stream()
    env.use_stream(side)
    env.reset(np.arange(E, dtype=np.uint64))
    before = env.get_state()
    acts = torch.zeros((E, 8), dtype=torch.uint8, device="cuda")
    with torch.cuda.stream(side):
        env.step(acts)                                                     # (the output buffers exist; the scratch does not)
        env.set_state(**{k: before[k] for k in ("x", "y", "active", "terminated", "truncated", "step_count")})
        side.synchronize()
        graph = torch.cuda.CUDAGraph()
        with pytest.raises(CcxError, match="allocates scratch buffers on first use"):
            with torch.cuda.graph(graph, stream=side):
                env.step_mixed(acts, "exiting", "greedy")
        side.synchronize()
    after = env.get_state()
    for k in before:
        np.testing.assert_array_equal(before[k], after[k], err_msg=k)
    env.close()


# ------------------------------------------------------------------------------------------- (f) errors
def test_documented_errors_leave_the_state_untouched(ccx):
    import ctypes as C

    import torch

    from collectivecrossing_amd._lib import CcxError
    cfg = _matrix_cfg(8)
    E, N = 16, 8
    env = ccx(cfg, E)
    env.reset(np.arange(E, dtype=np.uint64))
    before = env.get_state()
    acts = torch.zeros((E, N), dtype=torch.uint8, device="cuda")
    ro = _abi.CcxRolloutOut()

    def raw(mask, a, policy=_abi.POLICY_GREEDY):
        return env._lib.ccx_rollout_mixed(env._h, 1, policy, mask, None if a is None else a.data_ptr(), None, 0, C.byref(ro), None)

    assert raw(1 << N, acts) == _abi.EINVAL and b"at or above N" in env._lib.ccx_last_error()
    assert raw(0b1, None) == _abi.EINVAL and b"NULL only when" in env._lib.ccx_last_error()
    assert raw(0b1, acts, _abi.POLICY_RANDOM) == _abi.EINVAL
    with pytest.raises(ValueError):
        env.step_mixed(acts, [N], "greedy")
    with pytest.raises(ValueError):
        env.step_mixed(None, "exiting", "greedy")
    with pytest.raises(ValueError):
        env.step_mixed(acts, "exiting", "random")
    env.set_policy_stream("mt19937", 42)
    env.set_policy_epsilon(0.3)
    with pytest.raises(CcxError, match="MT19937.*sequential per env"):
        env.step_mixed(acts, "exiting", "greedy")
    after = env.get_state()
    for k in before:
        np.testing.assert_array_equal(before[k], after[k], err_msg=k)
    env.set_policy_epsilon(0.0)
    env.step_mixed(acts, "exiting", "greedy")                  # epsilon = 0: the stream kind does not matter
    assert int(env.get_state()["step_count"][0]) == int(before["step_count"][0]) + 1
    env.close()


def test_array_strategy_batches_refuse_mixed_control(ccx):
    import torch

    from collectivecrossing_amd import strategies as S

    class _ArrayReward(S.RewardFunction):
        def calculate_reward(self, agent_id, env):
            return 0.0

        def calculate_rewards_batch(self, view):
            return torch.zeros((view.num_envs, view.num_agents), dtype=torch.float64, device=view.device)

    S.REWARD_FUNCTIONS["mixed_control_array_reward"] = _ArrayReward
    cfg = config_from_dict(dict(width=12, height=8, division_y=4, tram_door_left=5, tram_door_right=7, tram_length=9,
                                num_boarding_agents=5, num_exiting_agents=3, exiting_destination_area_y=0,
                                boarding_destination_area_y=8, reward_config=dict(reward_function="mixed_control_array_reward")))
    env = ccx(cfg, 4)
    assert env.has_array_strategies
    env.reset(np.arange(4, dtype=np.uint64))
    before = env.get_state()
    acts = torch.zeros((4, 8), dtype=torch.uint8, device="cuda")
    with pytest.raises(NotImplementedError, match="array-form"):
        env.step_mixed(acts, "exiting")
    with pytest.raises(NotImplementedError, match="array-form"):
        env.rollout_mixed(acts[None], "exiting")
    after = env.get_state()
    for k in before:
        np.testing.assert_array_equal(before[k], after[k], err_msg=k)
    env.close()


# ------------------------------------------------------------------------------------------- (g) input checking
@pytest.mark.parametrize("unfused", [False, True])
def test_check_inputs_ignores_the_scripted_slots(ccx, unfused):
    import torch

    from collectivecrossing_amd._lib import CcxInputError
    cfg = _matrix_cfg(8)
    E, N = 32, 8
    env = ccx(cfg, E)
    if unfused:
        env.set_tunable("step_kernel", 0)
    env.set_check_inputs(True)
    env.reset(np.arange(E, dtype=np.uint64))
    acts = torch.zeros((E, N), dtype=torch.uint8, device="cuda")
    acts[3, 6] = 9                                   # an exiting slot: scripted below, so never looked at
    env.step_mixed(acts, "exiting", "greedy")
    env.check_inputs()
    env.step_mixed(acts, "boarding", "greedy")       # the same byte in a tensor-driven slot
    with pytest.raises(CcxInputError, match="1 action byte"):
        env.check_inputs()
    env.close()
