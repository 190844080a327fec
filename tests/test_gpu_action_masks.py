"""Legal-action masks on the device (include/ccx.h: CCX_ACTION_MASKS): the stand-alone kernel against the
reference-recorded fixtures and the NumPy spec, the masks a step's own launch writes against the stand-alone kernel run
behind the same launch, and that asking for masks changes nothing else."""

import numpy as np
import pytest
from _action_masks import MASK_NPZ, WAIT_ONLY, MaskFixture, random_states, spec_masks
from _fixtures import config_from_dict

from collectivecrossing_amd import _abi

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ccx():
    import torch

    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    from collectivecrossing_amd.batched import BatchedCollectiveCrossing

    return BatchedCollectiveCrossing


def _bits(t):
    import torch
    return t.view(torch.int64 if t.dtype is torch.float64 else torch.int32)


def _cfg(N, max_steps=20, big=False):
    short = dict(truncated_config=dict(truncated_function="max_steps", max_steps=max_steps))
    nb = {1: 1, 3: 2, 5: 3, 8: 5}.get(N, N // 2)
    if big:        # 100 x 100: the occupancy tables exceed the LDS, short launches take the rollout kernel
        geo = dict(width=100, height=100, division_y=50, tram_door_left=25, tram_door_right=35, tram_length=60,
                   boarding_destination_area_y=100)
    elif N <= 8:
        geo = dict(width=12, height=8, division_y=4, tram_door_left=5, tram_door_right=7, tram_length=9,
                   boarding_destination_area_y=8)
    elif N == 32:
        geo = dict(width=20, height=12, division_y=6, tram_door_left=6, tram_door_right=10, tram_length=16,
                   boarding_destination_area_y=12)
    else:
        geo = dict(width=32, height=16, division_y=8, tram_door_left=10, tram_door_right=16, tram_length=26,
                   boarding_destination_area_y=16,
                   terminated_config=dict(terminated_function="all_at_destination" if N == 64 else "individual_at_destination"))
        if N > 50:
            geo["_relaxed"] = True
    return config_from_dict(dict(geo, num_boarding_agents=nb, num_exiting_agents=N - nb, exiting_destination_area_y=0, **short))


def _tiled_states(oracle, params, E, seed):
    """E states: 192 random ones, repeated with a shift so that neighbouring envs of a wave differ."""
    base = random_states(oracle, params, min(E, 192), seed)
    idx = (np.arange(E) * 7) % min(E, 192)
    return {k: np.ascontiguousarray(v[idx]) for k, v in base.items()}


# ------------------------------------------------------------------------------------------- the stand-alone kernel
@pytest.mark.parametrize("name", MASK_NPZ)
def test_kernel_equals_the_reference_fixtures(ccx, name):
    f = MaskFixture(name)
    env = ccx(f.config, f.S)
    env.set_state(**f.state())
    got = env.action_masks().cpu().numpy()
    np.testing.assert_array_equal(got, f["masks"], err_msg=name)
    env.close()


@pytest.mark.parametrize("N,big", [(1, False), (3, False), (8, False), (32, False), (50, False), (64, False), (8, True), (50, True)])
def test_kernel_equals_the_spec_on_random_states(ccx, oracle, N, big):
    import torch
    cfg = _cfg(N, big=big)
    for E in (1, 3, 4096, 4099):
        env = ccx(cfg, E)
        st = _tiled_states(oracle, env.params, E, 100 * N + E)
        env.set_state(**st)
        out = torch.full((E, N), 0xAB, dtype=torch.uint8, device="cuda")
        assert env.action_masks(out=out) is out
        exp = spec_masks(oracle, env.params, **st)
        np.testing.assert_array_equal(out.cpu().numpy(), exp, err_msg=f"N={N} E={E} big={big}")
        if E >= 4096 and N > 1:
            live = (st["terminated"] == 0) & (st["truncated"] == 0)
            assert (exp[live] != 0x1F).any() and (exp[live] != WAIT_ONLY).any()
        env.close()
    torch.cuda.empty_cache()


# ------------------------------------------------------------------------------------------- fused == stand-alone
def test_which_launches_write_their_own_masks(ccx):
    env = ccx(_cfg(8), 64)
    assert env.step_shape()["ok"] == 1
    # the minimum set: one step without a move order, plain and mixed
    assert env.masks_fused(1) and env.masks_fused(1, mixed=True)
    # composed with the stand-alone kernel: a move order, more than one step
    assert not env.masks_fused(1, order=True) and not env.masks_fused(4) and not env.masks_fused(16)
    assert not env.masks_fused(16, mixed=True)
    env.set_tunable("step_kernel", 0)
    assert not env.masks_fused(1)
    env.close()
    big = ccx(_cfg(8, big=True), 5)
    assert big.step_shape()["ok"] == 0 and not big.masks_fused(1) and not big.masks_fused(1, mixed=True)
    big.close()


LAUNCHES = ("step", "step_order", "step_mixed", "rollout4_reset", "rollout16", "rollout_mixed3", "rollout_policy5", "rollout40")


@pytest.mark.parametrize("N,E", [(1, 3), (3, 4099), (5, 37), (8, 4096), (8, 3), (32, 4099), (50, 1), (64, 1027)])
def test_masks_of_a_launch_equal_the_kernel_run_behind_it(ccx, N, E):
    """Every kind of launch, 12 rounds each from a running state (max_steps = 20 and a reset pool: arrivals, done agents,
    truncation and restarts are crossed): the masks the launch left == ``action_masks()`` called right behind it."""
    import torch
    cfg = _cfg(N)
    env = ccx(cfg, E)
    env.make_reset_pool(11, 64)
    env.reset_from_pool()
    env.set_rng_seed(99)
    gen = torch.Generator(device="cpu").manual_seed(N * 1000 + E)
    seen = dict(reset=False, done=False, blocked=False, fused=False, composed=False)
    for kind in LAUNCHES:
        # every kind starts 14 steps into fresh episodes: truncation (max_steps = 20) falls into its 12 rounds, and -- a
        # finished env that is not restarted stays finished -- no kind inherits a dead batch from the one before
        env.reset_from_pool()
        env.rollout(torch.randint(0, 5, (14, E, N), dtype=torch.uint8, generator=gen), auto_reset=True, want_obs=False)
        for r in range(12):
            K = {"rollout4_reset": 4, "rollout16": 16, "rollout_mixed3": 3, "rollout_policy5": 5, "rollout40": 40}.get(kind, 1)
            acts = torch.randint(0, 6, (K, E, N), dtype=torch.uint8, generator=gen)
            acts[acts == 5] = 255
            acts = acts.cuda()
            order = torch.argsort(torch.rand((K, E, N), generator=gen), dim=-1).to(torch.uint8).cuda()
            mo = torch.full((E, N), 0xAB, dtype=torch.uint8, device="cuda")
            if kind == "step":
                got, fused = env.step(acts[0], want_masks=True).action_masks, env.masks_fused(1)
            elif kind == "step_order":
                got, fused = env.step(acts[0], order=order[0], want_masks=True).action_masks, env.masks_fused(1, order=True)
            elif kind == "step_mixed":
                got = env.step_mixed(acts[0], "exiting" if N > 1 else 0, "greedy", want_masks=True).action_masks
                fused = env.masks_fused(1, mixed=True)
            elif kind == "rollout_mixed3":
                res = env.rollout_mixed(acts, "boarding", "waiting", auto_reset=True, masks_out=mo, want_obs=False)
                got, fused = mo, env.masks_fused(K, mixed=True)
                seen["reset"] |= bool((res.env_flags & _abi.EF_RESET).any())
            elif kind == "rollout_policy5":
                res, _ = env.rollout_policy(K, "greedy", auto_reset=True, masks_out=mo, want_obs=False)
                got, fused = mo, False
                seen["reset"] |= bool((res.env_flags & _abi.EF_RESET).any())
            else:
                res = env.rollout(acts, order=order if r % 2 else None, auto_reset=True, masks_out=mo, want_obs=False)
                got, fused = mo, env.masks_fused(K, order=bool(r % 2))
                seen["reset"] |= bool((res.env_flags & _abi.EF_RESET).any())
            ref = env.action_masks()
            assert torch.equal(got, ref), f"N={N} E={E} {kind} round {r}"
            st = env.get_state()
            done = (st["terminated"] != 0) | (st["truncated"] != 0)
            g = got.cpu().numpy()
            assert (g[done] == WAIT_ONLY).all() and ((g & 0xF0) == 0x10).all()
            seen["done"] |= bool(done.any())
            seen["blocked"] |= bool((g[~done] != 0x1F).any())
            seen["fused" if fused else "composed"] = True
    # (a restart inside the FUSED single step needs auto_reset on a one-step rollout: its own round below)
    env.reset_from_pool()
    for r in range(25):
        acts = torch.randint(0, 5, (1, E, N), dtype=torch.uint8, generator=gen).cuda()
        mo = torch.full((E, N), 0xAB, dtype=torch.uint8, device="cuda")
        res = env.rollout(acts, auto_reset=True, masks_out=mo, want_obs=r % 2 == 0 and (E * N) % 2 == 0)
        assert env.masks_fused(1)
        assert torch.equal(mo, env.action_masks()), f"N={N} E={E} one-step rollout with auto-reset, round {r}"
        if bool((res.env_flags & _abi.EF_RESET).any()):
            seen["reset_fused"] = True
    assert all(seen.values()) and seen.get("reset_fused"), seen
    env.close()


def test_composed_paths_100x100_tunable_and_step_finish(ccx):
    import torch
    for which in ("100x100", "tunable"):
        env = ccx(_cfg(8, big=which == "100x100"), 37)
        if which == "tunable":
            env.set_tunable("step_kernel", 0)
        env.make_reset_pool(3, 16)
        env.reset_from_pool()
        assert not env.masks_fused(1)
        for r in range(24):
            acts = torch.randint(0, 5, (37, 8), dtype=torch.uint8, device="cuda")
            res = env.step(acts, want_masks=True) if r % 2 else env.step_mixed(acts, "exiting", want_masks=True)
            assert torch.equal(res.action_masks, env.action_masks()), (which, r)
        env.close()
    # the split step: ccx_step_finish leaves the masks too
    env = ccx(_cfg(8), 100)
    env.make_reset_pool(3, 16)
    env.reset_from_pool()
    mo = torch.full((100, 8), 0xAB, dtype=torch.uint8, device="cuda")
    for r in range(24):
        env.step_begin(torch.randint(0, 5, (100, 8), dtype=torch.uint8, device="cuda"))
        env._bind_masks(mo)
        env._finish(None, None, None, True, False, True)
        assert torch.equal(mo, env.action_masks()), r
    env.step_finish()           # (the public call without masks unbinds)
    env.close()


# ------------------------------------------------------------------------------------------- nothing else changes
@pytest.mark.parametrize("N,E", [(3, 3), (8, 4096), (32, 1027), (64, 515)])
@pytest.mark.parametrize("mixed", [False, True])
def test_want_masks_leaves_every_other_output_and_the_state_alone(ccx, N, E, mixed):
    import torch
    cfg = _cfg(N)
    A, B = ccx(cfg, E), ccx(cfg, E)
    for h in (A, B):
        h.make_reset_pool(5, 64)
        h.reset_from_pool()
    gen = torch.Generator(device="cpu").manual_seed(N + E)
    for s in range(30):
        acts = torch.randint(0, 5, (E, N), dtype=torch.uint8, generator=gen).cuda()
        if mixed:
            ra = A.step_mixed(acts, "boarding", "greedy", want_compact=True, want_masks=True)
            rb = B.step_mixed(acts, "boarding", "greedy", want_compact=True)
        else:
            ra = A.step(acts, want_compact=True, want_masks=True)
            rb = B.step(acts, want_compact=True)
        assert ra.action_masks is not None and rb.action_masks is None
        for f in ("obs", "reward", "obs_compact"):
            assert torch.equal(_bits(getattr(ra, f)), _bits(getattr(rb, f))), (f, s)
        assert torch.equal(ra.agent_flags, rb.agent_flags) and torch.equal(ra.env_flags, rb.env_flags), s
    sa, sb = A.get_state(), B.get_state()
    for k in sa:
        np.testing.assert_array_equal(sa[k], sb[k], err_msg=k)
    assert A.counters() == B.counters()
    A.close()
    B.close()


# ------------------------------------------------------------------------------------------- the mask is what a step does
@pytest.mark.parametrize("N", [3, 8, 32])
def test_single_agent_probes_through_step_agree_with_the_mask(ccx, oracle, N):
    """For a live, active agent i: bit a set <=> a step whose action tensor is 255 everywhere except actions[i] = a
    changes agent i's position.  An arrived (inactive) agent never moves.  One probe env per (state, agent, direction)."""
    import torch
    cfg = _cfg(N, max_steps=1000)
    S = 24
    env = ccx(cfg, S * N * 4)
    st = random_states(oracle, env.params, S, 7 * N)
    rep = lambda a: np.repeat(a, N * 4, axis=0)  # noqa: E731
    env.set_state(**{k: rep(v) for k, v in st.items()}, step_count=np.zeros(S * N * 4, np.int32))
    masks = env.action_masks().cpu().numpy().reshape(S, N, 4, N)
    actions = np.full((S, N, 4, N), 255, np.uint8)
    for i in range(N):
        for a in range(4):
            actions[:, i, a, i] = a
    env.step(torch.from_numpy(actions.reshape(S * N * 4, N)).cuda(), want_obs=False)
    after = env.get_state()
    moved = ((after["x"] != rep(st["x"])) | (after["y"] != rep(st["y"]))).reshape(S, N, 4, N)
    done = (st["terminated"] != 0) | (st["truncated"] != 0)
    checked = 0
    for i in range(N):
        live_active = ~done[:, i] & (st["active"][:, i] != 0)
        for a in range(4):
            bit = ((masks[:, i, a, i] >> a) & 1) != 0
            np.testing.assert_array_equal(moved[:, i, a, i][live_active], bit[live_active], err_msg=f"agent {i} action {a}")
            assert not moved[:, i, a, i][st["active"][:, i] == 0].any()
            checked += int(live_active.sum())
    assert checked > S
    env.close()


# ------------------------------------------------------------------------------------------- graphs
def test_a_captured_step_with_masks_replays_the_eager_masks(ccx):
    import torch

    from collectivecrossing_amd import unpack_action_masks
    cfg = _cfg(8, max_steps=1000)
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
        B.step(acts, want_masks=True)                  # first call: the output buffers
        side.synchronize()
        B.reset(seeds)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            rb = B.step(acts, want_masks=True)
            legal = unpack_action_masks(rb.action_masks)                  # (captures too: no host-to-device copy)
        B.reset(seeds)                                 # (the capture ran nothing)
        side.synchronize()
        for _ in range(20):
            graph.replay()
        side.synchronize()
    for _ in range(20):
        ra = A.step(acts)
    eager = A.action_masks()
    torch.cuda.synchronize()
    assert torch.equal(rb.action_masks, eager) and bool((eager != 0x1F).any())
    assert torch.equal(legal, unpack_action_masks(eager)) and tuple(legal.shape) == (E, N, 5)
    assert torch.equal(_bits(ra.obs), _bits(rb.obs)) and torch.equal(ra.agent_flags, rb.agent_flags)
    A.close()
    B.close()


# ------------------------------------------------------------------------------------------- the layers above
def test_vector_policy_inputs_carry_the_masks(ccx):
    import torch

    from collectivecrossing_amd import unpack_action_masks
    from collectivecrossing_amd.vector import VectorCollectiveCrossing
    cfg = _cfg(8, max_steps=6)
    E, nb = 33, 5
    vec = VectorCollectiveCrossing(cfg, E)

    def check(where):
        pi = vec.policy_inputs(obs)
        ref = unpack_action_masks(vec.batch.action_masks())
        assert pi["boarding"]["action_mask"].dtype is torch.bool and tuple(pi["exiting"]["action_mask"].shape) == (E, 3, 5)
        assert torch.equal(pi["boarding"]["action_mask"], ref[:, :nb]) and torch.equal(pi["exiting"]["action_mask"], ref[:, nb:]), where

    obs = vec.reset(np.arange(E, dtype=np.uint64))
    check("reset")
    for s in range(4):
        obs = vec.step(torch.randint(0, 5, (E, 8), dtype=torch.uint8, device="cuda")).obs
        check(f"step {s}")
    restarted = False
    for s in range(8):
        rng = np.random.default_rng(s)
        dicts = [{a: int(rng.integers(0, 5)) for a in vec.envs[e].agents} for e in range(E)]
        obs = vec.step_dicts(dicts, auto_reset=True, seed0=1000).obs
        restarted |= bool(vec._restarted.any())
        check(f"step_dicts {s}")
    assert restarted
    vec.close()


def test_env_action_masks_agree_with_the_batch_path(ccx):
    from collectivecrossing_amd import CollectiveCrossingEnv
    env = CollectiveCrossingEnv(_cfg(8, max_steps=30))
    env.reset(seed=3)
    rng = np.random.default_rng(0)
    for s in range(30):
        got = env.action_masks()
        env._upload()
        dev = env._batch.action_masks().cpu().numpy()[0]
        assert list(got) == env.agents
        for i, aid in enumerate(env.possible_agents):
            if aid in got:
                assert int((got[aid].astype(np.uint8) << np.arange(5, dtype=np.uint8)).sum()) == int(dev[i]), (s, aid)
            else:
                assert dev[i] == WAIT_ONLY
        if not env.agents:
            break
        env.step({a: int(rng.integers(0, 5)) for a in env.agents})
    env.close()
