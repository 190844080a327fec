"""Advantages and returns on the device (include/ccx.h: CCX_GAE) against the NumPy spec (tests/_gae_spec.py): adversarial
synthetic cases across the kernel's chunk boundaries and column counts, every output element written, a real auto-reset
trajectory with final_obs, a captured graph, and the refusals.  f32 values are compared as bit patterns throughout."""

import numpy as np
import pytest
from _fixtures import Golden
from _gae_spec import bits32, gae_spec, make_gae_case, step_classes

pytestmark = pytest.mark.gpu

CONFIG_OF_N = {3: "g7_n3_small", 8: "g8_rollout_c1", 1: "g7_n1_exiting_only", 64: "g4_c5_all_at_dest_greedy_32_32",
               50: "g4_c5_all_at_dest_greedy_25_25"}
# K: one step (its own branch), two, and C - 1, C, C + 1, 2C - 1, 2C, 2C + 1, 4C + 2 for the kernel's register chunk of
# C = 8 steps (GAE_CHUNK) -- and for C = 16, the other length the kernel is built with for timing
SYNTHETIC_K = (1, 2, 7, 8, 9, 15, 16, 17, 31, 32, 33, 34, 66)
# column counts off a multiple of 64 (15, 536, 130, 192 = three full waves of one-env waves, 450), one agent, a full-wave env
SHAPES = ((5, 3), (67, 8), (130, 1), (3, 64), (9, 50))
GAMMA, LAM = 0.99, 0.95


@pytest.fixture(scope="module")
def batches():
    import torch

    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    from collectivecrossing_amd.batched import BatchedCollectiveCrossing

    cache = {}

    def get(N, E):
        if (N, E) not in cache:
            cache[N, E] = BatchedCollectiveCrossing(Golden(CONFIG_OF_N[N]).config, E)
            assert cache[N, E].num_agents == N
        return cache[N, E]

    yield get
    for b in cache.values():
        b.close()


@pytest.fixture(scope="module")
def cases():
    """A generator case and the spec's answers with and without final_values, made once per (K, E, N)."""
    cache = {}

    def get(K, E, N):
        if (K, E, N) not in cache:
            case = make_gae_case(K, E, N, seed=K * 1000 + E, with_final=True)
            a = (case["reward"], case["agent_flags"], case["env_flags"], case["values"], case["last_values"])
            cache[K, E, N] = (case, gae_spec(*a, case["final_values"], GAMMA, LAM), gae_spec(*a, None, GAMMA, LAM))
        return cache[K, E, N]

    return get


KEYS = ("reward", "agent_flags", "env_flags", "values", "last_values", "final_values")


def _dev(case):
    import torch

    return {k: torch.from_numpy(np.ascontiguousarray(case[k])).cuda() for k in KEYS}


def _host(g):
    return (g.advantages.cpu().numpy(), g.returns.cpu().numpy(), None if g.valid is None else g.valid.cpu().numpy())


def _assert_equal(got, want, tag):
    for g, w, name in zip(got, want, ("advantages", "returns", "valid")):
        if g is not None:
            np.testing.assert_array_equal(bits32(g), bits32(w), err_msg=f"{name} {tag}")


def _traj(d):
    return (d["reward"], d["agent_flags"], d["env_flags"])


# ------------------------------------------------------------------------------------------------- 1. bits against the spec
@pytest.mark.parametrize("K", SYNTHETIC_K)
@pytest.mark.parametrize("E,N", SHAPES)
def test_bits_against_the_spec(batches, cases, E, N, K):
    batch = batches(N, E)
    case, with_final, without = cases(K, E, N)
    d = _dev(case)
    g = batch.compute_gae(_traj(d), d["values"], d["last_values"], d["final_values"], gamma=GAMMA, lam=LAM)
    batch.synchronize()
    _assert_equal(_host(g), with_final, f"E {E} N {N} K {K} final_values")
    g = batch.compute_gae(_traj(d), d["values"], d["last_values"], None, gamma=GAMMA, lam=LAM)
    batch.synchronize()
    _assert_equal(_host(g), without, f"E {E} N {N} K {K} no final_values")
    for final, want in ((d["final_values"], with_final), (None, without)):             # valid = None
        out = batch.alloc_gae(K, want_valid=False)
        assert out.valid is None
        batch.compute_gae(_traj(d), d["values"], d["last_values"], final, gamma=GAMMA, lam=LAM, out=out)
        batch.synchronize()
        _assert_equal(_host(out), want, f"E {E} N {N} K {K} no valid")
    assert not np.isnan(with_final[0]).any() and np.isnan(case["values"]).any() and np.isnan(case["reward"]).any()


# ------------------------------------------------------------------------------------------------- 2. every element written
@pytest.mark.parametrize("K,E,N", ((1, 5, 3), (17, 67, 8), (34, 9, 50)))
def test_every_element_is_written_and_no_input_is(batches, cases, K, E, N):
    import torch

    batch = batches(N, E)
    case, with_final, without = cases(K, E, N)
    d = _dev(case)
    before = {k: v.clone() for k, v in d.items()}
    for final, want in ((d["final_values"], with_final), (None, without)):
        out = batch.alloc_gae(K)
        for t in (out.advantages, out.returns, out.valid):
            t.view(torch.uint8).fill_(0xFF)
        torch.cuda.synchronize()
        batch.compute_gae(_traj(d), d["values"], d["last_values"], final, gamma=GAMMA, lam=LAM, out=out)
        batch.synchronize()
        _assert_equal(_host(out), want, f"prefilled K {K} E {E} N {N}")
        live = (case["agent_flags"] & 4) != 0
        assert (~live).any() and not bits32(out.advantages.cpu().numpy())[~live].any()      # +0.0 where not live
    for k in KEYS:
        assert torch.equal(d[k].view(torch.uint8), before[k].view(torch.uint8)), k


# ------------------------------------------------------------------------------------------------- 3. a real trajectory
def _allowed_to_change(live, term, cut):
    """Steps whose outputs may depend on final_values: the cut steps and the steps that continue into them."""
    K = live.shape[0]
    allowed = np.zeros_like(live)
    tainted = np.zeros(live.shape[1:], bool)
    for s in range(K - 1, -1, -1):
        tainted = np.where(~live[s] | term[s], False, np.where(cut[s], True, tainted))
        allowed[s] = tainted
    return allowed


def test_real_trajectory_with_final_obs(batches):
    import torch

    E, N, K = 32, 8, 60
    batch = batches(N, E)                                             # max_steps = 25: every env restarts at least twice
    batch.make_reset_pool(seed0=5, size=64)
    batch.reset_from_pool()
    obs0 = batch.observe()
    traj = batch.alloc_rollout(K, want_final=True)
    batch.rollout_policy(K, "greedy", auto_reset=True, reset_obs="next", out=traj)
    batch.synchronize()
    af, ef = traj.agent_flags.cpu().numpy(), traj.env_flags.cpu().numpy()
    live, term, cut, cont = step_classes(af, ef)
    assert term.any() and (live & ((af & 2) != 0)).any() and (ef & 4).any()       # terminated, truncated, EF_RESET
    # the critic: a seeded linear map of the rows, evaluated with torch
    w = torch.from_numpy(np.random.default_rng(3).standard_normal(batch.obs_len).astype(np.float32)).cuda()
    values = torch.empty((K, E, N), dtype=torch.float32, device="cuda")
    values[0] = obs0 @ w                                              # the rows step 0 acted on
    values[1:] = traj.obs[:-1] @ w                                    # NEXT mode: the new episode's rows at restarted envs
    last_values = (traj.obs[K - 1] @ w).contiguous()
    reset = (traj.env_flags & 4) != 0
    final_values = torch.where(reset[..., None], traj.final_obs @ w, torch.nan).contiguous()     # evaluated at EF_RESET rows only
    torch.cuda.synchronize()
    host = [t.cpu().numpy() for t in (traj.reward, traj.agent_flags, traj.env_flags, values, last_values, final_values)]
    with_final = batch.compute_gae(traj, values, last_values, final_values, gamma=GAMMA, lam=LAM)
    without = batch.compute_gae(traj, values, last_values, None, gamma=GAMMA, lam=LAM)
    batch.synchronize()
    want_with, want_without = gae_spec(*host, GAMMA, LAM), gae_spec(*host[:5], None, GAMMA, LAM)
    _assert_equal(_host(with_final), want_with, "real trajectory, final_values")
    _assert_equal(_host(without), want_without, "real trajectory, no final_values")
    assert not np.isnan(want_with[0]).any() and not np.isnan(want_with[1]).any()
    # final_values = None changes the outputs at the cut steps and at the steps of their episodes before them, nothing else
    diff = bits32(_host(with_final)[0]) != bits32(_host(without)[0])
    allowed = _allowed_to_change(live, term, cut)
    assert not (diff & ~allowed).any()
    # (a bootstrap value above 1e-3 cannot be absorbed: rewards and values here stay below 1e3, where an f32 ulp is 6e-5)
    assert np.abs(host[3]).max() < 1e3 and np.abs(host[0][live]).max() < 1e3
    nonzero = cut & (np.abs(np.nan_to_num(host[5])) > 1e-3)
    assert nonzero.any() and diff[nonzero].all() and diff[allowed & ~cut].any()
    rdiff = bits32(_host(with_final)[1]) != bits32(_host(without)[1])
    assert not (rdiff & ~allowed).any() and rdiff[nonzero].all()
    np.testing.assert_array_equal(_host(with_final)[2], _host(without)[2])


# ------------------------------------------------------------------------------------------------- 4. graph
def test_captured_rollout_and_gae():
    import torch

    from collectivecrossing_amd.batched import BatchedCollectiveCrossing

    E, N, K = 32, 8, 20
    B = BatchedCollectiveCrossing(Golden(CONFIG_OF_N[N]).config, E)
    B.make_reset_pool(seed0=5, size=64)
    B.reset_from_pool()
    rng = np.random.default_rng(4)
    values = torch.from_numpy(rng.standard_normal((K, E, N)).astype(np.float32)).cuda()
    last_values = torch.from_numpy(rng.standard_normal((E, N)).astype(np.float32)).cuda()
    final_values = torch.from_numpy(rng.standard_normal((K, E, N)).astype(np.float32)).cuda()
    side = torch.cuda.Stream()
    B.use_stream(side)
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        traj = B.alloc_rollout(K, want_final=True)
        acts = torch.empty((K, E, N), dtype=torch.uint8, device="cuda")
        out = B.alloc_gae(K)
        B.rollout_policy(K, "greedy", auto_reset=True, reset_obs="next", out=traj, actions_out=acts)   # eager first
        B.compute_gae(traj, values, last_values, final_values, gamma=GAMMA, lam=LAM, out=out)
        side.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            B.rollout_policy(K, "greedy", auto_reset=True, reset_obs="next", out=traj, actions_out=acts)
            B.compute_gae(traj, values, last_values, final_values, gamma=GAMMA, lam=LAM, out=out)
        side.synchronize()
        for _ in range(2):
            out.advantages.fill_(7.0)
            graph.replay()
            side.synchronize()
            replayed = _host(out)
            eager = B.compute_gae(traj, values, last_values, final_values, gamma=GAMMA, lam=LAM)   # on the replay's trajectory
            side.synchronize()
            _assert_equal(replayed, _host(eager), "graph replay against the eager call")
            host = [t.cpu().numpy() for t in (traj.reward, traj.agent_flags, traj.env_flags, values, last_values, final_values)]
            _assert_equal(replayed, gae_spec(*host, GAMMA, LAM), "graph replay against the spec")
    B.use_stream(None)
    B.close()


# ------------------------------------------------------------------------------------------------- 5. errors
def test_refusals_leave_the_batch_usable(batches, cases):
    import torch

    from collectivecrossing_amd import _abi

    K, E, N = 9, 5, 3
    batch = batches(N, E)
    case, with_final, _ = cases(K, E, N)
    d = _dev(case)
    ok = dict(traj=_traj(d), values=d["values"], last_values=d["last_values"], final_values=d["final_values"])
    bad = [
        dict(ok, gamma=1.5), dict(ok, lam=float("nan")), dict(ok, gamma=-0.1),
        dict(ok, traj=tuple(t[:0] for t in _traj(d)), values=d["values"][:0], final_values=None),          # K = 0
        dict(ok, values=d["values"].double()),                                                               # f64 values
        dict(ok, last_values=d["last_values"][:, :2].contiguous()),                                          # wrong shape
        dict(ok, values=d["values"][:-1]),
        dict(ok, values=d["values"].cpu()),                                                                  # a CPU tensor
        dict(ok, final_values=d["final_values"].transpose(0, 1).contiguous().transpose(0, 1)),               # not contiguous
        dict(ok, traj=(d["reward"].float(), d["agent_flags"], d["env_flags"])),
        dict(ok, out=batch.alloc_gae(K + 1)),
    ]
    for kw in bad:
        with pytest.raises(ValueError):
            batch.compute_gae(**kw)
    # the library's own refusals (the wrapper refuses first, so they are reached through the bindings)
    lib, h = batch._lib, batch._h
    out = batch.alloc_gae(K)
    p = [t.data_ptr() for t in (d["reward"], d["agent_flags"], d["env_flags"], d["values"], d["last_values"], d["final_values"])]
    o = [out.advantages.data_ptr(), out.returns.data_ptr(), out.valid.data_ptr()]
    for k, ptrs, gamma, lam, outs, word in ((K, p, 1.5, 0.5, o, "gamma"), (K, p, 0.5, float("nan"), o, "lam"),
                                           (0, p, 0.5, 0.5, o, "num_steps"), (K, [None] + p[1:], 0.5, 0.5, o, "NULL"),
                                           (K, p, 0.5, 0.5, [o[0], None, o[2]], "NULL")):
        assert lib.ccx_gae(h, k, *ptrs, gamma, lam, *outs) == _abi.EINVAL
        assert word in lib.ccx_last_error().decode()
    g = batch.compute_gae(gamma=GAMMA, lam=LAM, **ok)
    batch.synchronize()
    _assert_equal(_host(g), with_final, "after the refusals")
    assert torch.cuda.is_available()
