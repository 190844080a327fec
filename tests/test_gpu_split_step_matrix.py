"""The split-step kernels (csrc/ccx_split_step.hip: step_begin_kernel, step_finish_kernel<PAIR>) against the NumPy statement of
their contract (tests/_split_step_spec.py, pinned to the reference on the CPU by tests/test_split_step_spec.py) across agent
counts, batch sizes, launch shapes, caller-array values, output addresses, reset pools and malformed input.  Every comparison
is exact (bytes / u64 bit patterns), state included, after every half step.  Inputs are seeded (tests/_split_step_cases.py).

Wall time on an MI355X and the mutation check are reported with the change that added this file."""

import ctypes as C

import _split_step_cases as cases
import _split_step_spec as spec
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SENTINEL = 0xA5
COUNTERS = ("env_steps", "agent_steps", "live_agent_steps", "episodes", "moves", "arrivals")


@pytest.fixture(scope="module")
def ccx():
    import torch

    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    from collectivecrossing_amd.batched import BatchedCollectiveCrossing
    return BatchedCollectiveCrossing


class _Region:
    """``nbytes`` of device memory at ``lead`` bytes into a larger buffer filled with a sentinel byte."""

    def __init__(self, nbytes, lead, dtype):
        import torch
        self.nbytes, self.lead, self.dtype = int(nbytes), int(lead), dtype
        self.whole = torch.full((self.lead + self.nbytes + 64,), SENTINEL, dtype=torch.uint8, device="cuda")
        assert self.whole.data_ptr() % 64 == 0
        self.ptr = self.whole.data_ptr() + self.lead

    def read(self, what):
        host = self.whole.cpu().numpy()
        assert (host[:self.lead] == SENTINEL).all(), f"{what}: bytes in front of the region were written"
        assert (host[self.lead + self.nbytes:] == SENTINEL).all(), f"{what}: bytes behind the region were written"
        return host[self.lead:self.lead + self.nbytes].copy().view(self.dtype)


def _dev(a):
    import torch
    if a is None:
        return None
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.int64) if a.dtype == np.uint64 else a).cuda()


def _raw_finish(batch, r, t, u, regions, auto_reset=False):
    """ccx_step_finish through the ctypes binding with the caller's own pointers; returns the status code."""
    from collectivecrossing_amd import _abi
    ptr = lambda k: regions[k].ptr if regions.get(k) is not None else None  # noqa: E731
    so = _abi.CcxStepOut(ptr("obs"), ptr("reward"), ptr("agent_flags"), ptr("env_flags"), ptr("obs_compact"))
    keep = [_dev(r), _dev(t), _dev(u)]
    rc = batch._lib.ccx_step_finish(batch._h, *[C.c_void_p(None if k is None else k.data_ptr()) for k in keep], C.byref(so),
                                    C.c_void_p(ptr("term_present")), int(bool(auto_reset)))
    batch.synchronize()
    return rc


def _regions(E, N, off, want_obs=True, want_compact=True):
    """Output regions: byte streams ``off`` bytes past a 4-byte boundary, rewards 8-byte aligned and no more, rows at the
    minimum legal alignment for the parity of N (16 bytes, 8 for an odd count), compact rows 16-byte aligned."""
    L = 6 + 4 * N
    reg = dict(reward=_Region(E * N * 8, 72, np.uint64), agent_flags=_Region(E * N, 64 + off, np.uint8),
               term_present=_Region(E * N, 64 + (off + 1) % 4, np.uint8), env_flags=_Region(E, 64 + (off + 2) % 4, np.uint8))
    reg["obs"] = _Region(E * N * L * 4, 80 if N % 2 == 0 else 72, np.uint32) if want_obs else None
    reg["obs_compact"] = _Region(E * N * 16, 80, np.uint32) if want_compact else None
    return reg


def _assert_state(batch, want, tag):
    got = batch.get_state()
    for k in spec.STATE_KEYS:
        np.testing.assert_array_equal(got[k], want[k], err_msg=f"state {k}: {tag}")


def _compare_finish(oracle, p, mid, f, regions, tag):
    E, N = mid["x"].shape
    np.testing.assert_array_equal(regions["reward"].read("reward"), f.reward_bits.ravel(), err_msg=f"reward bits: {tag}")
    np.testing.assert_array_equal(regions["agent_flags"].read("agent_flags"), f.agent_flags.ravel(), err_msg=f"agent_flags: {tag}")
    np.testing.assert_array_equal(regions["term_present"].read("term_present"), f.term_present.ravel(), err_msg=f"term_present: {tag}")
    np.testing.assert_array_equal(regions["env_flags"].read("env_flags"), f.env_flags, err_msg=f"env_flags: {tag}")
    if regions.get("obs_compact") is not None:
        np.testing.assert_array_equal(regions["obs_compact"].read("obs_compact"), f.obs_compact.view(np.uint32).ravel(),
                                      err_msg=f"obs_compact: {tag}")
    if regions.get("obs") is not None:
        np.testing.assert_array_equal(regions["obs"].read("obs"), spec.observe(oracle, p, mid).view(np.uint32).ravel(),
                                      err_msg=f"obs rows: {tag}")


def _run_case(ccx, oracle, n, grid, E, seed, *, steps=3, shape=None, writers=None, null=(), config=None, tables=None,
              auto_reset=False, pool=None, env_offset=0, total_envs=None, state=None, with_order=True, inputs=None):
    """``steps`` x (begin -> caller arrays -> finish) on one handle against the spec; the last step runs with obs = NULL
    (and, for an odd seed, without compact rows as well).  ``null`` names the arrays passed as NULL (the built-in rule);
    ``inputs`` = per-step (actions, order, reward, terminated, truncated) instead of drawing them.
    Returns (launch shape, spec counters, final state, the per-step inputs)."""
    from collectivecrossing_amd.params import lower_config
    cfg = config if config is not None else cases.make_config(*grid, n)
    p = lower_config(cfg)
    rng = np.random.default_rng(seed)
    batch = ccx(cfg, E, env_offset=env_offset, total_envs=total_envs)
    try:
        if shape is not None:
            batch.set_launch_shape(*shape)
        if writers is not None:
            batch.set_writers(writers)
        if tables is not None:
            batch.set_reward_table(*tables[0])
            batch.set_terminated_table(*tables[1])
        ls = batch.launch_shape()
        tag0 = f"N={n} grid={grid} E={E} seed={seed} asked={shape} writers={writers} null={null} launch_shape={ls}"
        st = state if state is not None else cases.random_state(rng, p, E, n, kind_offset=seed)
        batch.set_state(**st)
        if pool is not None:
            batch.set_reset_pool(pool)
        batch.zero_counters()
        want = dict.fromkeys(COUNTERS, 0)
        drawn = []
        for s in range(steps):
            tag = f"{tag0} step {s}"
            if inputs is None:
                acts = cases.random_actions(rng, E, n)
                order = cases.random_orders(rng, E, n) if (with_order and s % 2 == 0) else None
                r, t, u = cases.caller_arrays(rng, st, kind_offset=seed)
            else:
                acts, order, r, t, u = inputs[s]
            drawn.append((acts, order, r, t, u))
            batch.step_begin(acts, order)
            mid, mv, ar = spec.begin(p, st, acts, order, oracle=oracle)
            _assert_state(batch, mid, tag + " after begin")
            if null:
                br, bt, bu = spec.builtin_arrays(oracle, p, mid, tables)
                r, t, u = (br if "reward" in null else r), (bt if "terminated" in null else t), (bu if "truncated" in null else u)
            f = spec.finish(p, mid, r, t, u, auto_reset=auto_reset, pool=pool, env_offset=env_offset, total_envs=total_envs)
            rows = s < steps - 1
            reg = _regions(E, n, (seed + s) % 4, want_obs=rows, want_compact=rows or seed % 2 == 0)
            rc = _raw_finish(batch, None if "reward" in null else r, None if "terminated" in null else t,
                             None if "truncated" in null else u, reg, auto_reset)
            assert rc == 0, (tag, batch._lib.ccx_last_error())
            _compare_finish(oracle, p, mid, f, reg, tag)
            _assert_state(batch, f.state, tag + " after finish")
            st = f.state
            want["moves"] += mv
            want["arrivals"] += ar
            for k in f.counters:
                want[k] += f.counters[k]
            del reg
        assert batch.counters() == want, tag0
        return ls, want, st, drawn
    finally:
        batch.close()


# ---------------------------------------------------------------------------------------------------------------------
# the shape matrix
# ---------------------------------------------------------------------------------------------------------------------
def _picked_shape(ccx, cfg, E, shape=None, writers=None):
    """launch_shape() of a probe handle of E envs."""
    b = ccx(cfg, E)
    try:
        if shape is not None:
            b.set_launch_shape(*shape)
        if writers is not None:
            b.set_writers(writers)
        return b.launch_shape()
    finally:
        b.close()


def _envs_of(ls, n):
    """(envs per wave, envs per workgroup) of a launch shape: what finish rides on."""
    ew = ls["lanes_per_wave"] // cases.lane_group(n)
    return ew, ew * ls["waves_per_block"]


def _class_envs_of_the_picked_shape(ccx, cfg, n, cls):
    """Batch size of an E class measured on the shape the library itself picks: the shape depends on E, so the size is
    re-derived from launch_shape() of a probe handle until it stays put (a few rounds at most)."""
    E = cases.class_envs(n, cls)
    if cls in ("one", "hundreds", "thousands"):
        return E
    for _ in range(4):
        ew, wg = _envs_of(_picked_shape(ccx, cfg, E), n)
        new = {"wave-1": max(ew - 1, 1), "wave+1": ew + 1, "block-1": max(wg - 1, 1), "block+1": wg + 1}[cls]
        if new == E:
            break
        E = new
    return E


def test_default_shape_matrix(ccx, oracle):
    """Every agent count x every batch class (the grid cycling, so that every count meets every grid) on the shape the
    library picks, with all three caller arrays.  The wave / workgroup classes are sized from launch_shape()."""
    ran, seen = 0, {n: dict(partial_wave=False, partial_block=False, shapes=[]) for n in cases.AGENT_COUNTS}
    for k, (n, grid, cls) in enumerate(cases.matrix_cases()):
        E = _class_envs_of_the_picked_shape(ccx, cases.make_config(*grid, n), n, cls)
        ls = _run_case(ccx, oracle, n, grid, E, seed=100 + k)[0]
        ew, wg = _envs_of(ls, n)
        seen[n]["partial_wave"] |= E % ew != 0 and E > ew
        seen[n]["partial_block"] |= E % wg != 0 and E > wg
        seen[n]["shapes"].append((cls, E, ls["lanes_per_wave"], ls["waves_per_block"]))
        ran += 1
    assert ran == 105
    for n, v in seen.items():
        # a last wave that is not full needs more than one env per wave: counts up to 32 (G <= 32) can have it.  A last
        # workgroup that is not full needs more than one env per workgroup: where the library picks one-tile workgroups of one
        # env at every size (some of the 64-lane counts), only the explicit shapes below reach it
        assert v["partial_block"] or all(c[2] // cases.lane_group(n) * c[3] == 1 for c in v["shapes"]), (n, v)
        assert v["partial_wave"] or cases.lane_group(n) == 64, (n, v)


@pytest.mark.parametrize("n", [8, 32])
def test_8192_tiles(ccx, oracle, n):
    """A batch of 8192 full waves of the begin kernel (and at least as many tiles of the finish kernel), plus one env."""
    import torch
    E = 8192 * (64 // cases.lane_group(n)) + 1
    assert E * n * (6 + 4 * n) * 4 < 1_000_000_000
    ls = _run_case(ccx, oracle, n, (40, 30), E, seed=700 + n, steps=2)[0]
    assert ls["num_blocks"] * ls["waves_per_block"] >= 8192, ls
    torch.cuda.empty_cache()


def test_explicit_launch_shapes_and_writers(ccx, oracle):
    """Every (lanes_per_wave, waves_per_block) of the explicit list at one workgroup of the shape that results - 1 / + 1 envs,
    and 1 .. 3 writers per tile; the pairs ccx_set_launch_shape must refuse are refused.  A workgroup holds at most 512
    threads = 8 waves, one simulation wave plus the writers per tile: 3 and 4 tiles per workgroup are asked for together
    with ONE writer (4 x 2 = 8 waves) and must be granted; with the library's own 2 or 3 writers, 1 and 2 tiles must be."""
    from collectivecrossing_amd._lib import CcxError
    ran = refused = 0
    tiles_seen = set()
    for a, n in enumerate(cases.AGENT_COUNTS):
        grid = cases.GRIDS[a % 2]
        cfg = cases.make_config(*grid, n)
        for b, (lanes, wpb) in enumerate(cases.explicit_shapes(n)):
            writers = 1 if wpb >= 3 else None
            ew, wg = _envs_of(_picked_shape(ccx, cfg, 4 * wpb * (lanes // cases.lane_group(n)), (lanes, wpb), writers), n)
            E = wg + 1 if b % 2 else max(wg - 1, 1)
            ls = _run_case(ccx, oracle, n, grid, E, seed=300 + 16 * a + b, shape=(lanes, wpb), writers=writers, steps=3)[0]
            assert ls["lanes_per_wave"] == lanes and ls["waves_per_block"] == wpb, (n, lanes, wpb, ls)
            assert _envs_of(ls, n) == (ew, wg) and (E == wg - 1 or E == wg + 1 or wg == 1), (n, E, ls)
            tiles_seen.add((n, wpb))
            ran += 1
        for w in (1, 2, 3):
            wg = _envs_of(_picked_shape(ccx, cfg, 300, writers=w), n)[1]
            ls = _run_case(ccx, oracle, n, grid, 2 * wg + 1, seed=500 + 4 * a + w, writers=w, steps=3)[0]
            assert ls["writers_per_tile"] == w, (n, w, ls)
            ran += 1
        probe = ccx(cfg, 5)
        for lanes, wpb in cases.refused_shapes(n):
            with pytest.raises(CcxError):
                probe.set_launch_shape(lanes, wpb)
            refused += 1
        with pytest.raises(CcxError):
            probe.set_writers(8)
        probe.close()
    # 15 counts x 3 writers + 12 pairs for the 8 counts with three distinct lane widths (G <= 16), 8 for the 3 counts with
    # G = 32, 4 for the 4 counts with G = 64
    assert ran == 15 * 3 + 8 * 12 + 3 * 8 + 4 * 4 == 181, ran
    assert tiles_seen == {(n, w) for n in cases.AGENT_COUNTS for w in (1, 2, 3, 4)}
    # 3 for every count, + "half a lane group" for the 14 counts with G > 1, + 48 lanes for the 7 counts with G = 32 / 64
    assert refused == 3 * 15 + 14 + 7 == 66, refused


# ---------------------------------------------------------------------------------------------------------------------
# each array alone, the built-in rules for the others
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("reward", ["default", "simple_distance", "binary", "constant_negative"])
@pytest.mark.parametrize("terminated", ["individual_at_destination", "all_at_destination"])
def test_each_array_alone_with_the_built_in_rules(ccx, oracle, reward, terminated):
    for k, (n, grid) in enumerate([(8, (12, 8)), (11, (40, 30))]):
        cfg = cases.make_config(*grid, n, max_steps=4, reward=reward, terminated=terminated)
        for j, null in enumerate([("terminated", "truncated"), ("reward", "truncated"), ("reward", "terminated"),
                                  ("reward", "terminated", "truncated")]):
            _run_case(ccx, oracle, n, grid, 131, seed=900 + 10 * k + j, config=cfg, null=null, steps=4)


def test_each_array_alone_with_position_only_tables(ccx, oracle):
    from collectivecrossing_amd.params import lower_config
    n, grid = 8, (12, 8)
    p = lower_config(cases.make_config(*grid, n))
    rng = np.random.default_rng(77)
    shape = (p.height + 1, p.width + 1)
    rew = tuple(cases.REWARD_BITS[rng.integers(0, len(cases.REWARD_BITS), size=shape)].view(np.float64) for _ in range(2))
    term = tuple((rng.random(shape) < 0.4).astype(np.uint8) for _ in range(2))
    for j, null in enumerate([("terminated", "truncated"), ("reward", "truncated"), ("reward", "terminated", "truncated")]):
        _run_case(ccx, oracle, n, grid, 131, seed=950 + j, null=null, tables=(rew, term), steps=3)


def test_bool_arrays_through_step_finish(ccx, oracle):
    """``BatchedCollectiveCrossing.step_finish`` with torch.bool termination / truncation tensors."""
    import torch

    from collectivecrossing_amd.params import lower_config
    n, grid, E = 7, (12, 8), 67
    cfg = cases.make_config(*grid, n)
    p = lower_config(cfg)
    rng = np.random.default_rng(5)
    batch = ccx(cfg, E)
    st = cases.random_state(rng, p, E, n)
    batch.set_state(**st)
    for s in range(3):
        acts = cases.random_actions(rng, E, n)
        batch.step_begin(acts)
        mid = spec.begin(p, st, acts, None, oracle=oracle)[0]
        r, t, u = cases.caller_arrays(rng, mid)
        tb, ub = t == 1, u != 0
        f = spec.finish(p, mid, r, tb.astype(np.int8), ub.astype(np.uint8))
        res = batch.step_finish(torch.from_numpy(r.view(np.float64).copy()), torch.from_numpy(tb), torch.from_numpy(ub), want_compact=True)
        np.testing.assert_array_equal(res.reward.cpu().numpy().view(np.uint64), f.reward_bits)
        np.testing.assert_array_equal(res.agent_flags.cpu().numpy(), f.agent_flags)
        np.testing.assert_array_equal(res.env_flags.cpu().numpy(), f.env_flags)
        assert res.term_present.cpu().numpy().all()
        np.testing.assert_array_equal(res.obs.cpu().numpy().view(np.uint32), spec.observe(oracle, p, mid).view(np.uint32))
        st = f.state
        _assert_state(batch, st, f"bool arrays step {s}")
    batch.close()


# ---------------------------------------------------------------------------------------------------------------------
# addresses
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [8, 11])
def test_misaligned_buffers_are_refused_without_a_launch(ccx, oracle, n):
    from collectivecrossing_amd import _abi
    from collectivecrossing_amd.params import lower_config
    E = 9
    cfg = cases.make_config(12, 8, n)
    p = lower_config(cfg)
    batch = ccx(cfg, E)
    st = cases.random_state(np.random.default_rng(1), p, E, n)
    batch.set_state(**st)
    r, t, u = cases.caller_arrays(np.random.default_rng(2), st)
    good = _regions(E, n, 0)
    rd = _dev(r)
    for what, shift in (("obs", 8 if n % 2 == 0 else 4), ("reward", 4), ("obs_compact", 8), ("user reward", 4)):
        reg = dict(good)
        so = {k: (reg[k].ptr if reg.get(k) is not None else None) for k in ("obs", "reward", "agent_flags", "env_flags", "obs_compact")}
        rptr = rd.data_ptr()
        if what == "user reward":
            rptr += shift
        else:
            so[what] += shift
        out = _abi.CcxStepOut(so["obs"], so["reward"], so["agent_flags"], so["env_flags"], so["obs_compact"])
        rc = batch._lib.ccx_step_finish(batch._h, C.c_void_p(rptr), None, None, C.byref(out), None, 0)
        assert rc == _abi.EINVAL, what
    batch.synchronize()
    for k, reg in good.items():
        assert (reg.whole.cpu().numpy() == SENTINEL).all(), f"{k} was written by a refused call"
    _assert_state(batch, st, "a refused call changed the state")
    batch.close()


@pytest.mark.parametrize("E", [5, 6, 7])
def test_rollout_slab_of_an_array_strategy_batch(ccx, oracle, E):
    """``rollout()`` of a batch with array-form strategies points finish at step s of the caller's [K][E][N] slabs
    (batched.py: _finish_into): 11 agents x 5 / 6 / 7 envs = 55 / 66 / 77 bytes per step, so the byte streams of the steps
    start at every residue mod 4.  Every step's slice of all six outputs equals the spec fed with what the config's own
    classes returned on a twin; the slabs live inside sentinel-filled buffers that stay intact around them."""
    import sys
    from pathlib import Path

    import torch
    sys.path.insert(0, str(Path(__file__).resolve().parent / "golden"))
    import array_strategies as ast

    from collectivecrossing_amd import configs as CFG
    from collectivecrossing_amd import strategies
    from collectivecrossing_amd.batched import RolloutResult
    from collectivecrossing_amd.params import lower_config
    undo = ast.register(strategies, ast.make_g15(strategies.RewardFunction, strategies.TerminatedFunction,
                                                 strategies.TruncatedFunction), ast.G15_NAMES)
    try:
        K, n = 5, 11
        config = ast.g15_config(CFG, CFG, CFG, CFG, ast.BIG, 3)
        p = lower_config(config, allow_position_only=True, allow_array_form=True)
        assert p.num_agents == n and (E * n) % 4 == 8 - E       # 3, 2, 1: step 1 starts at that residue
        L = 6 + 4 * n
        rng = np.random.default_rng(E)
        roll, twin = ccx(config, E), ccx(config, E)
        assert roll.has_array_strategies
        st = cases.random_state(rng, p, E, n, flags=False)
        for b in (roll, twin):
            b.set_state(**st)
        shapes = dict(obs=((K, E, n, L), torch.float32, 72), reward=((K, E, n), torch.float64, 72),
                      agent_flags=((K, E, n), torch.uint8, 65), env_flags=((K, E), torch.uint8, 67),
                      obs_compact=((K, E, n, 4), torch.float32, 80), term_present=((K, E, n), torch.uint8, 66))
        whole, views = {}, {}
        for k, (shape, dt, lead) in shapes.items():
            nbytes = int(np.prod(shape)) * torch.empty((), dtype=dt).element_size()
            whole[k] = torch.full((lead + nbytes + 64,), SENTINEL, dtype=torch.uint8, device="cuda")
            views[k] = whole[k][lead:lead + nbytes].view(dt).view(shape)
        out = RolloutResult(views["obs"], views["reward"], views["agent_flags"], views["env_flags"], views["obs_compact"],
                            views["term_present"])
        acts = np.stack([cases.random_actions(rng, E, n) for _ in range(K)])
        order = np.stack([cases.random_orders(rng, E, n) for _ in range(K)])
        assert roll.rollout(acts, order, out=out, want_compact=True) is out
        roll.synchronize()
        host = {k: views[k].cpu().numpy() for k in views}
        for k, (shape, dt, lead) in shapes.items():
            w = whole[k].cpu().numpy()
            assert (w[:lead] == SENTINEL).all() and (w[-64:] == SENTINEL).all(), f"{k}: bytes around the slab were written"
        truncs = 0
        for s in range(K):
            twin.step_begin(acts[s], order[s])
            mid = spec.begin(p, st, acts[s], order[s], oracle=oracle)[0]
            _assert_state(twin, mid, f"E={E} twin after begin {s}")
            r, t, u = (v.cpu().numpy() for v in twin.run_array_strategies())
            twin.step_finish(torch.from_numpy(r), torch.from_numpy(t), torch.from_numpy(u))
            f = spec.finish(p, mid, r, t, u)
            tag = f"E={E} step {s} (byte offset {s * E * n} = {(s * E * n) % 4} mod 4)"
            np.testing.assert_array_equal(host["reward"][s].view(np.uint64), f.reward_bits, err_msg=tag)
            np.testing.assert_array_equal(host["agent_flags"][s], f.agent_flags, err_msg=tag)
            np.testing.assert_array_equal(host["env_flags"][s], f.env_flags, err_msg=tag)
            np.testing.assert_array_equal(host["term_present"][s], f.term_present, err_msg=tag)
            np.testing.assert_array_equal(host["obs_compact"][s].view(np.uint32), f.obs_compact.view(np.uint32), err_msg=tag)
            np.testing.assert_array_equal(host["obs"][s].view(np.uint32), spec.observe(oracle, p, mid).view(np.uint32), err_msg=tag)
            truncs += int((f.agent_flags & 2).astype(bool).sum())
            st = f.state
        _assert_state(roll, st, f"E={E} after the rollout")
        assert truncs > 0, "the step budget ran out inside the rollout"
        roll.close()
        twin.close()
    finally:
        undo()


# ---------------------------------------------------------------------------------------------------------------------
# auto-reset: pool sizes, shards, large episode indices
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,grid,E", [(8, (12, 8), 70), (5, (40, 30), 33)])
def test_auto_reset_pool_sizes_and_shards(ccx, oracle, n, grid, E):
    from collectivecrossing_amd.params import lower_config
    p = lower_config(cases.make_config(*grid, n))
    total = 2 * E + 6
    for j, P in enumerate([1, 3, E, E + 1, total // 2, total - 1 if total % (total - 1) else total - 2]):
        rng = np.random.default_rng(600 + j)
        pool = cases.make_pool(rng, p, P, n)
        st = cases.random_state(rng, p, total, n)
        st["episode"] = rng.integers(P, 2**31 - 8, size=total).astype(np.int32)
        st["episode"][::5] = 2**31 - 8        # (four resets from here stay inside int32)
        whole = _run_case(ccx, oracle, n, grid, total, seed=40 + j, auto_reset=True, pool=pool, state=st, steps=4)
        assert whole[1]["episodes"] > 0, f"pool size {P}: the batch must reset"
        # two shards of the same global batch on the slices of the SAME per-step inputs: each equals the spec (inside
        # _run_case), and together they equal the unsharded batch, state and counters
        cut = lambda sl: [tuple(None if v is None else np.ascontiguousarray(v[sl]) for v in step) for step in whole[3]]  # noqa: E731
        lo = {k: v[:E] for k, v in st.items()}
        hi = {k: v[E:] for k, v in st.items()}
        a = _run_case(ccx, oracle, n, grid, E, seed=40 + j, auto_reset=True, pool=pool, state=lo, steps=4, env_offset=0, total_envs=total,
                      inputs=cut(slice(0, E)))
        b = _run_case(ccx, oracle, n, grid, total - E, seed=40 + j, auto_reset=True, pool=pool, state=hi, steps=4, env_offset=E,
                      total_envs=total, inputs=cut(slice(E, total)))
        assert a[1]["episodes"] > 0 and b[1]["episodes"] > 0
        for k in spec.STATE_KEYS:
            np.testing.assert_array_equal(np.concatenate([a[2][k], b[2][k]]), whole[2][k], err_msg=f"pool size {P}: shards vs whole, {k}")
        assert {k: a[1][k] + b[1][k] for k in COUNTERS} == whole[1]


def test_auto_reset_with_built_in_rules_equals_a_one_step_rollout(ccx, oracle):
    n, grid, E, P = 8, (12, 8), 150, 7
    cfg = cases.make_config(*grid, n, max_steps=3)
    from collectivecrossing_amd.params import lower_config
    p = lower_config(cfg)
    rng = np.random.default_rng(21)
    pool = cases.make_pool(rng, p, P, n)
    split, twin = ccx(cfg, E, env_offset=11, total_envs=400), ccx(cfg, E, env_offset=11, total_envs=400)
    st = cases.random_state(rng, p, E, n, flags=False)
    for b in (split, twin):
        b.set_state(**st)
        b.set_reset_pool(pool)
    resets = 0
    for s in range(8):
        acts = cases.random_actions(rng, E, n)
        split.step_begin(acts)
        r = split.step_finish(auto_reset=True)
        t = twin.rollout(acts[None], auto_reset=True)
        for what in ("obs", "reward", "agent_flags", "env_flags"):
            np.testing.assert_array_equal(getattr(r, what).cpu().numpy().view(np.uint8), getattr(t, what)[0].cpu().numpy().view(np.uint8),
                                          err_msg=f"{what} step {s}")
        mid = spec.begin(p, st, acts, None, oracle=oracle)[0]
        f = spec.finish(p, mid, *spec.builtin_arrays(oracle, p, mid), auto_reset=True, pool=pool, env_offset=11, total_envs=400)
        st = f.state
        _assert_state(split, st, f"split step {s}")
        _assert_state(twin, st, f"rollout twin step {s}")
        resets += f.counters["episodes"]
    assert resets > E
    split.close()
    twin.close()


# ---------------------------------------------------------------------------------------------------------------------
# begin: dense crowds, the ccx_step twin, malformed input
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", cases.AGENT_COUNTS)
def test_begin_dense_crowds_equal_the_spec_and_ccx_step(ccx, oracle, n):
    import torch

    from collectivecrossing_amd.params import lower_config
    cfg = cases.make_config(12, 8, n, max_steps=50)
    p = lower_config(cfg)
    E = cases.QUEUE_ENVS
    st, acts, order = cases.queue_case(p, n, np.random.default_rng(2000 + n), E=E)
    rng = np.random.default_rng(n)
    st["terminated"] = (rng.random((E, n)) < 0.2).astype(np.uint8)
    st["truncated"] = (rng.random((E, n)) < 0.2).astype(np.uint8)
    st["episode"] = rng.integers(0, 1000, size=E).astype(np.int32)
    for use_order in (order, None):
        split, twin = ccx(cfg, E), ccx(cfg, E)
        res = split.step_finish(want_compact=True)          # (allocates the handle's own step buffers; the state is set below)
        bufs = [v for v in (res.obs, res.reward, res.agent_flags, res.env_flags, res.obs_compact, res.term_present)]
        for v in bufs:
            v.view(-1).view(torch.uint8).fill_(SENTINEL)
        split.set_state(**st)
        twin.set_state(**st)
        split.zero_counters()
        cur = st
        for s in range(3):
            a = acts if s == 0 else cases.random_actions(rng, E, n, toward_door=True, p=p, st=cur)
            o = use_order if s == 0 or use_order is None else cases.random_orders(rng, E, n)
            split.step_begin(a, o)
            twin.step(a, o)
            cur, mv, ar = spec.begin(p, cur, a, o, oracle=oracle)
            _assert_state(split, cur, f"N={n} step {s}: begin left flags and episode alone, moved as the spec says")
            assert all(bool((v.view(-1).view(torch.uint8) == SENTINEL).all()) for v in bufs), f"N={n} step {s}: begin wrote an output"
            got = twin.get_state()
            for k in ("x", "y", "active", "step_count"):
                np.testing.assert_array_equal(got[k], cur[k], err_msg=f"ccx_step twin {k}, N={n} step {s}")
            c = split.counters()
            assert (c["moves"], c["arrivals"], c["env_steps"]) == (mv, ar, 0), (n, s, c)
            split.zero_counters()
            twin.set_state(**cur)                # (the twin's own flags moved on: put it back on the split handle's state)
        split.close()
        twin.close()


@pytest.mark.parametrize("n", [3, 8, 11, 17, 33, 64])
def test_malformed_move_orders_follow_the_documented_rule(ccx, oracle, n):
    """include/ccx.h, ccx_step_begin: an order byte >= N names no agent and moves nothing -- whatever its low bits are: for
    8 agents the byte 9 used to move slot 1 --, a slot named twice moves at most once; the other envs of the wave are not
    affected and the launch completes."""
    from collectivecrossing_amd.params import lower_config
    cfg = cases.make_config(12, 8, n, max_steps=50)
    p = lower_config(cfg)
    E = cases.QUEUE_ENVS
    st, acts, order = cases.queue_case(p, n, np.random.default_rng(2000 + n), E=E)
    G = cases.lane_group(n)
    m = min(n - 1, p.width - 1)
    bad = order.copy()
    bad[0, 0] = G + (m - 1)                                       # >= G (at most 74), low bits name the head of the queue
    bad[1, 1] = bad[1, 0]                                         # a slot twice
    if G > n:
        bad[2, 0] = n                                             # a lane of the group without an agent
    bad[7] = 255
    bad[9, ::2] = np.arange(200, 200 + len(bad[9, ::2]))
    batch = ccx(cfg, E)
    batch.set_state(**st)
    batch.step_begin(acts, bad)
    want, _, _ = spec.begin(p, st, acts, bad, oracle=oracle)
    assert not spec.well_formed_orders(bad, n)[[0, 1, 7, 9]].any() and spec.well_formed_orders(bad, n)[10:].all()
    assert want["x"][0, m - 1] == st["x"][0, m - 1], "the head of env 0 was not named"
    _assert_state(batch, want, f"N={n}")
    batch.close()


@pytest.mark.parametrize("kind", ["ok", "absent_only", "action5", "action254", "order_twice", "order_ge_n", "order_ge_group"])
def test_check_inputs_on_the_begin_path_raises_when_ccx_step_does(ccx, kind):
    from collectivecrossing_amd._lib import CcxInputError
    n, E = 8, 70
    cfg = cases.make_config(12, 8, n)
    rng = np.random.default_rng(9)
    acts = rng.integers(0, 5, size=(E, n)).astype(np.uint8)
    acts[3, 2] = 255
    order = cases.random_orders(rng, E, n)
    if kind == "absent_only":
        acts[...] = 255
    if kind == "action5":
        acts[40, 1] = 5
    if kind == "action254":
        acts[0, 7] = 254
    if kind == "order_twice":
        order[69, 0] = order[69, 1]
    if kind == "order_ge_n":                      # 8 agents: the group has no spare lane, 8 is already outside it
        order[5, 3] = 8
    if kind == "order_ge_group":
        order[64, 7] = 9 + 8 * 30
    outcomes = []
    for path in ("begin", "step"):
        b = ccx(cfg, E, check_inputs=True)
        (b.step_begin if path == "begin" else b.step)(acts, order)
        try:
            b.synchronize()
            outcomes.append(None)
        except CcxInputError as e:
            outcomes.append(type(e))
        b.synchronize()                                           # (reported once)
        b.close()
    assert outcomes[0] == outcomes[1] == (None if kind in ("ok", "absent_only") else CcxInputError)
