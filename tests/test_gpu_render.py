"""ccx_render / ccx_render_compact on the MI355X, bit for bit against the NumPy restatement of the frame spec
(tests/_render_spec.py), and CollectiveCrossingEnv.render() against the reference's recorded frames (tests/golden/render)."""

import json
from pathlib import Path

import numpy as np
import pytest

import _render_spec as spec

pytestmark = pytest.mark.gpu

GOLDEN = Path(__file__).resolve().parent / "golden" / "render"


def _cfg(**kw):
    from collectivecrossing_amd.configs import CollectiveCrossingConfig, MaxStepsTruncatedConfig
    kw.setdefault("truncated_config", MaxStepsTruncatedConfig(max_steps=kw.pop("max_steps", 20)))
    return CollectiveCrossingConfig(**kw)


def c2():
    return _cfg(width=12, height=8, division_y=4, tram_door_left=5, tram_door_right=7, tram_length=9,
                num_boarding_agents=5, num_exiting_agents=3, exiting_destination_area_y=0, boarding_destination_area_y=8)


def _batch(cfg, E, seed=1, steps=0, pool=64):
    import torch
    from collectivecrossing_amd.batched import BatchedCollectiveCrossing
    env = BatchedCollectiveCrossing(cfg, E, device="cuda:0")
    env.make_reset_pool(seed, pool)
    env.reset_from_pool()
    if steps:
        acts = np.random.default_rng(seed).integers(0, 5, size=(steps, E, env.num_agents), dtype=np.uint8)
        env.rollout(torch.from_numpy(acts).cuda(), auto_reset=True, want_traj=False)
    return env


def _want(env, cp, env_ids=None):
    st = env.get_state()
    return spec.render_state(spec.geometry(env.params), st["x"], st["y"], env.params.num_boarding, cp, env_ids)


def _check(got, want):
    got = got.cpu().numpy()
    assert got.shape == want.shape and got.dtype == np.uint8
    bad = np.argwhere((got != want).any(axis=-1))
    assert bad.size == 0, f"{len(bad)} pixels differ, first {bad[:5].tolist()}"


def test_c2_4096_envs_after_a_random_rollout_cp8():
    env = _batch(c2(), 4096, seed=3, steps=37)
    frames = env.render()
    assert tuple(frames.shape) == (4096, 64, 96, 3)
    _check(frames, _want(env, 8))
    env.close()


@pytest.mark.parametrize("cp", [1, 2, 3, 7, 16])
def test_cell_sizes(cp):
    env = _batch(c2(), 61, seed=cp, steps=9)
    _check(env.render(cell_px=cp), _want(env, cp))
    env.close()


def test_100x100_with_50_agents_cp4():
    cfg = _cfg(width=100, height=100, division_y=50, tram_door_left=20, tram_door_right=26, tram_length=60,
               num_boarding_agents=30, num_exiting_agents=20, exiting_destination_area_y=5,
               boarding_destination_area_y=90)
    env = _batch(cfg, 6, seed=5, steps=40)
    _check(env.render(cell_px=4), _want(env, 4))
    env.close()


@pytest.mark.parametrize("cp", [1, 3, 5])
def test_13x9_frames_that_are_not_16_byte_multiples(cp):
    cfg = _cfg(width=13, height=9, division_y=4, tram_door_left=4, tram_door_right=7, tram_length=9,
               num_boarding_agents=3, num_exiting_agents=2, exiting_destination_area_y=2, boarding_destination_area_y=9)
    env = _batch(cfg, 33, seed=cp, steps=12)
    assert (13 * 9 * cp * cp * 3) % 16
    _check(env.render(cell_px=cp), _want(env, cp))
    env.close()


def test_env_id_list_with_repeats_and_an_id_out_of_range():
    import torch
    env = _batch(c2(), 50, seed=8, steps=15)
    ids = [7, 3, 3, 49, 0, 50, 7, 12]
    _check(env.render(ids, cell_px=5), _want(env, 5, ids))
    dev_ids = torch.tensor(ids[::-1], dtype=torch.int64, device=env.device)
    _check(env.render(dev_ids, cell_px=5), _want(env, 5, ids[::-1]))
    assert np.array_equal(_want(env, 5, [50])[0], _want(env, 5, [-1])[0])
    env.close()


def test_render_compact_of_a_trajectory_equals_render_after_each_step():
    import torch
    cfg = c2()
    K, E = 6, 40
    a = _batch(cfg, E, seed=9)
    b = _batch(cfg, E, seed=9)
    acts = torch.from_numpy(np.random.default_rng(9).integers(0, 5, size=(K, E, 8), dtype=np.uint8)).cuda()
    traj = a.rollout(acts, want_obs=False, want_compact=True)
    video = a.render_compact(traj.obs_compact, cell_px=4)
    assert tuple(video.shape) == (K, E, 32, 48, 3)
    for s in range(K):
        b.step(acts[s], want_obs=False)
        assert torch.equal(video[s], b.render(cell_px=4)), f"step {s}"
    _check(video.reshape(K * E, 32, 48, 3), spec.render_compact(spec.geometry(a.params),
                                                                traj.obs_compact.cpu().numpy(), 4).reshape(K * E, 32, 48, 3))
    a.close()
    b.close()


def test_step_and_render_capture_into_a_graph():
    import torch
    cfg = c2()
    E, K = 64, 5
    acts = torch.from_numpy(np.random.default_rng(2).integers(0, 5, size=(K, E, 8), dtype=np.uint8)).cuda()
    eager = _batch(cfg, E, seed=2)
    want = []
    for s in range(K):
        eager.step(acts[s], want_obs=False)
        want.append(eager.render(cell_px=6).clone())
    env = _batch(cfg, E, seed=2)
    side = torch.cuda.Stream(device=env.device)
    env.use_stream(side)
    a_in = torch.empty((E, 8), dtype=torch.uint8, device=env.device)
    frames = torch.empty((E, 48, 72, 3), dtype=torch.uint8, device=env.device)
    with torch.cuda.stream(side):
        a_in.copy_(acts[0])
        env.step(a_in, want_obs=False)             # warm-up outside the capture (allocates the step buffers)
        env.render(cell_px=6, out=frames)
        side.synchronize()
        env.reset_from_pool()
        side.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            env.step(a_in, want_obs=False)
            env.render(cell_px=6, out=frames)
        for s in range(K):
            a_in.copy_(acts[s])
            graph.replay()
            side.synchronize()
            assert torch.equal(frames, want[s]), f"step {s}"
    env.close()
    eager.close()


def test_host_side_checks_raise_before_a_launch():
    import torch
    env = _batch(c2(), 4)
    for cp in (0, 65, 2.0, True):
        with pytest.raises(ValueError):
            env.render(cell_px=cp)
    with pytest.raises(ValueError):
        env.render(out=torch.empty((4, 64, 96, 3), dtype=torch.float32, device=env.device))
    with pytest.raises(ValueError):
        env.render(out=torch.empty((4, 64, 96, 3), dtype=torch.uint8))
    with pytest.raises(ValueError):
        env.render(out=torch.empty((3, 64, 96, 3), dtype=torch.uint8, device=env.device))
    with pytest.raises(ValueError):
        env.render(env_ids=[[0, 1]])
    with pytest.raises(ValueError):
        env.render(env_ids=np.array([0.5]))
    with pytest.raises(ValueError):
        env.render_compact(torch.zeros((2, 7, 4), device=env.device))
    env.close()


def test_vector_env_render_delegates():
    from collectivecrossing_amd.vector import VectorCollectiveCrossing
    vec = VectorCollectiveCrossing(c2(), 5)
    vec.reset(np.arange(5))
    _check(vec.render([4, 0], cell_px=3), _want(vec.batch, 3, [4, 0]))
    vec.close()


@pytest.mark.parametrize("path", sorted(p for p in GOLDEN.glob("*.npz") if not bool(np.load(p)["relaxed"])),
                         ids=lambda p: p.stem)
def test_env_render_matches_the_batch_and_the_reference(path):
    from collectivecrossing_amd import CollectiveCrossingEnv
    from test_render_spec import load_fixture, sample_points

    g, z = load_fixture(path)
    env = CollectiveCrossingEnv(config=_cfg(**json.loads(str(z["config_json"]))))
    obs, _ = env.reset(seed=int(z["seed"]))
    for i, aid in enumerate(env.possible_agents):
        env._agents[aid].update_position(np.array([int(z["x"][i]), int(z["y"][i])]))
    frame = env.render()
    assert frame.shape == (800, 1200, 3) and frame.dtype == np.uint8
    cp = env.render_cell_px()
    top, left = env.render_board_origin()
    H, W = g["height"], g["width"]
    board = frame[top:top + H * cp, left:left + W * cp]
    assert np.array_equal(board, env._batch.render(cell_px=cp).cpu().numpy()[0])
    assert (frame[:top] == 255).all() and (frame[:, :left] == 255).all()
    assert np.array_equal(board, spec.render_frame(g, z["x"], z["y"], z["types"], cp))
    pts = sample_points(g, z, cp)
    got = np.array([board[r, c] for r, c, _ in pts], np.int64)
    want = np.array([w for _, _, w in pts], np.int64)
    assert (np.abs(got - want) <= 2).all()
    assert env.render(mode="human") is None
    with pytest.raises(NotImplementedError):
        env.render(mode="ansi")
    env.close()
