"""bench.py --dump-outputs on CPU tensors: what it writes (float32 / float64 .npy), the size limit, and the seeded
sample of envs / steps it falls back to above the limit -- the same sample every call."""

import sys
from pathlib import Path

import numpy as np
import pytest
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
import bench  # noqa: E402

from collectivecrossing_amd.batched import RolloutResult  # noqa: E402


class _Env:
    device = torch.device("cpu")

    def synchronize(self):
        pass


def _outputs(K, E, N, seed=0):
    g = torch.Generator().manual_seed(seed)
    L = 6 + 4 * N
    return RolloutResult(torch.randint(0, 30, (K, E, N, L), generator=g).float(),
                         torch.randn((K, E, N), generator=g, dtype=torch.float64),
                         torch.randint(0, 256, (K, E, N), generator=g).to(torch.uint8),
                         torch.randint(0, 8, (K, E), generator=g).to(torch.uint8))


def _load(d):
    return {p.stem: np.load(p) for p in sorted(Path(d).glob("*.npy"))}


def test_small_outputs_are_written_whole(tmp_path):
    out = _outputs(5, 7, 3)
    info = bench.dump_outputs(torch, _Env(), out, str(tmp_path))
    a = _load(tmp_path)
    assert sorted(a) == ["agent_flags", "env_flags", "obs", "reward"] and info["envs"] == "7 of 7"
    assert a["obs"].dtype == np.float32 and a["reward"].dtype == np.float64
    assert a["agent_flags"].dtype == np.float32 and a["env_flags"].dtype == np.float32
    np.testing.assert_array_equal(a["obs"], out.obs.numpy())
    np.testing.assert_array_equal(a["reward"].view(np.uint64), out.reward.numpy().view(np.uint64))
    np.testing.assert_array_equal(a["agent_flags"], out.agent_flags.numpy())
    np.testing.assert_array_equal(a["env_flags"], out.env_flags.numpy())


@pytest.mark.parametrize("limit", [40_000, 3_000], ids=["envs", "envs_and_steps"])
def test_large_outputs_become_the_same_seeded_sample_every_time(tmp_path, monkeypatch, limit):
    monkeypatch.setattr(bench, "DUMP_BYTES", limit)
    K, E, N = 12, 50, 4
    out = _outputs(K, E, N)
    bench.dump_outputs(torch, _Env(), out, str(tmp_path / "a"))
    bench.dump_outputs(torch, _Env(), _outputs(K, E, N), str(tmp_path / "b"))
    a, b = _load(tmp_path / "a"), _load(tmp_path / "b")
    assert sum(x.nbytes for x in a.values()) <= limit
    for k in a:
        np.testing.assert_array_equal(a[k].view(np.uint8), b[k].view(np.uint8), err_msg=k)
    per_env = K * N * (4 * (6 + 4 * N) + 8 + 4) + K * 4
    steps, envs = bench.dump_sample(K, E, per_env)
    assert 1 <= len(envs) < E and (len(steps) == K) == (limit == 40_000)
    for idx in (steps, envs):
        assert np.all(np.diff(idx) > 0) and idx[0] >= 0
    assert steps[-1] < K and envs[-1] < E
    for k in a:
        want = getattr(out, k).numpy()[steps][:, envs]
        np.testing.assert_array_equal(a[k], want.astype(a[k].dtype), err_msg=k)
