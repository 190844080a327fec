"""CCX_EPISODE_STATS on the CPU: the NumPy spec (tests/_episode_stats_spec.py) against hand-written cases and against a
literal Python-float loop over the committed goldens, the ctypes mirror of the new struct against the header, and the
register budget of the new kernels.  No GPU needed."""

import ctypes
import subprocess

import numpy as np
import pytest
from _episode_stats_spec import (AF_LIVE, EF_ALL_TERMINATED, EF_ALL_TRUNCATED, EF_RESET, StatsSpec, bits, make_trajectory,
                                 sort_log)
from _fixtures import Golden
from test_kernel_resources import ROOT, _kernels

T, U, R = EF_ALL_TERMINATED, EF_ALL_TRUNCATED, EF_RESET
# records the fixtures hold (counted once on the fixtures; asserted so that nothing below passes vacuously), and the
# (step, env) pairs on which an __all__ flag is raised
RECORDS = {"g8_rollout_c1": (36, 36), "g8_rollout_small_all_at_dest": (40, 40), "g9_c1_waiting_policy": (8, 648),
           "g7_n1_exiting_only": (4, 56)}


def _one_env(rewards, live, ef, capacity=8):
    """A 1-env spec fed one update: rewards / live [K][N], ef [K]."""
    rewards = np.asarray(rewards, np.float64)
    K, N = rewards.shape
    spec = StatsSpec(1, N, capacity)
    af = np.where(np.asarray(live, bool), AF_LIVE, 0).astype(np.uint8)
    spec.update(rewards.reshape(K, 1, N), af.reshape(K, 1, N), np.asarray(ef, np.uint8).reshape(K, 1))
    return spec


def test_running_sum_is_left_to_right():
    spec = _one_env([[1e16], [1.0], [-1e16]], [[1], [1], [1]], [0, 0, 0])
    assert spec.ret[0, 0] == 0.0                  # (1e16 + 1.0) - 1e16: the 1.0 is absorbed; any other order gives 1.0
    assert spec.steps[0] == 3 and spec.live_steps[0, 0] == 3 and spec.finished[0] == 0 and not spec.records


def test_not_live_rewards_are_not_read_and_do_not_count():
    spec = _one_env([[1.0, np.nan], [2.0, 5.0], [np.nan, np.nan]], [[1, 0], [1, 1], [0, 0]], [0, 0, 0])
    assert spec.ret.tolist() == [[3.0, 5.0]] and spec.live_steps.tolist() == [[2, 1]] and spec.steps[0] == 3


def test_negative_zero_start():
    spec = _one_env([[-0.0]], [[1]], [0])
    assert bits(spec.ret)[0, 0] == 0              # +0.0 + -0.0 = +0.0, as Python's `total = 0.0; total += -0.0`


def test_finish_record_and_reset():
    spec = _one_env([[1.0], [2.0], [4.0], [8.0]], [[1]] * 4, [0, T | R, 0, U])
    log = spec.log()
    assert log["env"].tolist() == [0, 0] and log["episode"].tolist() == [0, 1]
    assert log["steps"].tolist() == [2, 2] and log["end"].tolist() == [T, U]
    assert log["ret"].tolist() == [[3.0], [12.0]] and log["live_steps"].tolist() == [[2], [2]]
    assert spec.finished[0] == 2 and spec.closed[0] == 1 and spec.steps[0] == 2 and spec.ret[0, 0] == 12.0
    assert spec.last_ret[0, 0] == 12.0 and spec.last_steps[0] == 2 and spec.last_end[0] == U


def test_latch_without_reset_then_reset_alone():
    # raised on steps 1..3 without RESET: ONE record; steps behind it do not count; RESET alone reopens without a record
    spec = _one_env([[1.0], [2.0], [4.0], [8.0], [16.0], [32.0]], [[1]] * 6, [0, T, T, T | U, R, 0])
    log = spec.log()
    assert log["steps"].tolist() == [2] and log["ret"].tolist() == [[3.0]] and log["end"].tolist() == [T]
    assert spec.finished[0] == 1 and spec.closed[0] == 0
    assert spec.steps[0] == 1 and spec.ret[0, 0] == 32.0           # step 4 fell into the closed episode, step 5 opened anew
    assert spec.last_ret[0, 0] == 3.0


def test_last_is_zero_before_the_first_finish_and_reset_keeps_it():
    spec = _one_env([[1.0]], [[1]], [0])
    assert not spec.last_ret.any() and not spec.last_steps.any() and not spec.last_end.any()
    spec.update(np.full((1, 1, 1), 2.0), np.full((1, 1, 1), AF_LIVE, np.uint8), np.full((1, 1), T, np.uint8))
    spec.reset()
    assert spec.ret[0, 0] == 0.0 and spec.steps[0] == 0 and spec.closed[0] == 0 and spec.live_steps[0, 0] == 0
    assert spec.finished[0] == 1 and spec.last_ret[0, 0] == 3.0 and spec.last_steps[0] == 2 and len(spec.records) == 1


def test_masked_reset():
    r, af, ef = make_trajectory(9, 5, 2, seed=3)
    spec = StatsSpec(5, 2)
    spec.update(r, af, np.zeros_like(ef))
    before = spec.ret.copy()
    spec.reset([0, 1, 0, 1, 0])
    assert not spec.ret[[1, 3]].any() and not spec.steps[[1, 3]].any()
    assert (bits(spec.ret[[0, 2, 4]]) == bits(before[[0, 2, 4]])).all() and (spec.steps[[0, 2, 4]] == 9).all()


def test_log_order_is_env_major_and_overflow_is_counted():
    # env 0 finishes at steps 3 and 5, env 1 at step 0: one update orders them (0, s3), (0, s5), (1, s0)
    ef = np.zeros((6, 2), np.uint8)
    ef[3, 0] = ef[5, 0] = ef[0, 1] = T | R
    ones = np.ones((6, 2, 1))
    spec = StatsSpec(2, 1, log_capacity=2, env_offset=100)
    spec.update(ones, np.full((6, 2, 1), AF_LIVE, np.uint8), ef)
    log = spec.log()
    assert log["env"].tolist() == [100, 100] and log["steps"].tolist() == [4, 2] and spec.dropped == 1 and spec.emitted == 3
    spec.clear_log()
    spec.update(ones, np.full((6, 2, 1), AF_LIVE, np.uint8), ef)
    assert spec.log()["episode"].tolist() == [2, 3] and spec.dropped == 1


def test_cut_invariance_of_the_spec():
    r, af, ef = make_trajectory(37, 15, 3, seed=5)
    whole = StatsSpec(15, 3, 10_000)
    whole.update(r, af, ef)
    cut = StatsSpec(15, 3, 10_000)
    for a, b in ((0, 1), (1, 17), (17, 18), (18, 37)):
        cut.update(r[a:b], af[a:b], ef[a:b])
    for k, v in whole.accumulators().items():
        assert (bits(v) == bits(cut.accumulators()[k])).all(), k
    lw, lc = sort_log(whole.log()), sort_log(cut.log())
    assert len(lw["env"]) == whole.emitted > 15
    for k in lw:
        assert (bits(lw[k]) == bits(lc[k])).all(), k


def _literal_loop(g: Golden):
    """What a user of the reference writes (examples/waiting_policy_demo.py:52-85): `total[a] += float(r)` per live agent,
    the episode cut at the first raised `__all__`; a new episode only after the env was restarted."""
    rew, af, ef = g["reward"], g["agent_flags"], g["env_flags"]
    out = []
    for e in range(g.E):
        tot, n, steps, done = [0.0] * g.N, [0] * g.N, 0, False
        for s in range(g.K):
            if not done:
                steps += 1
                for a in range(g.N):
                    if af[s, e, a] & AF_LIVE:
                        tot[a] += float(rew[s, e, a])
                        n[a] += 1
                if ef[s, e] & 3:
                    out.append((e, steps, int(ef[s, e] & 3), list(tot), list(n)))
                    done = True
            if ef[s, e] & EF_RESET:
                tot, n, steps, done = [0.0] * g.N, [0] * g.N, 0, False
    return out


@pytest.mark.parametrize("name", sorted(RECORDS))
def test_spec_equals_the_literal_loop_on_the_goldens(name):
    g = Golden(name)
    records, raised = RECORDS[name]
    assert int(((g["env_flags"] & 3) != 0).sum()) == raised
    spec = StatsSpec(g.E, g.N, log_capacity=1000)
    spec.update(g["reward"], g["agent_flags"], g["env_flags"])
    lit = _literal_loop(g)
    log = spec.log()
    assert len(lit) == records == len(log["env"]) == spec.emitted and spec.dropped == 0
    assert log["env"].tolist() == [r[0] for r in lit] and log["steps"].tolist() == [r[1] for r in lit]
    assert log["end"].tolist() == [r[2] for r in lit]
    assert (bits(log["ret"]) == bits(np.array([r[3] for r in lit], np.float64))).all()
    assert (log["live_steps"] == np.array([r[4] for r in lit], np.int32)).all()
    assert int(spec.finished.sum()) == records


def test_struct_mirror_matches_the_header(tmp_path):
    from collectivecrossing_amd import _abi

    src = r'''
#include <stdio.h>
#include <stddef.h>
#include "ccx.h"
int main(void){ printf("%zu %zu %zu %zu\n", sizeof(ccx_episode_stats), offsetof(ccx_episode_stats, last_end),
                       offsetof(ccx_episode_stats, log_count), offsetof(ccx_episode_stats, log_capacity)); return 0; }'''
    (tmp_path / "t.c").write_text(src)
    subprocess.run(["gcc", "-I", str(ROOT / "include"), "-o", str(tmp_path / "t"), str(tmp_path / "t.c")], check=True)
    out = subprocess.run([str(tmp_path / "t")], check=True, capture_output=True, text=True).stdout.split()
    S = _abi.CcxEpisodeStats
    assert [int(v) for v in out] == [ctypes.sizeof(S), S.last_end.offset, S.log_count.offset, S.log_capacity.offset]


def test_episode_stats_kernels_have_no_scratch_and_no_spills(tmp_path):
    kernels = {n: v for n, v in _kernels(tmp_path).items() if "stats_" in n}
    # accumulate x {log, no log} x {pipelined, one load per step}, count, scan, reset
    assert len(kernels) == 7 and sum("stats_accumulate" in n for n in kernels) == 4, sorted(kernels)
    for name, (vgpr, scratch, sgpr_spill) in kernels.items():
        assert scratch == 0 and sgpr_spill == 0, (name, vgpr, scratch, sgpr_spill)
        assert vgpr <= 256, (name, vgpr)          # (two chunks of 16 steps in registers; two waves per SIMD are enough)
