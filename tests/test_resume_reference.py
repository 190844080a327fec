"""The composed CPU references of tests/_rainbow_chain.py stopped and resumed (``stop_after=`` / ``resume=``): what
tests/test_gpu_resume.py holds a run to that was checkpointed, closed and continued on a new handle.  Three things, all on bit
patterns: a split run IS the unsplit run (every link of every later round and the final state); at the resume points the
state is one in which a lost component would show (conditions, not measurements); and every component of the checkpoint
matters -- resumed with ONE of them left as a freshly constructed object holds it (OMISSIONS / PPO_OMISSIONS), the run
differs from the unsplit one in a later link and in the final parameters, so a device run that lost that component could
not pass the comparison.  Each (resume point, omission) pair prints the first link that differs.

Resume points: Rainbow before round 6 (ring wrapped, hand-set ``truncated`` flags still up, the event and a target copy
ahead) and before round 8 (just behind ``reset_from_pool()`` + ``mark_cut()``); the PPO minibatch iteration before update
5 of 8 (second epoch, mid-epoch, behind the rate change, ahead of the partly EMPTY tail).  ``truncated`` is all zero before
round 8, so leaving it out there restores the same bytes: that omission is asserted before round 6 only."""

import numpy as np
import pytest
from _learner_chain import H, N, PPO, PPO_INIT_SEEDS
from _mlp_spec import linear_init
from _prio_spec import ONE_FIXED
from _rainbow_chain import (LINKS, OMISSIONS, PPO_MB, PPO_MB_KEYS, PPO_OMISSIONS, RAINBOW, RAINBOW_INIT_SEEDS, first_difference,
                            ppo_minibatch_reference, rainbow_reference)

L = 6 + 4 * N
RESUME_ROUNDS = (6, 8)
PPO_RESUME_STEP = 5
RAINBOW_FINAL = ("params", "target", "m", "v", "state_bytes", "ring_state", "leaf", "pstate", "cut")
PPO_FINAL = ("params", "m", "v", "state_bytes", "mb_state")
PPO_LINKS = ("index",) + tuple(f"mb.{k}" for k in PPO_MB_KEYS) + ("stats", "grads", "adam_stats")
INERT = {(8, "truncated")}                       # no flag is set before round 8: the omission restores the same bytes


def rainbow_init():
    return [linear_init(L, H, RAINBOW["O"], seed=s) for s in RAINBOW_INIT_SEEDS]


def ppo_init():
    return linear_init(L, H, 5, seed=PPO_INIT_SEEDS[0]), linear_init(L, H, 1, seed=PPO_INIT_SEEDS[1])


def as_bytes(a) -> bytes:
    if isinstance(a, (list, tuple)):
        return b"".join(as_bytes(x) for x in a)
    return np.ascontiguousarray(a).tobytes()


def ppo_link(r, i, k):
    return r["mb"][i][k[3:]] if k.startswith("mb.") else r[k][i]


def first_ppo_difference(a, b):
    for i in range(len(a["index"])):
        for k in PPO_LINKS:
            if as_bytes(ppo_link(a, i, k)) != as_bytes(ppo_link(b, i, k)):
                return f"update {i}: {k}"
    return None


@pytest.fixture(scope="module")
def rainbow(oracle):
    return rainbow_reference(rainbow_init())


@pytest.fixture(scope="module")
def stopped(oracle):
    return {k: rainbow_reference(rainbow_init(), stop_after=k) for k in RESUME_ROUNDS}


@pytest.fixture(scope="module")
def ppo_mb(oracle):
    return ppo_minibatch_reference(*ppo_init(), "rows")


@pytest.fixture(scope="module")
def ppo_stopped(oracle):
    return ppo_minibatch_reference(*ppo_init(), "rows", stop_after=PPO_RESUME_STEP)


# ------------------------------------------------------------------------------------------------------------ split == unsplit
@pytest.mark.parametrize("k", RESUME_ROUNDS)
def test_a_split_rainbow_run_is_the_unsplit_run(rainbow, stopped, k):
    part = stopped[k]
    assert len(part["rounds"]) == k and part["facts"] is None and part["snapshot"]["round"] == k
    assert first_difference(rainbow, part) is None                       # (zip: the k rounds the stopped run has)
    whole = rainbow_reference(None, resume=(part["snapshot"], None))
    assert len(whole["rounds"]) == RAINBOW["ROUNDS"] and first_difference(rainbow, whole) is None
    for u in range(RAINBOW["ROUNDS"]):
        for link in LINKS:
            assert as_bytes(whole["rounds"][u][link]) == as_bytes(rainbow["rounds"][u][link]), f"round {u}: {link}"
    for key in RAINBOW_FINAL + ("actions", "explored", "reward", "agent_flags", "env_flags", "epsilon", "beta"):
        assert as_bytes(whole[key]) == as_bytes(rainbow[key]), key
    assert whole["facts"] == rainbow["facts"]


def test_a_split_ppo_minibatch_iteration_is_the_unsplit_one(ppo_mb, ppo_stopped):
    assert len(ppo_stopped["index"]) == PPO_RESUME_STEP and ppo_stopped["facts"] is None
    for form, unsplit in (("rows", ppo_mb), ("compact", ppo_minibatch_reference(*ppo_init(), "compact"))):
        part = ppo_stopped if form == "rows" else ppo_minibatch_reference(*ppo_init(), form, stop_after=PPO_RESUME_STEP)
        whole = ppo_minibatch_reference(None, None, form, resume=(part["snapshot"], None))
        assert len(whole["index"]) == 8 and first_ppo_difference(unsplit, whole) is None, form
        for key in PPO_FINAL + ("norm", "advantages"):
            assert as_bytes(whole[key]) == as_bytes(unsplit[key]), (form, key)
        assert whole["facts"] == unsplit["facts"]


# ------------------------------------------------------------------------------------------------------------ coverage
def drawn_from_before(ref, k):
    """Per round u >= k: how many of its drawn records were pushed before the checkpoint (their ring step has not been
    overwritten by the u - k + 1 pushes since)."""
    R = RAINBOW
    S, E, head_k = R["RING_STEPS"], R["E"], R["WARMUP"] + k
    out = []
    for u in range(k, R["ROUNDS"]):
        new_steps = {(head_k + j) % S for j in range(u - k + 1)}
        out.append(int(sum(int(i) // E not in new_steps for i in ref["rounds"][u]["index"] if i >= 0)))
    return out


def test_the_state_before_round_6_is_one_a_lossy_checkpoint_would_show_in(rainbow, stopped):
    R, snap, f = RAINBOW, stopped[6]["snapshot"], rainbow["facts"]
    env = snap["env"]
    assert int(snap["ring"]["state"][0]) == 8 > R["RING_STEPS"] == 6                 # the ring has wrapped
    assert int(env["truncated"].sum()) == 4                              # hand-set flags of round 3 still up
    assert set(env["episode"].tolist()) == {0, 1}
    assert env["step_count"].tolist() == [8, 11, 2, 5, 8, 11, 2, 5]
    assert int(np.count_nonzero(snap["cut"])) == 4
    assert int(snap["pstate"][0]) == 198857 > ONE_FIXED                  # max_leaf
    assert int(snap["pstate"][1]) == 6                                   # the draw counter
    assert as_bytes(snap["target"]) != as_bytes(snap["online"])          # copied behind round 4, one update since
    assert f["copies"][4] and not any(f["copies"][:4]) and not f["copies"][5]
    assert snap["adam"]["step"] == 6 and any(s < 1.0 for s in f["adam_scales"][:6])
    assert any(np.any(m) for m in snap["m"]) and any(np.any(v) for v in snap["v"])
    assert R["EVENT_ROUND"] == 7 > 6 and f["copies"][9]                  # the event and a target copy lie behind the resume
    before = drawn_from_before(rainbow, 6)
    print(f"rounds 6..11 draw records pushed before the checkpoint: {before} of {R['BATCH']}")
    assert before == [29, 24, 17, 12, 5, 0]
    later = rainbow["rounds"][6:]
    assert sorted({int(s) for x in later for s in np.unique(x["mb.span"])}) == [1, 2, 3]
    assert [u for u in f["rounds_with_a_duplicate_index"] if u >= 6]
    assert sum(f["drawn_records_that_end_an_episode"][6:]) > 0
    assert f["rows_dropped_that_were_live"][6:8] == [9, 5]               # the ring's own ``valid`` bytes from before matter


def test_the_state_before_round_8_is_just_behind_the_event(rainbow, stopped):
    snap, f = stopped[8]["snapshot"], rainbow["facts"]
    assert int(np.count_nonzero(snap["cut"])) == 10                      # reset_from_pool() + mark_cut() before round 7
    print(f"windows shortened by the event, per round: {f['windows_shortened_by_the_event']}")
    assert f["windows_shortened_by_the_event"][8:] == [8, 8, 10, 5] and sum(f["windows_shortened_by_the_event"][8:]) > 0
    assert not snap["env"]["truncated"].any()                            # why ``truncated`` is inert here (INERT)
    assert snap["adam"]["step"] == 8 and int(snap["pstate"][1]) == 8 and f["copies"][9]


def test_the_state_before_ppo_update_5(ppo_mb, ppo_stopped):
    snap, f = ppo_stopped["snapshot"], ppo_mb["facts"]
    assert snap["mb_state"].tolist() == [1, PPO_MB["B"], 0, 0] == [1, 80, 0, 0]      # the second epoch, mid-epoch
    assert PPO["LR_CHANGE_AFTER"] == 4 < PPO_RESUME_STEP and f["adam_lrs"][3] != f["adam_lrs"][4] == f["adam_lrs"][5]
    assert snap["adam"]["step"] == 5
    assert f["empty_rows_run"][7] > 0 and f["real_records"][7] < PPO_MB["B"]         # the partly EMPTY tail lies behind it


# ------------------------------------------------------------------------------------------------------------ sensitivity
@pytest.mark.parametrize("omit", OMISSIONS)
@pytest.mark.parametrize("k", RESUME_ROUNDS)
def test_every_component_of_the_rainbow_checkpoint_matters(rainbow, stopped, k, omit):
    wrong = rainbow_reference(None, resume=(stopped[k]["snapshot"], omit))
    first = first_difference(rainbow, wrong)
    print(f"rainbow resumed before round {k} without {omit}: first link that differs: {first}")
    if (k, omit) in INERT:
        assert not stopped[k]["snapshot"]["env"][omit].any() and first is None       # the same bytes: nothing to lose here
        return
    assert first is not None and int(first.split(":")[0].split()[1]) >= k, (k, omit, first)
    assert as_bytes(rainbow["params"]) != as_bytes(wrong["params"]), (k, omit)


@pytest.mark.parametrize("omit", PPO_OMISSIONS)
def test_every_component_of_the_ppo_checkpoint_matters(ppo_mb, ppo_stopped, omit):
    wrong = ppo_minibatch_reference(None, None, "rows", resume=(ppo_stopped["snapshot"], omit))
    first = first_ppo_difference(ppo_mb, wrong)
    print(f"ppo minibatches resumed before update {PPO_RESUME_STEP} without {omit}: first link that differs: {first}")
    assert first is not None and int(first.split(":")[0].split()[1]) >= PPO_RESUME_STEP, (omit, first)
    assert as_bytes(ppo_mb["params"]) != as_bytes(wrong["params"]), omit
