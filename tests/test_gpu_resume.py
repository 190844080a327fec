"""Checkpoint and resume of the two whole loops of tests/_chain_device.py on a NEW handle, against the composed CPU
references of tests/_rainbow_chain.py, bit for bit.  A run is stopped behind round k - 1, its state is collected with the
public API only, written to a file with ``torch.save``, every object of the run is deleted and its batch closed; the file
is read back with ``torch.load(map_location="cpu")`` and a second batch on a new stream, with new heads, replay objects,
optimiser, static buffers and (captured mode) new graphs, runs the remaining rounds.  Every link of every later round and
the final state must be the unsplit reference's: tests/test_resume_reference.py shows on the CPU that a split reference run
is the unsplit one, that the state at the resume points is one in which a lost component shows, and that each component
left out changes a later link and the final parameters.

What is compared here and nowhere else: that ``get_state()`` + the four ``state_dict()`` + the episode-statistics arrays
are the WHOLE state of a run (nothing lives only in the old handle or in a Python wrapper: the ``episode`` counters that key
the reset-pool cursor and every action draw, hand-set ``truncated`` flags, the draw counters of ``ring.state`` and ``pstate``,
``max_leaf``, the sum tree derived from ``leaf``, the cut bytes of ``mark_cut()``, Adam's step powers, ``{epoch, cursor}`` of
``RolloutMinibatches``), that every ``load_state_dict`` takes the CPU tensors ``torch.load`` returns, and that the episode
statistics continue -- accumulators, ``finished`` ordinals and the concatenated log -- across the two handles.

One negative control on the device: resumed before round 6 with a fresh ``NStepReplay`` whose ring is restored but whose
``cut`` is not, the run must equal the CPU reference resumed with the ``cut`` omission, link for link -- so it differs from
the true reference where the CPU test says (``round 6: mb.next_obs``)."""

import gc

import numpy as np
import pytest
from _chain_device import (L, MinibatchUpdates, RainbowLoop, World, _np, check_ppo_final, check_rainbow_final, collect,
                           minibatch_source, values_and_advantages)
from _episode_stats_spec import ACC_KEYS, LOG_KEYS, StatsSpec, bits
from _learner_chain import H, N, PPO_INIT_SEEDS
from _mlp_spec import linear_init
from _rainbow_chain import (PPO_MB, RAINBOW, RAINBOW_INIT_SEEDS, first_difference, ppo_minibatch_reference,
                            rainbow_reference, same)

pytestmark = pytest.mark.gpu

LOG_CAPACITY = 64
PPO_RESUME_STEP = 5                              # tests/test_resume_reference.py: second epoch, mid-epoch, behind the rate change


@pytest.fixture(scope="module")
def rainbow_ref(oracle):
    """The unsplit reference from the committed ``linear_init`` parameters; run once."""
    init = [linear_init(L, H, RAINBOW["O"], seed=s) for s in RAINBOW_INIT_SEEDS]
    ref = rainbow_reference(init)
    ref["init"] = init
    return ref


@pytest.fixture(scope="module")
def stats_spec(rainbow_ref):
    """The episode statistics of the whole run from the reference's per-step arrays; ``reset()`` at the event, as
    ``reset_from_pool`` does on the device."""
    R = RAINBOW
    spec = StatsSpec(R["E"], N, log_capacity=LOG_CAPACITY)
    for s in range(R["WARMUP"] + R["ROUNDS"]):
        if s == R["WARMUP"] + R["EVENT_ROUND"]:
            spec.reset()
        spec.update(*(rainbow_ref[k][s][None] for k in ("reward", "agent_flags", "env_flags")))
    assert 0 < len(spec.records) < LOG_CAPACITY and spec.dropped == 0 and spec.finished.max() >= 1
    return spec


# ------------------------------------------------------------------------------------------------------------ save / load
def save_rainbow(loop, path) -> None:
    """Everything a run must save, public API only, into one file."""
    import torch

    env = loop.env
    loop.stream.synchronize()
    stats = env.episode_stats()
    log = env.finished_episodes(clear=True)
    torch.save(dict(env=env.get_state(), replay=loop.pr.state_dict(), adam=loop.opt.state_dict(), online=loop.online.state_dict(),
                    target=loop.target.state_dict(), stats={k: getattr(stats, k).clone() for k in ACC_KEYS},
                    log={k: getattr(log, k) for k in LOG_KEYS}, log_dropped=log.dropped), path)


def load_rainbow(loop, ckpt, restore_cut: bool = True) -> None:
    """Everything a run must redo on a new batch: the constructor of ``RainbowLoop`` has made the reset pool, the terminated
    table and the seed again; here the env state, every dict, the statistics, and the actor's inputs recomputed."""
    env = loop.env
    env.set_state(**ckpt["env"])
    if restore_cut:
        loop.pr.load_state_dict(ckpt["replay"])
    else:                                                                # the negative control: the ring, not ``cut``
        sd = ckpt["replay"]
        loop.ring.load_state_dict(sd["ring"]["ring"])
        loop.pr.leaf.copy_(sd["leaf"])
        loop.pr.pstate.copy_(sd["pstate"])
        loop.pr.beta = sd["beta"]
    loop.opt.load_state_dict(ckpt["adam"])
    loop.online.load_state_dict(ckpt["online"])
    loop.target.load_state_dict(ckpt["target"])
    stats = env.episode_stats()
    for k in ACC_KEYS:
        getattr(stats, k).copy_(ckpt["stats"][k])
    loop.refresh_actor_inputs()
    loop.stream.synchronize()


def resumed_rainbow(ref, k: int, captured: bool, tmp_path, want, restore_cut: bool = True):
    """Rounds 0 .. k - 1 on batch A, through a file, rounds k .. 11 on batch B checked against ``want``.  Returns B's final
    state, its accumulators, A's drained log followed by B's, and the two logs' lengths."""
    import torch

    path = tmp_path / "checkpoint.pt"
    a = RainbowLoop(track=LOG_CAPACITY)
    try:
        with a.scope():
            a.start(ref["init"])
            a.warm_up(ref)
            if captured:
                a.capture()
            a.run_rounds(ref, 0, k, check=True)
            save_rainbow(a, path)
    finally:
        a.close()
    del a
    gc.collect()
    torch.cuda.empty_cache()
    ckpt = torch.load(path, map_location="cpu", weights_only=False)
    assert all(not t.is_cuda for t in (ckpt["replay"]["leaf"], ckpt["replay"]["ring"]["cut"], ckpt["adam"]["state"], ckpt["stats"]["ret"]))
    b = RainbowLoop(track=LOG_CAPACITY)
    try:
        with b.scope():
            load_rainbow(b, ckpt, restore_cut)
            if captured:
                b.capture()
            b.run_rounds(want, k, RAINBOW["ROUNDS"], check=True)
            assert b.opt.counts() == (RAINBOW["ROUNDS"], 0)
            final = b.final()
            stats = b.env.episode_stats()
            acc = {key: _np(getattr(stats, key)) for key in ACC_KEYS}
            log_b = b.env.finished_episodes()
            assert ckpt["log_dropped"] == 0 and log_b.dropped == 0
            log = {key: np.concatenate([ckpt["log"][key], getattr(log_b, key)]) for key in LOG_KEYS}
            return final, acc, log, (len(ckpt["log"]["env"]), len(log_b))
    finally:
        b.close()


# ------------------------------------------------------------------------------------------------------------ Rainbow
@pytest.mark.parametrize("captured", (False, True), ids=("eager", "captured"))
@pytest.mark.parametrize("k", (6, 8))
def test_a_rainbow_run_resumed_on_a_new_handle_is_the_unsplit_run(rainbow_ref, stats_spec, tmp_path, k, captured):
    final, acc, log, parts = resumed_rainbow(rainbow_ref, k, captured, tmp_path, rainbow_ref)
    assert sum(parts) == len(stats_spec.records) and (k != 6 or min(parts) > 0)      # before round 6: records on either handle
    check_rainbow_final(final, rainbow_ref, f"resumed before round {k}")
    for key in ACC_KEYS:
        same(bits(acc[key]), bits(stats_spec.accumulators()[key]), f"episode statistics behind the last round: {key}")
    want = stats_spec.log()
    for key in LOG_KEYS:
        same(bits(log[key]), bits(want[key]), f"the first handle's drained log followed by the second's: {key}")


def test_a_rainbow_run_resumed_without_its_cut_bytes_is_the_references_omission(rainbow_ref, tmp_path):
    """The negative control: what the device does with a checkpoint that lost ``cut`` is what the CPU reference says, so the
    comparison of the test above would have named it."""
    k = 6
    stopped = rainbow_reference(rainbow_ref["init"], stop_after=k)
    wrong = rainbow_reference(None, resume=(stopped["snapshot"], "cut"))
    first = first_difference(rainbow_ref, wrong)
    print(f"resumed before round {k} without cut: the reference first differs at {first}")
    assert first == "round 6: mb.next_obs"
    final, _, _, _ = resumed_rainbow(rainbow_ref, k, True, tmp_path, wrong, restore_cut=False)
    check_rainbow_final(final, wrong, "resumed without cut")
    assert any(final["params"][i].tobytes() != rainbow_ref["params"][i].tobytes() for i in range(len(final["params"])))


# ------------------------------------------------------------------------------------------------------------ PPO minibatches
@pytest.fixture(scope="module")
def ppo_refs(oracle):
    init = [linear_init(L, H, 5, seed=PPO_INIT_SEEDS[0]), linear_init(L, H, 1, seed=PPO_INIT_SEEDS[1])]
    out = {form: ppo_minibatch_reference(*init, form) for form in ("rows", "compact")}
    for ref in out.values():
        ref["init"] = init
    return out


@pytest.mark.parametrize("form", ("rows", "compact"))
def test_a_ppo_minibatch_iteration_resumed_on_a_new_handle_is_the_unsplit_one(ppo_refs, tmp_path, form):
    """Updates 0 .. 4 on batch A (eager), ``mbs.state``, the source tensors, ``norm``, the parameters and the Adam dict through
    a file, updates 5 .. 7 on batch B with a new ``RolloutMinibatches`` (one captured graph for the compact source, eager for
    the rows source): per update ``index``, every gathered array, stats, gradients and Adam's stats, then the final state."""
    import torch

    ref, path, total = ppo_refs[form], tmp_path / "checkpoint.pt", PPO_MB["EPOCHS"] * 4
    a = World(ref["init"])
    try:
        with a.scope():
            col = collect(a, form == "compact")
            va = values_and_advantages(a, col)
            source = minibatch_source(col, va, form)
            updates = MinibatchUpdates(a, source, va["norm"])
            updates.run(ref, 0, PPO_RESUME_STEP, check=True)
            a.side.synchronize()
            torch.save(dict(mb_state=updates.mb.state, source=source, norm=va["norm"], actor=a.actor.state_dict(),
                            critic=a.critic.state_dict(), adam=a.opt.state_dict()), path)
    finally:
        a.close()
    del a, col, va, source, updates
    gc.collect()
    torch.cuda.empty_cache()
    ckpt = torch.load(path, map_location="cpu", weights_only=False)
    assert ckpt["mb_state"].tolist() == [1, PPO_MB["B"], 0, 0] and not ckpt["source"]["obs"].is_cuda
    b = World()
    try:
        with b.scope():
            dev = b.env.device
            b.actor.load_state_dict(ckpt["actor"])
            b.critic.load_state_dict(ckpt["critic"])
            b.opt.load_state_dict(ckpt["adam"])
            updates = MinibatchUpdates(b, {key: t.to(dev) for key, t in ckpt["source"].items()}, ckpt["norm"].to(dev))
            updates.mb.state.copy_(ckpt["mb_state"])
            if form == "compact":
                updates.capture()
            updates.run(ref, PPO_RESUME_STEP, total, check=True)
            final = b.final(updates.mb)
            assert b.opt.counts() == (total, 0)
    finally:
        b.close()
    check_ppo_final(final, ref, f"{form}, resumed before update {PPO_RESUME_STEP}")
