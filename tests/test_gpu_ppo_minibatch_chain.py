"""The whole iteration of examples/ppo_minibatches.py on the device against the composed CPU reference of
tests/_rainbow_chain.py (``ppo_minibatch_reference``), bit for bit: the collection with a real actor across auto-resets, the
critic's values, GAE and the moments as in tests/test_gpu_learner_chain.py, then ``RolloutMinibatches.set_source(..., obs0=)``
and ONE captured update graph with ``mb.next`` inside, replayed eight times.  What is compared here and nowhere else: the
device's cursor walking two epochs whose last minibatch is partly EMPTY (index -1, action 255, valid 0) straight into
``ppo_loss``, the backward and Adam; ``obs0`` and the rollout's own ``obs`` answering for the row each step ACTED ON; the
epoch entering the permutation; and the compact source giving the rows source's parameters.

The heads are made with ``env.mlp_head`` and the ``linear_init`` parameters of tests/test_rainbow_chain_reference.py are copied
into them, so the reference is the one whose coverage the CPU test asserts (asserted again here, once per module)."""

import pytest
from _chain_device import L, MinibatchUpdates, World, _np, collect, minibatch_source, values_and_advantages
from _chain_device import check_ppo_final as check_final
from _learner_chain import GRAD_ORDER, H, PPO_INIT_SEEDS
from _mlp_spec import linear_init
from _rainbow_chain import PPO_MB, assert_ppo_minibatch_coverage, ppo_minibatch_reference, same, same_lists

pytestmark = pytest.mark.gpu

FORMS = ("rows", "compact")


@pytest.fixture(scope="module")
def refs(oracle):
    """The two references from the committed ``linear_init`` parameters; run once."""
    init = [linear_init(L, H, 5, seed=PPO_INIT_SEEDS[0]), linear_init(L, H, 1, seed=PPO_INIT_SEEDS[1])]
    out = {form: ppo_minibatch_reference(*init, form) for form in FORMS}
    for k, v in out["rows"]["facts"].items():
        print(f"ppo minibatches {k}: {v}")
    for ref in out.values():
        ref["init"] = init
        assert_ppo_minibatch_coverage(ref)
    return out


def check_inputs(col, va, ref, form):
    """Everything ``set_source`` is given, and what it was made from."""
    traj = col["traj"]
    same(_np(col["obs0"]), ref["rows"][0], "obs0: the rows step 0 acts on")
    same(_np(traj.obs)[:-1], ref["rows"][1:], "the rollout's own obs: the rows behind every step but the last")
    same(_np(traj.obs)[-1], ref["last_rows"], "the rows behind the last step")
    for k in ("masks", "actions", "logp"):
        same(_np(col[k]), ref[k], k)
    for k in ("reward", "agent_flags", "env_flags"):
        same(_np(getattr(traj, k)), ref[k], k)
    if form == "compact":
        same(_np(traj.obs_compact), ref["source"]["obs"], "the rollout's compact records")
    for k in ("values", "last_values", "final_values"):
        same(_np(va[k]), ref[k], k)
    for k in ("advantages", "returns", "valid"):
        same(_np(getattr(va["gae"], k)), ref[k], k)
    same(_np(va["norm"]), ref["norm"], "norm")


def run_updates(w, col, va, ref, form, captured, check):
    """The eight updates of examples/ppo_minibatches.py on static buffers, ``mb.next`` inside (tests/_chain_device.py): eager,
    or ONE captured graph replayed eight times; the rate changes after the fourth.  ``check``: every link after every step."""
    updates = MinibatchUpdates(w, minibatch_source(col, va, form), va["norm"])
    assert updates.mb.minibatches_per_epoch == ref["per_epoch"] == 4
    if captured:
        updates.capture()
    updates.run(ref, 0, PPO_MB["EPOCHS"] * updates.mb.minibatches_per_epoch, check)
    got = w.final(updates.mb)
    assert w.opt.counts() == (8, 0)
    return got


@pytest.mark.parametrize("form", FORMS)
def test_ppo_minibatch_iteration_against_the_reference(refs, form):
    """The captured run ends in the reference's state; its eager twin is checked after every step.  The compact form's final
    parameters are also the rows form's."""
    import torch

    ref = refs[form]
    w, e = World(ref["init"]), World(ref["init"])
    try:
        with torch.cuda.stream(e.side), torch.no_grad():
            col = collect(e, form == "compact")
            va = values_and_advantages(e, col)
            e.side.synchronize()
            check_inputs(col, va, ref, form)
            eager = run_updates(e, col, va, ref, form, captured=False, check=True)
        check_final(eager, ref, f"{form}, eager")
        with torch.cuda.stream(w.side), torch.no_grad():
            col = collect(w, form == "compact")
            captured = run_updates(w, col, values_and_advantages(w, col), ref, form, captured=True, check=False)
        check_final(captured, ref, f"{form}, captured")
        same_lists(captured["params"], refs["rows"]["params"], GRAD_ORDER, f"{form}: the rows form's final parameters")
    finally:
        w.close()
        e.close()
