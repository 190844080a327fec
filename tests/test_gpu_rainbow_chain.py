"""The whole loop of examples/dqn_dueling.py on the device against the composed CPU reference of tests/_rainbow_chain.py, bit
for bit: prioritised replay over an n-step ring, per-side dueling heads, the fused actor launch, both sides' ``td_error`` into
``update_priorities``.  What no per-op test and no run-against-run comparison can see is compared here: the leaves made from
the loss's own ``td_error`` and what they do to the next draw and its weights, max-leaf on records pushed after it rose, the
window's end on real cut bytes under a prioritised draw when the ring wraps, ``next_obs`` / ``masks_next`` from the window's
last slot, the per-row discount in the loss, ``dueling_backward`` between ``grad_q`` and ``backward_into``, the fused actor on
a real state across auto-resets, ``beta`` and ``epsilon`` written between graph replays, and two out-of-band acts between two
replays: a hand truncation (``set_state(truncated=)``: dropped rows) and the envs put back (``reset_from_pool`` + ``mark_cut``).

The loop is built from library calls only, as the example does, on a batch and stream of its own; the heads are made with
``env.mlp_head(H, O=6)`` and the ``linear_init`` parameters of tests/test_rainbow_chain_reference.py are copied into them, so the
reference the device is held to is the one whose coverage the CPU test asserts (asserted again here, once per module).
Comparisons go in chain order (``LINKS``), so a failure names the first link that differs."""

import pytest
from _chain_device import L, RainbowLoop
from _chain_device import check_rainbow_final as check_final
from _learner_chain import H
from _mlp_spec import linear_init
from _rainbow_chain import RAINBOW, RAINBOW_INIT_SEEDS, assert_rainbow_coverage, rainbow_reference

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def rainbow_ref(oracle):
    """The reference from the committed ``linear_init`` parameters; run once."""
    init = [linear_init(L, H, RAINBOW["O"], seed=s) for s in RAINBOW_INIT_SEEDS]
    ref = rainbow_reference(init)
    ref["init"] = init
    for k, v in ref["facts"].items():
        print(f"rainbow {k}: {v}")
    assert_rainbow_coverage(ref)
    return ref


def run_loop(ref, captured: bool, check: bool) -> dict:
    """The loop of examples/dqn_dueling.py with the reference's shapes (tests/_chain_device.py), eager or as two graphs
    replayed alternately; ``check``: every link of every round against the reference.  Returns the final state as NumPy arrays."""
    loop = RainbowLoop()
    try:
        with loop.scope():
            loop.start(ref["init"])
            loop.warm_up(ref)
            if captured:
                loop.capture()
            loop.run_rounds(ref, 0, RAINBOW["ROUNDS"], check)
            assert loop.opt.counts() == (RAINBOW["ROUNDS"], 0)
            return loop.final()
    finally:
        loop.close()


def test_rainbow_loop_captured_against_the_reference(rainbow_ref):
    """An actor graph and an update graph replayed alternately, ``ql.epsilon`` and ``pr.beta`` set between replays, the hand
    truncation and the event eagerly between two replays: every link of every round, then the final state."""
    check_final(run_loop(rainbow_ref, captured=True, check=True), rainbow_ref, "captured")


def test_rainbow_loop_eager_ends_in_the_references_state(rainbow_ref):
    """The same loop without graphs; only the final state is compared."""
    check_final(run_loop(rainbow_ref, captured=False, check=False), rainbow_ref, "eager")
