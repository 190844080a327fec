"""A whole categorical (C51) double-DQN loop with prioritised n-step replay on the device against the composed CPU reference of
tests/_c51_chain.py, bit for bit.  What the per-op tests of ``CategoricalQ`` cannot see, because they feed every kernel arrays
made for it, is compared here: ``q_values`` feeding ``q_actions`` on a live batch across auto-resets; ``loss`` reading
``discount``, ``valid`` and ``masks_next`` from a real ``NStepReplay`` fetch and ``weights`` from a real
``PrioritizedReplay.sample``; ``row_loss`` going back into ``update_priorities`` and what the new leaves do to the next draws;
``grad_logits`` in its ``[..., 5, A]`` layout taken apart into five ``mlp_backward`` calls, and Adam stepping on the twenty
results; the target copy; all of it eager, replayed from two graphs, and through ``loss.backward()``.

The loop is built from library calls only (tests/_chain_device.py ``CategoricalLoop``) on a batch and stream of its own; the
heads are made with ``env.mlp_head(H, O=8)`` and the ``linear_init`` parameters of tests/test_c51_chain_reference.py are copied
into them, so the reference the device is held to is the one whose coverage and sensitivity the CPU test asserts (the coverage
asserted again here, once per module).  Comparisons go in chain order (``C51_LINKS``), so a failure names the first link that
differs."""

import pytest
from _c51_chain import C51, assert_c51_coverage, c51_init, c51_reference
from _chain_device import CategoricalLoop
from _chain_device import check_c51_final as check_final

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def c51_ref(oracle):
    """The reference from the committed ``linear_init`` parameters; run once and left unchanged."""
    init = c51_init()
    ref = c51_reference(init)
    ref["init"] = init
    for k, v in ref["facts"].items():
        print(f"c51 {k}: {v}")
    assert_c51_coverage(ref)
    return ref


def run_loop(ref, captured: bool = False, autograd: bool = False) -> dict:
    """One loop of WARMUP + ROUNDS actor steps and ROUNDS updates, every link of every round against the reference; returns
    the final state as NumPy arrays."""
    loop = CategoricalLoop(autograd=autograd)
    try:
        with loop.scope():
            loop.start(ref["init"])
            loop.warm_up(ref)
            if captured:
                loop.capture()
            loop.run_rounds(ref, 0, C51["ROUNDS"], check=True)
            assert loop.opt.counts() == (C51["ROUNDS"], 0)
            return loop.final()
    finally:
        loop.close()


def test_c51_loop_eager_against_the_reference(c51_ref):
    """Static buffers, no graph: every link of every round equal in dtype, shape and bytes (the sign of a zero included),
    then the final parameters, target, moments, Adam state, ring state, leaves, ``pstate`` and cut bytes."""
    check_final(run_loop(c51_ref), c51_ref, "eager")


def test_c51_loop_captured_against_the_reference(c51_ref):
    """An actor graph and an update graph replayed alternately, ``ql.epsilon`` and ``pr.beta`` set between replays, the hand
    truncation and the event eagerly between two replays: every link of every round, then the final state."""
    check_final(run_loop(c51_ref, captured=True), c51_ref, "captured")


def test_c51_loop_through_autograd_against_the_reference(c51_ref):
    """The update in its autograd form: a leaf logits tensor that requires a gradient is filled from the heads,
    ``r.loss.backward()`` runs ``ccx_c51_loss_backward`` and ``logits.grad`` is taken apart for the five heads.  The same
    links and the same final state: ``_CategoricalLoss`` and the static path are one computation inside a loop too."""
    check_final(run_loop(c51_ref, autograd=True), c51_ref, "autograd")
