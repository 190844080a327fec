"""Completeness of the stream-order table (tests/_stream_order.py; needs no GPU): every public method of
BatchedCollectiveCrossing, LearnerOps, MlpHead and DeviceAdam that reaches the library is either played by a case of the
table, in both directions on the GPU (tests/test_gpu_stream_order.py), or exempted with a one-line reason.  A new op
cannot be added without that decision."""

import re
from pathlib import Path

import _stream_order as so


def test_every_enqueueing_method_is_in_the_table_or_exempt():
    flagged, covered, exempt = so.enqueueing_methods(), so.covered(), set(so.EXEMPT)
    undecided = sorted(flagged - covered - exempt)
    assert not undecided, (f"{undecided} reach the library: add a case to tests/_stream_order.py (both directions), or an "
                           "EXEMPT entry with the reason (host-synchronous, query only, setting only)")
    assert not covered & exempt, sorted(covered & exempt)


def test_the_walk_finds_what_it_should():
    """Anchors: direct callers, callers through a private method, through another class and through an autograd Function
    are flagged; pure Python is not."""
    flagged = so.enqueueing_methods()
    for name in ("BatchedCollectiveCrossing.step", "BatchedCollectiveCrossing.rollout_policy", "BatchedCollectiveCrossing.reset_host",
                 "LearnerOps.ppo_loss", "LearnerOps.evaluate_actions", "LearnerOps.mlp_backward", "MlpHead.forward",
                 "DeviceAdam.step", "BatchedCollectiveCrossing.masks_fused"):
        assert name in flagged, name
    for name in ("BatchedCollectiveCrossing.frame_shape", "BatchedCollectiveCrossing.rows_alignment", "LearnerOps.alloc_gae",
                 "MlpHead.to_sequential", "DeviceAdam.zero_grad"):
        assert name not in flagged, name


def test_learner_modules_reach_the_library_through_enqueue_only():
    """In learner.py, sides.py and qlearn.py a library function is named only as the first argument of ``_enqueue(``
    (which orders what it passes: tests/test_enqueue_host.py) or as a ``*_workspace_bytes`` query.  A new op that spells
    entry, call and exit by hand fails here."""
    import collectivecrossing_amd

    named = re.compile(r"_lib\.(ccx_\w+)")
    enqueued = re.compile(r"\b_enqueue\(\s*\w+\._lib\.(ccx_\w+)\s*[,)]")
    for module in ("learner.py", "sides.py", "qlearn.py"):
        text = (Path(collectivecrossing_amd.__file__).parent / module).read_text()
        ok = {m.start(1) for m in enqueued.finditer(text)}
        stray = [m.group(1) for m in named.finditer(text) if m.start(1) not in ok and not m.group(1).endswith("_workspace_bytes")]
        assert not stray, f"{module}: {stray} must go through _enqueue"
        assert ok, module


def test_table_and_exemptions_name_real_public_methods():
    classes = so._classes()
    for name in sorted(so.covered() | set(so.EXEMPT)):
        cls, _, attr = name.partition(".")
        assert cls in classes and not attr.startswith("_") and attr in vars(classes[cls]), name
    for name, reason in so.EXEMPT.items():
        assert reason.startswith((so._SYNC, so._QUERY, so._SET, "copies on", "allocation on")) and "\n" not in reason, name
    names = [c.name for c in so.CASES]
    assert len(names) == len(set(names))
    assert all(c.world in ("sim", "array", "tracked") and c.covers for c in so.CASES)
