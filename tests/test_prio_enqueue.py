"""prioritized.py reaches the library through ``_enqueue`` only (the walk of tests/test_replay_enqueue.py, on the new module): a
library function is named only as the first argument of ``_enqueue(`` -- the size query of the constructor excepted --, which
orders every tensor it passes: the leaves, the tree, ``pstate`` and ``beta_dev`` travel as arguments.  And the public
surface: the lazy exports, the ABI table.  No GPU."""

import inspect
import re
from pathlib import Path

import collectivecrossing_amd
from collectivecrossing_amd import _abi

QUERIES = {"ccx_prio_tree_words"}


def test_prioritized_reaches_the_library_through_enqueue_only():
    named = re.compile(r"_lib\.(ccx_\w+)")
    enqueued = re.compile(r"\b_enqueue\(\s*\w+\._lib\.(ccx_\w+)\s*[,)]")
    text = (Path(collectivecrossing_amd.__file__).parent / "prioritized.py").read_text()
    ok = {m.start(1) for m in enqueued.finditer(text)}
    stray = [m.group(1) for m in named.finditer(text) if m.start(1) not in ok and m.group(1) not in QUERIES]
    assert not stray, f"prioritized.py: {stray} must go through _enqueue"
    assert sorted(m.group(1) for m in enqueued.finditer(text)) == ["ccx_prio_push", "ccx_prio_sample", "ccx_prio_update"]
    assert "torch.rand" not in text and "Generator" not in text           # nothing comes from torch's generator


def test_the_priorities_travel_as_arguments():
    from collectivecrossing_amd.prioritized import PrioritizedReplay

    src = inspect.getsource(PrioritizedReplay)
    calls = {m.group(1): src[m.end():].split("\n\n")[0][:260] for m in re.finditer(r"_enqueue\(\s*\w+\._lib\.(ccx_\w+),", src)}
    assert all(k in calls["ccx_prio_push"] for k in ("ring.state", "self.leaf", "self.pstate"))
    assert all(k in calls["ccx_prio_update"] for k in ("self.leaf", "self.pstate", "index", "also=tds"))
    assert all(k in calls["ccx_prio_sample"] for k in ("self.leaf", "self.pstate", "self.beta_dev", "self.tree", "out.batch.index",
                                                       "out.weights", "out.leaf_drawn"))
    # the ring's own calls stay the ring's: push and fetch are called, not restated
    assert "ring.push(" in src and "self.ring.fetch(" in src and "ccx_replay_" not in src


def test_exports_and_prototypes():
    import ctypes as C

    from collectivecrossing_amd import PrioritizedBatch, PrioritizedReplay
    from collectivecrossing_amd.prioritized import PrioritizedBatch as PB
    from collectivecrossing_amd.prioritized import PrioritizedReplay as PR

    assert PrioritizedReplay is PR and PrioritizedBatch is PB
    assert {"PrioritizedReplay", "PrioritizedBatch"} <= set(collectivecrossing_amd.__all__)
    for name, arity in (("ccx_prio_tree_words", 1), ("ccx_prio_push", 6), ("ccx_prio_update", 10), ("ccx_prio_sample", 11)):
        restype, args = _abi.PROTOTYPES[name]
        assert len(args) == arity, name
    assert _abi.PROTOTYPES["ccx_prio_tree_words"][0] is C.c_int64 and _abi.ABI_VERSION == 5 and _abi.PRIO_MAX_TD == 8
    header = (Path(collectivecrossing_amd.__file__).parent.parent / "include" / "ccx.h").read_text()
    for name, (_, args) in ((n, _abi.PROTOTYPES[n]) for n in ("ccx_prio_push", "ccx_prio_update", "ccx_prio_sample", "ccx_prio_tree_words")):
        proto = re.search(r"\b(?:int|int64_t) " + name + r"\(([^;]*)\);", header).group(1)
        assert len(re.sub(r"/\*.*?\*/", "", proto, flags=re.S).split(",")) == len(args), name
    assert [f for f in PrioritizedBatch.__dataclass_fields__] == ["batch", "weights", "leaf_drawn"]
    for method in ("push", "update_priorities", "sample", "alloc_batch", "clear", "state_dict", "load_state_dict", "beta"):
        assert hasattr(PrioritizedReplay, method)
