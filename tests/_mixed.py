"""The reference-recorded mixed-control episodes (tests/golden/mixed/g15_mixed_*.npz, made by gen_golden_mixed.py) and the
inputs the tests derive from them."""

from __future__ import annotations

import sys

import numpy as np
from _fixtures import GOLDEN, Golden

sys.path.insert(0, str(GOLDEN))
from gen_golden_mixed import garbage_bytes  # noqa: E402  (the generator's own definition of the garbage)

MIXED_NPZ = sorted(p.stem for p in (GOLDEN / "mixed").glob("g15_mixed_*.npz"))


class MixedGolden(Golden):
    def __init__(self, name: str):
        super().__init__(f"mixed/{name}")
        self.name = name
        self.mask = int(self["scripted_mask"])
        self.policy = str(self["policy"])
        self.slots = [a for a in range(self.N) if (self.mask >> a) & 1]

    def tensor(self) -> np.ndarray:
        """The action tensor a caller hands over: the recorded bytes in the tensor-driven slots, GARBAGE (uniform 0..4) in
        the scripted ones."""
        t = self["actions"].copy()
        t[:, :, self.slots] = garbage_bytes(self.name, t.shape)[:, :, self.slots]
        return t

    def identity_order(self) -> bool:
        return bool((self["order"] == np.arange(self.N, dtype=np.uint8)).all())
