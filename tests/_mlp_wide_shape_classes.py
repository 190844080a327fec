"""The (L, H, O) shapes at which the wide perceptron kernels (csrc/ccx_mlp_wide.hip) are run, and the branch of their layout
each is there for.  TEST INFRASTRUCTURE ONLY.

CCX_MLP_WIDE accepts 1 <= L <= 512, H = 16 G with G = 1 .. 16, 1 <= O <= 320.  The forward runs layer 2 over chunks of C
outputs -- the most, in multiples of 32, whose [G][C][65] partials fit 65536 bytes of LDS, 32 where those do not, never more
than O -- and opts in above 65536 bytes (the x tile of 64 (L | 1) floats, or the partials from G = 8 on).  The backward's
blocks kernel gives grid.y slices of 256 output tiles to ONE part each: the first slices1 walk [x | 1]^T ga in sub-tiles of
rows1 rows with w2 streamed in slabs of S = min(O, 4096 / H) outputs, the others grad_y^T [hidden | 1] in sub-tiles of rows2
rows.  The rule depends on none of this.

The figures below were computed by the library's own functions (csrc/ccx_mlp_wide.h); tests/test_mlp_wide_shape_classes.py
recomputes every one of them through the host-rule shim and asserts that the classes are covered, so a catalogue shape that
leaves its class -- or a class boundary that moves -- fails there, on the CPU."""

from __future__ import annotations

from typing import NamedTuple

from _mlp_spec import RELU, TANH

LDS_BUDGET = 65536


class WideShape(NamedTuple):
    L: int
    H: int
    O: int
    act: int
    chunk: int                         # outputs of a chunk of the forward's layer 2
    chunks: int                        # chunks per tile
    forward_bytes: int                 # dynamic LDS of a forward workgroup
    slab: int                          # outputs of a w2 slab
    slabs: int
    rows1: int                         # rows of a sub-tile in the slices of [x | 1]^T ga
    rows2: int                         # .. of grad_y^T [hidden | 1]
    slices1: int
    grid_y: int
    why: str

    @property
    def dims(self):
        return (self.L, self.H, self.O, self.act)

    @property
    def last_chunk_partial(self):
        return self.O % self.chunk != 0

    @property
    def opt_in(self):
        return self.forward_bytes > LDS_BUDGET

    @property
    def elements(self):
        return (self.L + 1) * self.H + self.O * (self.H + 1)


CATALOGUE = (
    WideShape(38, 64, 255, TANH, 32, 8, 33280, 64, 4, 64, 64, 1, 6, "the 8-agent batch's C51 head: a last chunk of 31, a last slab of 63"),
    WideShape(7, 16, 224, RELU, 224, 1, 58240, 224, 1, 32, 64, 1, 3, "one wave, one whole chunk of 224"),
    WideShape(7, 16, 225, TANH, 224, 2, 58240, 225, 1, 32, 64, 1, 3, "a last chunk of one output"),
    WideShape(38, 64, 64, RELU, 32, 2, 33280, 64, 1, 64, 64, 1, 3, "two whole chunks, the last O of one slab"),
    WideShape(38, 64, 65, TANH, 32, 3, 33280, 64, 2, 64, 64, 1, 3, "a second slab of one output"),
    WideShape(7, 112, 255, RELU, 32, 8, 58240, 36, 8, 64, 64, 1, 9, "G = 7: the last forward without the opt-in; slabs of 36, a last one of 3"),
    WideShape(7, 48, 255, TANH, 64, 4, 49920, 85, 3, 64, 64, 1, 5, "G = 3: chunks of 64, a last one of 63; slabs of 85, no whole number of quads"),
    WideShape(7, 128, 32, TANH, 32, 1, 66560, 32, 1, 64, 64, 1, 3, "G = 8: the first partials with the opt-in"),
    WideShape(7, 256, 17, RELU, 17, 1, 70720, 16, 2, 32, 32, 1, 3, "G = 16, a chunk of 17; a second slab of one output"),
    WideShape(255, 16, 9, TANH, 9, 1, 65280, 9, 1, 32, 64, 1, 2, "odd L; the last x tile without the opt-in"),
    WideShape(256, 16, 9, RELU, 9, 1, 65792, 9, 1, 32, 64, 2, 3, "the first x tile with the opt-in; two slices of the first part"),
    WideShape(512, 16, 9, TANH, 9, 1, 131328, 9, 1, 16, 64, 3, 4, "the largest x tile; sub-tiles of 16 rows"),
    WideShape(200, 64, 255, RELU, 32, 8, 51456, 64, 4, 32, 64, 4, 9, "sub-tiles of 32 rows beside four slabs"),
    WideShape(38, 256, 255, TANH, 32, 8, 133120, 16, 16, 32, 32, 3, 20, "G = 16: 133120 bytes of partials; sixteen slabs"),
    WideShape(330, 256, 320, RELU, 32, 10, 133120, 16, 20, 16, 32, 21, 42, "sub-tiles of 16 rows at the widest head"),
    WideShape(512, 256, 320, TANH, 32, 10, 133120, 16, 20, 8, 32, 33, 54, "every limit at once: sub-tiles of 8 rows, grid.y = 54"),
)

# O in 1 .. 8 at which the wide entry points must give the narrow ones' bits (kernel against kernel)
NARROW = ((38, 64, 1, TANH), (38, 64, 5, RELU), (262, 256, 8, TANH))


def by_dims(L, H, O):
    return next(s for s in CATALOGUE if (s.L, s.H, s.O) == (L, H, O))


def backward_rows(R):
    """row counts around one sub-tile of R rows, two sub-tiles and a tail, and one block"""
    return (R - 1, R, R + 1, 2 * R + 3, 256, 257)


FORWARD_ROWS = (1, 63, 64, 65, 129)
