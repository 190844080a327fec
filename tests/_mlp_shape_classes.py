"""The (L, H, O) shapes at which the perceptron kernels are run beyond tests/_mlp_spec.SHAPES, and the branch of the
kernels' layout each is there for.  TEST INFRASTRUCTURE ONLY.

CCX_MLP accepts 1 <= L <= 512, H = 16 G with G = 1 .. 16 waves, 1 <= O <= 8, and the layout of its kernels depends on the
shape: the backward's blocks kernels (csrc/ccx_mlp_backward.hip) walk a block in sub-tiles of R = 64, 32, 16 or 8 rows --
the most whose row images fit 65536 bytes of LDS beside w2, eight more bytes per row in the picked-rows kernel of
ccx_sides_backward -- over grid.y slices of 256 output tiles; the forward's workgroup (csrc/ccx_mlp_tile.h) has G waves and
an x tile of 64 (L | 1) floats, opted in above 65536 bytes.  The rule of each op depends on none of this.

The figures below were computed by the library's own functions (ccx_mlp_grad::sub_rows, grid_y, ccx_mlp::lds_floats);
tests/test_mlp_shape_classes.py recomputes every one of them through the host-rule shims and asserts that the classes are
covered, so a catalogue shape that leaves its class -- or a class boundary that moves -- fails there, on the CPU."""

from __future__ import annotations

from typing import NamedTuple

from _mlp_spec import RELU, TANH

LDS_BUDGET = 65536
PICKED_PER_ROW = 8                                                         # the flat row (a long long) of a picked row


class Shape(NamedTuple):
    L: int
    H: int
    O: int
    act: int
    r_adjacent: int                    # rows of a sub-tile, ccx_mlp_backward
    r_picked: int                      # .. ccx_sides_backward
    bytes_adjacent: int                # dynamic LDS of a blocks workgroup
    bytes_picked: int
    forward_bytes: int                 # dynamic LDS of a forward workgroup (ccx_mlp_forward)
    grid_y: int                        # slices of 256 output tiles
    why: str

    @property
    def dims(self):
        return (self.L, self.H, self.O, self.act)

    @property
    def elements(self):
        """output elements of a backward call: what the NumPy spec's Python loop walks"""
        return (self.L + 1) * self.H + self.O * (self.H + 1)


BACKWARD = (
    Shape(106, 64, 5, TANH, 64, 64, 64768, 65280, 27392, 2, "last L before the drop to 32 rows, near the budget"),
    Shape(110, 64, 5, TANH, 32, 32, 33536, 33792, 28416, 2, "first R = 32"),
    Shape(206, 64, 5, RELU, 32, 32, 45824, 46080, 52992, 4, "the 50-agent workload's head"),
    Shape(255, 16, 1, TANH, 32, 32, 37952, 38208, 65280, 2, "odd L; last forward without the opt-in"),
    Shape(256, 16, 1, RELU, 32, 32, 38464, 38720, 65792, 2, "first forward with the opt-in, even L"),
    Shape(257, 16, 1, TANH, 32, 32, 38464, 38720, 65792, 2, "forward with the opt-in, odd L"),
    Shape(368, 256, 8, TANH, 16, 8, 65536, 36928, 94464, 24, "exactly the budget; the two kernels differ in R"),
    Shape(484, 256, 1, RELU, 16, 8, 65536, 33344, 124160, 31, "exactly the budget with O = 1"),
    Shape(372, 256, 8, RELU, 8, 8, 36992, 37056, 95488, 25, "first R = 8"),
    Shape(511, 240, 7, TANH, 8, 8, 38848, 38912, 130816, 31, "odd L, G = 15, O = 7: a padded grad_y quad"),
    Shape(512, 256, 8, TANH, 8, 8, 41472, 41536, 131328, 33, "every limit at once; grid.y = 33"),
    Shape(512, 16, 1, RELU, 16, 16, 35648, 35776, 131328, 3, "largest x tile, one wave"),
)

# every G = H / 16 in the forward: (7, H, 3), 64 rows to a sub-tile in the backward, which these do not run
EVERY_G = tuple((7, 16 * g, 3, TANH if g % 2 else RELU) for g in range(1, 17))

EXACT_BUDGET = ((368, 256, 8), (484, 256, 1))
SIDES_BACKWARD = ((110, 64, 5), (368, 256, 8), (511, 240, 7), (512, 256, 8))
SIDES_FORWARD = ((256, 16, 1), (511, 240, 7), (512, 256, 8))

# the NumPy backward spec walks a Python loop over every output element and row count, the host-compiled rule does not, and
# tests/test_mlp_backward_host_rule.py shows the two equal on every shape above: at two blocks of rows below this many
# elements, at nine rows above
NUMPY_SPEC_BELOW = 20000
# tests/test_gpu_mlp_shapes.py: the NumPy spec is the reference of a test that asks it for fewer final sums than this (one per
# element and row count), the host-compiled rule of the others
NUMPY_SPEC_FINAL_SUMS = 100000


def by_dims(L, H, O):
    return next(s for s in BACKWARD if (s.L, s.H, s.O) == (L, H, O))


def backward_rows(R):
    """row counts around one sub-tile of R rows, two sub-tiles and a tail, and one block"""
    return (R - 1, R, R + 1, 2 * R + 3, 256, 257)


FORWARD_ROWS = (1, 63, 64, 65, 129)
