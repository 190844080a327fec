"""The three calls of CCX_MLP_WIDE with EVERY pointer at its weakest legal address (tests/_placed.py): x, hidden and grad_a at
+16 of a 128-byte line, the workspace at +8, every other f32 array -- the four parameters, y, grad_y, the four gradients -- at
+4, each between sentinel bands.  A row of y or grad_y is 4 O bytes (1020 at A = 51), so rows start at every 4-byte residue
whatever the base; the base at +4 takes the last excuse away.  Each call is compared, byte for byte, with the same call on
ordinary tensors; the guards and the inputs' own bytes are checked after each."""

import numpy as np
import pytest
from _mlp_backward_spec import make_mlp_backward_case
from _mlp_spec import RELU, TANH
from _placed import PlacedCall
from _reset_obs_spec import make_config

pytestmark = pytest.mark.gpu

# (L, H, O, activation, rows): the customary head over two blocks and a tail tile; the widest one with the LDS opt-in; one
# wave, an odd L and a partial last chunk (rows * L is no multiple of 4)
CASES = ((38, 64, 255, TANH, 321), (9, 256, 320, RELU, 70), (7, 16, 225, TANH, 129))


@pytest.fixture(scope="module")
def batch():
    import torch

    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    from collectivecrossing_amd.batched import BatchedCollectiveCrossing

    b = BatchedCollectiveCrossing(make_config(8, max_steps=12), 16)
    yield b
    b.close()


@pytest.mark.parametrize("L,H,O,act,rows", CASES)
def test_every_pointer_at_its_weakest_address(batch, L, H, O, act, rows):
    import torch

    lib, f = batch._lib, torch.float32
    c = make_mlp_backward_case(rows, L, H, O, act, seed=rows + O)
    dev = {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in c.items()}
    # ---- the same calls on ordinary tensors
    y, hid = torch.empty((rows, O), device="cuda"), torch.empty((rows, H), device="cuda")
    batch._enqueue(lib.ccx_mlp_wide_forward, rows, L, H, O, act, dev["x"], dev["w1t"], dev["b1"], dev["w2"], dev["b2"], y, hid)
    need = lib.ccx_mlp_wide_backward_workspace_bytes(rows, L, H, O)
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    plain = {k: torch.empty(s, device="cuda") for k, s in (("grad_w1t", (L, H)), ("grad_b1", (H,)), ("grad_w2", (O, H)), ("grad_b2", (O,)),
                                                           ("grad_a", (rows, H)))}
    batch._enqueue(lib.ccx_mlp_wide_backward, rows, L, H, O, act, dev["x"], dev["hidden"], dev["grad_y"], dev["w2"], ws, *plain.values())
    batch.synchronize()
    assert y.dtype is f and np.isfinite(y.cpu().numpy()).all()

    # ---- the forward, placed
    pc = PlacedCall(f"ccx_mlp_wide_forward {L}-{H}-{O}, {rows} rows")
    x = pc.inp("x", dev["x"], 16, 16)
    params = [pc.inp(k, dev[k], 4, 4) for k in ("w1t", "b1", "w2", "b2")]
    py, ph = pc.out("y", (rows, O), f, 4, 4), pc.out("hidden", (rows, H), f, 16, 16)
    batch._enqueue(lib.ccx_mlp_wide_forward, rows, L, H, O, act, x, *params, py, ph)
    batch.synchronize()
    pc.check(dict(y=y, hidden=hid))
    # .. without hidden
    pc = PlacedCall(f"ccx_mlp_wide_forward {L}-{H}-{O}, {rows} rows, no hidden")
    x = pc.inp("x", dev["x"], 16, 16)
    params = [pc.inp(k, dev[k], 4, 4) for k in ("w1t", "b1", "w2", "b2")]
    py = pc.out("y", (rows, O), f, 4, 4)
    batch._enqueue(lib.ccx_mlp_wide_forward, rows, L, H, O, act, x, *params, py, None)
    batch.synchronize()
    pc.check(dict(y=y))

    # ---- the backward, placed: with grad_a and without
    for with_ga in (True, False):
        pc = PlacedCall(f"ccx_mlp_wide_backward {L}-{H}-{O}, {rows} rows, grad_a {with_ga}")
        x, h = pc.inp("x", dev["x"], 16, 16), pc.inp("hidden", dev["hidden"], 16, 16)
        gy, w2 = pc.inp("grad_y", dev["grad_y"], 4, 4), pc.inp("w2", dev["w2"], 4, 4)
        pws = pc.scratch("workspace", need, 8, 8)
        outs = [pc.out(k, tuple(plain[k].shape), f, 4, 4) for k in ("grad_w1t", "grad_b1", "grad_w2", "grad_b2")]
        ga = pc.out("grad_a", (rows, H), f, 16, 16) if with_ga else None
        batch._enqueue(lib.ccx_mlp_wide_backward, rows, L, H, O, act, x, h, gy, w2, pws, *outs, ga)
        batch.synchronize()
        pc.check({k: v for k, v in plain.items() if with_ga or k != "grad_a"})
