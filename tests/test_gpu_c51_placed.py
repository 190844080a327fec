"""The three entry points of CCX_C51 with each pointer at the weakest address include/ccx.h allows -- +4 for the f32 arrays
(rows of 51 floats are 204 bytes: nothing wider can be assumed), +16 for ``q`` (16-byte aligned: what ccx_q_actions takes), +8
for ``reward`` and the workspace, +1 for the byte arrays --, between guard bands (tests/_placed.py, imported): the call on
ordinary tensors gives the expected bits; asserted are bit-equal results, 4096 untouched sentinel bytes on either side of
every array, and unchanged input bytes."""

import numpy as np
import pytest
from _c51_spec import c51_args, make_c51_case
from _placed import PlacedCall
from _reset_obs_spec import make_config

pytestmark = pytest.mark.gpu

A, M = 51, 257
KEYS = ("logits", "actions", "reward", "done", "next_target", "next_online", "masks_next", "valid", "weights")
OFFSET = dict(logits=4, actions=1, reward=8, done=1, next_target=4, next_online=4, masks_next=1, valid=1, weights=4, discount=4)


@pytest.fixture(scope="module")
def batch():
    import torch

    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    from collectivecrossing_amd.batched import BatchedCollectiveCrossing

    b = BatchedCollectiveCrossing(make_config(8, max_steps=12), 4)
    yield b
    b.close()


@pytest.mark.parametrize("with_discount", (False, True))
def test_every_pointer_at_its_weakest_address(batch, with_discount):
    import torch

    from collectivecrossing_amd import CategoricalQ
    from collectivecrossing_amd.categorical import CategoricalLossResult

    cq = CategoricalQ(batch, atoms=A)
    kw = c51_args(make_c51_case(M, A, seed=21), True, True, True, True, with_discount)
    d = {k: (None if v is None else torch.from_numpy(np.ascontiguousarray(v)).cuda()) for k, v in kw.items()}
    gamma = None if with_discount else 0.97
    gloss = torch.tensor([-1.75], device="cuda")
    want_q = cq.q_values(d["logits"])
    want = cq.loss(*(d[k] for k in KEYS), gamma=gamma, discount=d["discount"], want_row_loss=True)
    want_g = cq.loss_backward(d["logits"], d["actions"], want.proj, d["valid"], d["weights"], stats=want.stats, grad_loss=gloss)
    batch.synchronize()
    assert torch.isfinite(want.stats).all() and want.stats[6] > 100

    p = PlacedCall(f"c51 A={A} M={M} discount={with_discount}")
    pd = {k: p.inp(k, v, OFFSET[k], 8 if k == "reward" else (4 if OFFSET[k] == 4 else 1)) for k, v in d.items()}
    f = torch.float32
    cq.q_values(pd["logits"], out=p.out("q", (M, 5), f, 16, 16))
    need = int(batch._lib.ccx_c51_workspace_bytes(M))
    out = CategoricalLossResult(None, p.out("stats", (8,), f, 4, 4), p.out("row_loss", (M,), f, 4, 4), p.out("proj", (M, A), f, 4, 4),
                                p.scratch("workspace", need, 8, 8), p.out("grad_logits", (M, 5, A), f, 4, 4))
    cq.loss(*(pd[k] for k in KEYS), gamma=gamma, discount=pd["discount"], out=out)
    cq.loss_backward(pd["logits"], pd["actions"], out.proj, pd["valid"], pd["weights"], stats=out.stats,
                     grad_loss=p.inp("grad_loss", gloss, 4, 4), out=out)
    p.check(dict(q=want_q, stats=want.stats, row_loss=want.row_loss, proj=want.proj, grad_logits=want_g))
