"""The calls of CCX_MLP_DEEP with EVERY pointer at its weakest legal address (tests/_placed.py): x / obs, hidden1, hidden2,
grad_a1 and grad_a2 at +16 of a 128-byte line, the workspace at +8, every other f32 array -- the six parameters, y, grad_y,
the six gradients, logp, entropy, logits, q, epsilon -- at +4, the u8 arrays at +1, each between sentinel bands.  Each call is
compared, byte for byte, with the same call on ordinary tensors; the guards and the inputs' own bytes are checked after
each."""

import numpy as np
import pytest
from _mlp_deep_spec import NAMES, RELU, TANH, make_deep_backward_case
from _placed import PlacedCall
from _reset_obs_spec import make_config

pytestmark = pytest.mark.gpu

# (L, H1, H2, O, activation, rows): the workload's head over two blocks and a tail tile; the largest one with the LDS opt-in;
# one layer-1 wave under two layer-2 waves with an odd L (rows * L is no multiple of 4); fewer layer-2 waves
CASES = ((38, 64, 64, 5, TANH, 321), (262, 256, 256, 8, RELU, 70), (7, 16, 32, 5, TANH, 129), (38, 48, 16, 6, RELU, 65))
GRADS = tuple("grad_" + n for n in NAMES)


@pytest.fixture(scope="module")
def batch():
    import torch

    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    from collectivecrossing_amd.batched import BatchedCollectiveCrossing

    b = BatchedCollectiveCrossing(make_config(8, max_steps=12), 16)
    b.make_reset_pool(seed0=5, size=256)
    yield b
    b.close()


@pytest.mark.parametrize("L,H1,H2,O,act,rows", CASES)
def test_every_pointer_at_its_weakest_address(batch, L, H1, H2, O, act, rows):
    import torch

    lib, f = batch._lib, torch.float32
    c = make_deep_backward_case(rows, L, H1, H2, O, act, seed=rows + O)
    dev = {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in c.items()}
    dims = (rows, L, H1, H2, O, act)
    shapes = dict(zip(GRADS, ((L, H1), (H1,), (H1, H2), (H2,), (O, H2), (O,))), grad_a1=(rows, H1), grad_a2=(rows, H2))
    # ---- the same calls on ordinary tensors
    y, h1, h2 = (torch.empty((rows, k), device="cuda") for k in (O, H1, H2))
    batch._enqueue(lib.ccx_mlp_deep_forward, *dims, dev["x"], *(dev[k] for k in NAMES), y, h1, h2)
    need = lib.ccx_mlp_deep_backward_workspace_bytes(rows, L, H1, H2, O)
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    plain = {k: torch.empty(s, device="cuda") for k, s in shapes.items()}
    batch._enqueue(lib.ccx_mlp_deep_backward, *dims, dev["x"], dev["hidden1"], dev["hidden2"], dev["grad_y"], dev["w2t"], dev["w3"], ws,
                   *plain.values())
    batch.synchronize()
    assert y.dtype is f and np.isfinite(y.cpu().numpy()).all()

    # ---- the forward, placed: with both hiddens, with one, with none
    for with1, with2 in ((True, True), (True, False), (False, True), (False, False)):
        pc = PlacedCall(f"ccx_mlp_deep_forward {L}-{H1}-{H2}-{O}, {rows} rows, hiddens {with1} {with2}")
        x = pc.inp("x", dev["x"], 16, 16)
        params = [pc.inp(k, dev[k], 4, 4) for k in NAMES]
        py = pc.out("y", (rows, O), f, 4, 4)
        p1 = pc.out("hidden1", (rows, H1), f, 16, 16) if with1 else None
        p2 = pc.out("hidden2", (rows, H2), f, 16, 16) if with2 else None
        batch._enqueue(lib.ccx_mlp_deep_forward, *dims, x, *params, py, p1, p2)
        batch.synchronize()
        pc.check({k: v for k, v, on in (("y", y, True), ("hidden1", h1, with1), ("hidden2", h2, with2)) if on})

    # ---- the backward, placed: with both grad_a and without
    for with_ga in (True, False):
        pc = PlacedCall(f"ccx_mlp_deep_backward {L}-{H1}-{H2}-{O}, {rows} rows, grad_a {with_ga}")
        x, a, b = pc.inp("x", dev["x"], 16, 16), pc.inp("hidden1", dev["hidden1"], 16, 16), pc.inp("hidden2", dev["hidden2"], 16, 16)
        gy, w2t, w3 = pc.inp("grad_y", dev["grad_y"], 4, 4), pc.inp("w2t", dev["w2t"], 4, 4), pc.inp("w3", dev["w3"], 4, 4)
        pws = pc.scratch("workspace", need, 8, 8)
        outs = [pc.out(k, shapes[k], f, 4, 4) for k in GRADS]
        ga = [pc.out(k, shapes[k], f, 16, 16) if with_ga else None for k in ("grad_a1", "grad_a2")]
        batch._enqueue(lib.ccx_mlp_deep_backward, *dims, x, a, b, gy, w2t, w3, pws, *outs, *ga)
        batch.synchronize()
        pc.check({k: v for k, v in plain.items() if with_ga or k in GRADS})


@pytest.mark.parametrize("H1,H2,O,act", ((64, 64, 5, TANH), (16, 48, 6, RELU)))
def test_fused_actor_launches_on_placed_arrays(batch, H1, H2, O, act):
    import torch

    lib, f, u8 = batch._lib, torch.float32, torch.uint8
    E, N, L = batch.num_envs, batch.num_agents, batch.obs_len
    batch.reset_from_pool()
    batch.set_rng_seed(77)
    batch.rollout_greedy(9, want_obs=False)
    obs, masks = batch.observe(), batch.action_masks()
    c = make_deep_backward_case(4, L, H1, H2, O, act, seed=O)
    dev = {k: torch.from_numpy(np.ascontiguousarray(c[k])).cuda() for k in NAMES}
    dev["w3"] *= 4.0
    eps = torch.full((1,), 0.25, device="cuda")
    if O == 5:
        plain = dict(actions=torch.empty((E, N), dtype=u8, device="cuda"), logp=torch.empty((E, N), device="cuda"),
                     entropy=torch.empty((E, N), device="cuda"), logits=torch.empty((E, N, 5), device="cuda"))
        batch._enqueue(lib.ccx_mlp_deep_sample_actions, H1, H2, act, obs, *(dev[k] for k in NAMES), masks, 0, *plain.values())
        batch.synchronize()
        pc = PlacedCall(f"ccx_mlp_deep_sample_actions {H1}-{H2}")
        po, pm = pc.inp("obs", obs, 16, 16), pc.inp("masks", masks, 1, 1)
        params = [pc.inp(k, dev[k], 4, 4) for k in NAMES]
        outs = [pc.out("actions", (E, N), u8, 1, 1), pc.out("logp", (E, N), f, 4, 4), pc.out("entropy", (E, N), f, 4, 4),
                pc.out("logits", (E, N, 5), f, 4, 4)]
        batch._enqueue(lib.ccx_mlp_deep_sample_actions, H1, H2, act, po, *params, pm, 0, *outs)
        batch.synchronize()
        pc.check(plain)
    plain = dict(actions=torch.empty((E, N), dtype=u8, device="cuda"), explored=torch.empty((E, N), dtype=u8, device="cuda"),
                 q=torch.empty((E, N, 5), device="cuda"))
    batch._enqueue(lib.ccx_mlp_deep_q_actions, H1, H2, act, O, obs, *(dev[k] for k in NAMES), masks, eps, *plain.values())
    batch.synchronize()
    pc = PlacedCall(f"ccx_mlp_deep_q_actions {H1}-{H2}-{O}")
    po, pm, pe = pc.inp("obs", obs, 16, 16), pc.inp("masks", masks, 1, 1), pc.inp("epsilon", eps, 4, 4)
    params = [pc.inp(k, dev[k], 4, 4) for k in NAMES]
    outs = [pc.out("actions", (E, N), u8, 1, 1), pc.out("explored", (E, N), u8, 1, 1), pc.out("q", (E, N, 5), f, 4, 4)]
    batch._enqueue(lib.ccx_mlp_deep_q_actions, H1, H2, act, O, po, *params, pm, pe, *outs)
    batch.synchronize()
    pc.check(plain)
    assert plain["explored"].any() and (plain["actions"] < 5).any()
