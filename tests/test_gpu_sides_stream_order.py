"""The stream-order contract of every enqueueing method of ``SideHeads``, with the harness of
tests/_stream_order.py (imported, not edited; its table stays the table of the batch's own classes): the forward on static
buffers, the fused draw, ``backward_into`` and the autograd path, each with torch's current stream another one than the
handle's, in both directions, against the same call on a twin batch with the handle's stream current throughout -- bit
patterns."""

import numpy as np
import pytest
import _stream_order as so
from _stream_order import E, H, N, Plan, dev, fill_bytes, inp, normal, param_inputs, prefilled, tensors

pytestmark = pytest.mark.gpu

K = 4                                            # leading rows of the learner-side cases: x is [K, E, N, L]


def _sides(b, O=5, keys=("boarding", "exiting")):
    from collectivecrossing_amd import SideHeads

    sides = SideHeads(b, {key: b.mlp_head(H, O=O) for key in keys})
    return sides, [pair for _, head in sides.groups for pair in param_inputs(b, head)]


def _forward(w, rng):
    import torch

    b = w.batch
    sides, params = _sides(b)
    x = inp(normal(rng, K, E, N, sides.L))
    y, hidden = prefilled((K, E, N, 5), torch.float32), prefilled((K, E, N, H), torch.float32)

    def call():
        with torch.no_grad():
            return [sides(x[0], out=y, hidden_out=hidden), hidden]
    return Plan([x] + params, call, [y, hidden])


def _sample(w, rng):
    import torch

    b = w.batch
    sides, params = _sides(b, keys=("boarding",))                        # the exiting slots are unowned: 255 / +0.0 / +0.0
    obs, masks = inp(b.observe(), 0.0), inp(b.action_masks(), 0x1F)
    out = b.alloc_sample(True, True)
    logits = prefilled((E, N, 5), torch.float32)
    fill_bytes(*tensors(out))

    def sanity(got):
        acts = got[0].reshape(E, N)
        assert (acts[:, 5:] == 255).all() and (acts[:, :5] < 5).any()
    return Plan([obs, masks] + params,
                lambda: tensors(sides.sample_actions(obs[0], masks[0], logits_out=logits, out=out)) + [logits],
                tensors(out) + [logits], sanity)


def _backward_into(w, rng):
    import torch

    b = w.batch
    sides, params = _sides(b)
    xr = dev(normal(rng, K, E, N, sides.L))
    hid = torch.empty((K, E, N, H), dtype=torch.float32, device="cuda")
    with torch.no_grad():
        sides(xr, hidden_out=hid)
    x, hidden, gy = inp(xr), inp(hid), inp(normal(rng, K, E, N, 5))
    out = sides.alloc_backward((K, E, N), want_grad_a=True)
    grads = [t for o in out for t in (o.w1t, o.b1, o.w2, o.b2)] + [out[0].grad_a]
    fill_bytes(*grads)

    def call():
        sides.backward_into(x[0], hidden[0], gy[0], out=out)
        return grads
    return Plan([x, hidden, gy] + params, call, grads)


def _autograd(O):
    def setup(w, rng):
        import torch

        b = w.batch
        sides, params = _sides(b, O=O)
        x, gy = inp(normal(rng, K, E, N, sides.L)), inp(normal(rng, K, E, N, O))

        def call():
            with torch.enable_grad():
                y = sides(x[0])
                y.backward(gy[0])
            return [y, *(p.grad for p in sides.parameters())]
        return Plan([x, gy] + params, call)
    return setup


CASES = [so.Case("sides_forward_out", "sim", ("SideHeads.forward",), _forward),
         so.Case("sides_sample_actions", "sim", ("SideHeads.sample_actions",), _sample),
         so.Case("sides_backward_into", "sim", ("SideHeads.backward_into",), _backward_into),
         so.Case("sides_autograd_actor", "sim", ("SideHeads.forward",), _autograd(5)),
         so.Case("sides_autograd_critic", "sim", ("SideHeads.forward",), _autograd(1))]


@pytest.fixture(scope="module")
def rig():
    import torch

    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    main, other = torch.cuda.Stream(), torch.cuda.Stream()
    blocker = so.Blocker()
    blocker.warm(main, other)
    yield main, other, blocker
    torch.cuda.synchronize()


def _play(case, direction, rig, block=True):
    main, other, blocker = rig
    seed = 900_000 + 1000 * CASES.index(case) + (direction == "after")   # (beyond every seed of the harness's own table)
    return so.run(case, direction, main, other, blocker, block=block, seed=seed)


@pytest.mark.parametrize("direction", ["before", "after"])
@pytest.mark.parametrize("case", CASES, ids=lambda c: c.name)
def test_order(case, direction, rig):
    want = _play(case, direction, rig, block=False)                      # the twin: the handle's stream is current
    got = _play(case, direction, rig)
    print(f"{case.name} {direction}: host {got.host_ms:.3f} ms, {len(got.got)} outputs, {sum(map(len, got.got))} bytes")
    assert got.open, "blocker too short: it had ended before the last piece was enqueued, the run proves nothing"
    assert len(got.got) == len(want.got) and got.got
    for i, (g, w) in enumerate(zip(got.got, want.got)):
        np.testing.assert_array_equal(g, w, err_msg=f"{case.name} output {i} ({direction}): "
                                      + ("the launch did not wait for its inputs" if direction == "before"
                                         else "the consumer did not wait for the launch"))
    if direction == "before":                                            # write after read: the snapshot holds the old bytes
        assert len(got.snaps) == len(got.pre)
        for i, (s, p) in enumerate(zip(got.snaps, got.pre)):
            np.testing.assert_array_equal(s, p, err_msg=f"{case.name} output {i}: overwritten while the current stream still read it")
    assert any(so.differs([g], [p]) for g, p in zip(want.got, want.pre)) or not want.pre, "the call changed no output"


def test_the_harness_table_is_unchanged():
    """This file adds nothing to the table tests/test_stream_order_table.py walks."""
    assert not any(c.name.startswith("sides_") for c in so.CASES)
