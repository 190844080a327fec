"""The four entry points of CCX_DUELING with each pointer at the weakest address include/ccx.h allows -- +16 for the rows
of six and of five and for the observation rows, +4 for the parameters, the rate and ``q``, +1 for the byte arrays --,
between guard bands (tests/_placed.py, imported): the call on ordinary tensors gives the expected bits; asserted are bit-equal
results, 4096 untouched sentinel bytes on either side of every array, and unchanged input bytes."""

import numpy as np
import pytest
from _dueling_spec import make_dueling_rows
from _mlp_spec import linear_init
from _placed import PlacedCall
from _reset_obs_spec import make_config

pytestmark = pytest.mark.gpu

SEED = 0x0123_4567_89AB_CDEF
PARAMS = ("w1t", "b1", "w2", "b2")


@pytest.fixture(scope="module")
def batches():
    import torch

    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    from collectivecrossing_amd.batched import BatchedCollectiveCrossing

    made = {}

    def get(N, E):
        if (N, E) not in made:
            b = BatchedCollectiveCrossing(make_config(N, max_steps=12), E)
            b.make_reset_pool(seed0=5, size=64)
            b.reset_from_pool()
            b.set_rng_seed(SEED)
            rng = np.random.default_rng(N + E)
            b.rollout(rng.integers(0, 5, size=(14, E, N), dtype=np.uint8), auto_reset=True, want_traj=False)   # a second episode
            st = b.get_state()
            term = st["terminated"].copy()
            term[::3, 0] = 1                                             # dead slots, whatever the steps left
            b.set_state(terminated=term, truncated=st["truncated"], step_count=st["step_count"], episode=st["episode"])
            made[N, E] = b
        return made[N, E]

    yield get
    for b in made.values():
        b.close()


@pytest.mark.parametrize("M", (1, 63, 65, 257))                          # 6 M and 5 M floats with and without a tail behind the last piece
def test_forward_and_backward_on_placed_rows(batches, M):
    import torch

    from collectivecrossing_amd import QLearning

    ql = QLearning(batches(8, 9))
    num = 3
    rows = [make_dueling_rows(M, seed=M + i, special=i == 0) for i in range(num)]
    want_q = [ql.dueling(torch.from_numpy(va).cuda()) for va, _ in rows]
    want_g = ql.dueling_backward(torch.from_numpy(rows[0][1]).cuda())
    p = PlacedCall(f"dueling M={M}")
    vas = tuple(p.inp(f"va[{i}]", va, 16, 16) for i, (va, _) in enumerate(rows))
    qs = tuple(p.out(f"q[{i}]", (M, 5), torch.float32, 16, 16) for i in range(num))
    ql.dueling_into(vas, qs)
    ql.dueling_backward(p.inp("grad_q", rows[0][1], 16, 16), out=p.out("grad_va", (M, 6), torch.float32, 16, 16))
    p.check({**{f"q[{i}]": want_q[i] for i in range(num)}, "grad_va": want_g})


def _heads(batch, H, O, keys, p=None):
    """MlpHeads with Linear-style parameters, a different draw per key; with ``p`` the parameters live in placed arrays at +4."""
    import torch

    heads = {}
    for i, key in enumerate(keys):
        head = batch.mlp_head(H, O)
        w1t, b1, w2, b2 = linear_init(batch.obs_len, H, O, seed=40 + i)
        values = dict(w1t=w1t, b1=b1, w2=(w2 * np.float32(4.0)).astype(np.float32), b2=b2)
        with torch.no_grad():
            for name in PARAMS:
                if p is None:
                    getattr(head, name).copy_(torch.from_numpy(values[name]))
                else:
                    getattr(head, name).data = p.inp(f"{key}.{name}", values[name], 4, 4)
        heads[key] = head
    return heads


@pytest.mark.parametrize("O", (5, 6))
@pytest.mark.parametrize("N,E,H", [(3, 22, 16), (8, 9, 64)])             # 66 and 72 slots: a full tile and a tail tile
def test_fused_actor_launches_on_placed_arrays(batches, N, E, H, O):
    import torch

    from collectivecrossing_amd import QLearning, SideHeads
    from collectivecrossing_amd.qlearn import QActions

    b = batches(N, E)
    obs, masks = b.observe(), b.action_masks()
    ql = QLearning(b, epsilon=0.4)
    head = _heads(b, H, O, ("all",))["all"]
    sides = SideHeads(b, _heads(b, H, O, ("boarding",)))
    want_q, want_sq = torch.empty((E, N, 5), device="cuda"), torch.full((E, N, 5), 7.0, device="cuda")
    want = ql.mlp_q_actions(head, obs, masks, want_explored=True, q_out=want_q)
    want_s = ql.sides_q_actions(sides, obs, masks, want_explored=True, q_out=want_sq)
    torch.cuda.synchronize()
    assert (want.actions == 255).any() and want.explored.any() and not want.explored.all()

    p = PlacedCall(f"mlp_q_actions N={N} E={E} H={H} O={O}")
    pl = QLearning(b, epsilon=0.4)
    pl.epsilon_dev = p.inp("epsilon", pl.epsilon_dev, 4, 4)
    phead = _heads(b, H, O, ("all",), p)["all"]
    out = QActions(p.out("actions", (E, N), torch.uint8, 1, 1), p.out("explored", (E, N), torch.uint8, 1, 1))
    pl.mlp_q_actions(phead, p.inp("obs", obs, 16, 16), p.inp("masks", masks, 1, 1), q_out=p.out("q_out", (E, N, 5), torch.float32, 4, 4), out=out)
    p.check(dict(actions=want.actions, explored=want.explored, q_out=want_q))

    p = PlacedCall(f"sides_q_actions N={N} E={E} H={H} O={O}")
    pl = QLearning(b, epsilon=0.4)
    pl.epsilon_dev = p.inp("epsilon", pl.epsilon_dev, 4, 4)
    psides = SideHeads(b, _heads(b, H, O, ("boarding",), p))
    out = QActions(p.out("actions", (E, N), torch.uint8, 1, 1), p.out("explored", (E, N), torch.uint8, 1, 1))
    q_out = p.out("q_out", (E, N, 5), torch.float32, 4, 4)
    q_out.fill_(7.0)                                                     # unowned slots keep what the array held
    pl.sides_q_actions(psides, p.inp("obs", obs, 16, 16), p.inp("masks", masks, 1, 1), q_out=q_out, out=out)
    p.check(dict(actions=want_s.actions, explored=want_s.explored, q_out=want_sq))
