"""Every entry point of CCX_MINIBATCH with each pointer at a chosen residue mod 128 -- the observation rows and compact arrays
at {0, 16, 48, 112} (plus 8 for the rows of an odd agent count, whose alignment is 8), int64 arrays 8 further, f32 arrays 4
further and byte arrays 1 further: the weakest addresses include/ccx.h allows --, between guard bands (tests/_placed.py,
imported): a fetch, a draw and a permutation on placed sources and outputs give the bits of the same calls on a twin with
ordinary tensors; asserted are bit-equal results, every byte of every output written, 4096 untouched sentinel bytes on either
side of every array, and unchanged input bytes."""

import numpy as np
import pytest
from _placed import SENTINEL, PlacedCall
from _reset_obs_spec import make_config

pytestmark = pytest.mark.gpu

E, K, M = 5, 3, 15
FIELDS = ("obs", "actions", "logp", "advantages", "returns", "masks", "valid", "index")
INDEX = np.array([0, 14, 7, 7, -1, 15, 4, 5, 9, 10, 0, 3, 12, 13, 8, 2, 1, 6, 11], np.int64)


@pytest.mark.parametrize("off", [0, 16, 48, 112])
@pytest.mark.parametrize("form", ["rows", "compact"])
@pytest.mark.parametrize("N", [3, 8])
def test_fetch_next_and_permutation_on_placed_arrays(N, form, off):
    import torch

    from collectivecrossing_amd import OnPolicyBatch, RolloutMinibatches
    from collectivecrossing_amd.batched import BatchedCollectiveCrossing

    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    b = BatchedCollectiveCrossing(make_config(N, max_steps=12), E)
    try:
        b.set_rng_seed(77)
        L = b.obs_len
        rng = np.random.default_rng(N + off)
        W = 4 if form == "compact" else L
        f32 = np.float32
        src = dict(obs=rng.integers(-2, 9, (K, E, N, W)).astype(f32), obs0=rng.integers(-2, 9, (E, N, W)).astype(f32),
                   actions=rng.integers(0, 5, (K, E, N)).astype(np.uint8), logp=-rng.random((K, E, N)).astype(f32),
                   advantages=rng.standard_normal((K, E, N)).astype(f32), returns=rng.standard_normal((K, E, N)).astype(f32),
                   masks=(rng.integers(0, 32, (K, E, N)) | 0x10).astype(np.uint8), valid=((rng.random((K, E, N)) < 0.8) * 4).astype(np.uint8))
        rows_align = 16 if N % 2 == 0 else 8
        rows_off = off + (8 if N % 2 else 0)                             # odd N: 8 mod 16
        src_obs = (off, 16) if form == "compact" else (rows_off, rows_align)
        where = dict(obs=src_obs, obs0=src_obs, actions=(off + 1, 1), logp=(off + 4, 4), advantages=(off + 4, 4), returns=(off + 4, 4),
                     masks=(off + 1, 1), valid=(off + 1, 1))
        out_where = dict(obs=(rows_off, rows_align), actions=(off + 1, 1), logp=(off + 4, 4), advantages=(off + 4, 4),
                         returns=(off + 4, 4), masks=(off + 1, 1), valid=(off + 1, 1), index=(off + 8, 8))

        p = PlacedCall(f"RolloutMinibatches N={N} {form} +{off}")
        twin = RolloutMinibatches(b, num_steps=K, batch_size=4)
        twin.set_source(**{k: torch.from_numpy(v).cuda() for k, v in src.items()})
        placed = RolloutMinibatches(b, num_steps=K, batch_size=4)
        placed.set_source(**{k: p.inp(k, v, *where[k]) for k, v in src.items()})
        state = p.out("state", (4,), torch.int64, off + 8, 8)
        state.zero_()
        placed.state = state

        def outputs(tag, B):
            like = twin.alloc(B)
            return OnPolicyBatch(*(p.out(f"{tag}.{k}", getattr(like, k).shape, getattr(like, k).dtype, *out_where[k]) for k in FIELDS))

        B = len(INDEX)
        fetched, drawn = outputs("fetch", B), [outputs(f"next{d}", 4) for d in range(5)]
        perm = p.out("perm", (M,), torch.int64, off + 8, 8)
        want = {}
        placed.fetch(p.inp("index_in", INDEX, off + 8, 8), out=fetched)
        want["fetch"] = twin.fetch(torch.from_numpy(INDEX).cuda())
        for d in range(5):                                               # an epoch of four draws (the last padded) and one more
            placed.next(out=drawn[d])
            want[f"next{d}"] = twin.next()
        placed.permutation(2 ** 40 + 7, out=perm)
        torch.cuda.synchronize()
        assert twin.state.tolist() == [1, 4, 0, 0] and int((want["next3"].index < 0).sum()) == 1
        expected = {"state": twin.state, "perm": twin.permutation(2 ** 40 + 7)}
        for tag, res in want.items():
            expected.update({f"{tag}.{k}": getattr(res, k) for k in FIELDS})
        p.check(expected)
        for name, (view, _h) in p.outs.items():                          # every byte inside is written: twin results hold no run of sentinels
            if name.endswith(".obs"):
                assert not (view.view(torch.uint8).reshape(-1, 4) == SENTINEL).all(dim=1).any(), name
    finally:
        b.close()
