"""CCX_MINIBATCH on the device against tests/_minibatch_spec.py and torch's own ``index_select``: the permutation kernel, the
gather on hand-made indices in both source forms (rows / compact, with and without ``obs0``, without ``masks`` / ``valid``,
without an ``obs`` output), the draws and the state over two and a half epochs, a captured ``next`` against eager calls on a
twin, the seed, every refusal, and one ``ppo_loss`` on a gathered minibatch.  E = 5 envs, K = 3 steps (M = 15 records), N = 3
(odd: 8-byte units) and N = 8 (16-byte units)."""

import numpy as np
import pytest
from _minibatch_spec import M_LIST, advance_spec, draw_spec, gather_spec, perm_spec
from _replay_spec import rows_spec
from _reset_obs_spec import make_config

pytestmark = pytest.mark.gpu

E, K, M = 5, 3, 15
SEED = 0x0123_4567_89AB_CDEF
FIELDS = ("obs", "actions", "logp", "advantages", "returns", "masks", "valid", "index")
EPOCHS = (0, 1, 2 ** 32, 2 ** 40 + 7)


def same(got, want, what=""):
    got = got.detach().cpu().numpy() if hasattr(got, "detach") else np.asarray(got)
    want = want.detach().cpu().numpy() if hasattr(want, "detach") else np.asarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, want.dtype, got.shape, want.shape)
    raw = {4: np.uint32, 8: np.uint64, 1: np.uint8}[got.dtype.itemsize]
    np.testing.assert_array_equal(got.view(raw), want.view(raw), err_msg=what)


class World:
    def __init__(self, N):
        import torch
        from collectivecrossing_amd.batched import BatchedCollectiveCrossing

        self.N = N
        b = self.batch = BatchedCollectiveCrossing(make_config(N, max_steps=12), E)
        b.make_reset_pool(seed0=3, size=32)
        b.reset_from_pool()
        b.set_rng_seed(SEED)
        self.L = b.obs_len
        self.consts = tuple(float(x) for x in b.observe()[0, 0, 2:6].cpu())
        rng = np.random.default_rng(40 + N)
        f32 = np.float32
        self.np = dict(rows=rng.standard_normal((K, E, N, self.L)).astype(f32), rows0=rng.standard_normal((E, N, self.L)).astype(f32),
                       compact=rng.integers(-2, 9, (K, E, N, 4)).astype(f32), compact0=rng.integers(-2, 9, (E, N, 4)).astype(f32),
                       actions=rng.integers(0, 5, (K, E, N)).astype(np.uint8), logp=-rng.random((K, E, N)).astype(f32),
                       advantages=rng.standard_normal((K, E, N)).astype(f32), returns=rng.standard_normal((K, E, N)).astype(f32),
                       masks=(rng.integers(0, 32, (K, E, N)) | 0x10).astype(np.uint8),
                       valid=((rng.random((K, E, N)) < 0.8) * 4).astype(np.uint8))
        self.np["masks"] |= (1 << self.np["actions"]).astype(np.uint8)    # every stored action is legal under its mask
        self.np["rows"][0, 0, 0, :3] = [np.nan, -0.0, np.inf]             # bits, not values
        self.dev = {k: torch.from_numpy(v).cuda() for k, v in self.np.items()}
        torch.cuda.synchronize()

    def source(self, form="rows", obs0=False, masks=True, valid=True, obs=True):
        """(keyword arguments of set_source, the spec's src dict)"""
        small = ("actions", "logp", "advantages", "returns")
        kw = {k: self.dev[k] for k in small}
        src = {k: self.np[k] for k in small}
        for k, on in (("masks", masks), ("valid", valid)):
            kw[k], src[k] = (self.dev[k], self.np[k]) if on else (None, None)
        kw["obs"], src["obs"] = (self.dev[form], self.np[form]) if obs else (None, None)
        kw["obs0"], src["obs0"] = (self.dev[form + "0"], self.np[form + "0"]) if obs and obs0 else (None, None)
        return kw, src

    def minibatches(self, B, **how):
        from collectivecrossing_amd import RolloutMinibatches

        mb = RolloutMinibatches(self.batch, num_steps=K, batch_size=B)
        kw, src = self.source(**how)
        mb.set_source(**kw)
        return mb, src

    def close(self):
        self.batch.close()


@pytest.fixture(scope="module", params=[3, 8], ids=lambda n: f"N{n}")
def world(request):
    import torch

    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    w = World(request.param)
    yield w
    w.close()


def prefilled(mb, B, want_obs=True):
    import torch

    out = mb.alloc(B, want_obs=want_obs)
    for t in vars(out).values():
        if t is not None:
            t.view(torch.uint8).fill_(0xA5)
    return out


def check(world, out, src, index, tag):
    want = gather_spec(src, index, E, world.consts)
    for k in FIELDS:
        got = getattr(out, k)
        if want[k] is None:
            assert got is None, (tag, k)
        else:
            same(got, want[k], f"{tag}: {k}")


# ---------------------------------------------------------------------------------------------------------------- the permutation
def test_permutation_equals_the_spec(world):
    import torch

    b = world.batch
    for m in M_LIST:
        out = torch.full((m,), -7, dtype=torch.int64, device="cuda")
        for epoch in EPOCHS:
            b._enqueue(b._lib.ccx_minibatch_permutation, m, epoch, out)
            same(out, perm_spec(m, SEED, epoch), f"M {m} epoch {epoch}")
    mb, _ = world.minibatches(4)
    for epoch in EPOCHS:
        same(mb.permutation(epoch), perm_spec(M, SEED, epoch), f"permutation({epoch})")
    out = torch.empty((M,), dtype=torch.int64, device="cuda")
    assert mb.permutation(3, out=out) is out
    same(out, perm_spec(M, SEED, 3))


def test_seed_changes_the_permutation_and_repeats_it(world):
    b = world.batch
    mb, _ = world.minibatches(4)
    first = mb.permutation(0).cpu().numpy()
    b.set_rng_seed(SEED + 1)
    other = mb.permutation(0).cpu().numpy()
    same(other, perm_spec(M, SEED + 1, 0))
    b.set_rng_seed(SEED)
    again = mb.permutation(0).cpu().numpy()
    assert not np.array_equal(first, other) and np.array_equal(first, again)


# ---------------------------------------------------------------------------------------------------------------- fetch
INDEX = np.array([0, 14, 7, 7, -1, 15, 4, 5, 9, 10, 0, 2 ** 40, -2 ** 62, 3, 14, 1, 6, 11, 12, 13, 8, 2, 7], np.int64)   # in range, repeated, -1, M


@pytest.mark.parametrize("obs0", [False, True], ids=["obs_as_is", "obs0_shift"])
@pytest.mark.parametrize("form", ["rows", "compact"])
def test_fetch_equals_index_select(world, form, obs0):
    import torch

    mb, src = world.minibatches(4, form=form, obs0=obs0)
    index = torch.from_numpy(INDEX).cuda()
    B = len(INDEX)
    out = prefilled(mb, B)
    assert mb.fetch(index, out=out) is out
    check(world, out, src, INDEX, f"fetch {form} obs0={obs0}")
    assert mb.state.tolist() == [0, 0, 0, 0]                             # a fetch leaves the state alone
    # torch's own statement, for the records in range: index_select of each flattened source
    inside = torch.from_numpy(np.flatnonzero((INDEX >= 0) & (INDEX < M))).cuda()
    at = index[inside]
    for k in ("actions", "logp", "advantages", "returns", "masks", "valid"):
        want = torch.index_select(world.dev[k].reshape(M, world.N), 0, at)
        same(getattr(out, k)[inside], want, k)
    flat = world.dev[form].reshape(M, world.N, -1)
    if obs0:
        flat = torch.cat([world.dev[form + "0"], flat[:M - E]])          # record j acted on the row behind step s - 1
    picked = torch.index_select(flat, 0, at)
    if form == "compact":
        same(out.obs[inside], world.batch.expand_observations(picked), "obs: expand_observations of the selected records")
    else:
        same(out.obs[inside], picked, "obs")
    outside = torch.from_numpy(np.flatnonzero((INDEX < 0) | (INDEX >= M))).cuda()
    same(out.obs[outside][0], rows_spec(np.zeros((world.N, 4), np.float32), world.consts), "the EMPTY row")
    assert (out.actions[outside] == 255).all() and (out.valid[outside] == 0).all() and (out.masks[outside] == 0x10).all()
    # in place: the index output may be the index input
    out2 = prefilled(mb, B)
    out2.index.copy_(index)
    mb.fetch(out2.index, out=out2)
    check(world, out2, src, INDEX, "fetch in place")


@pytest.mark.parametrize("form", ["rows", "compact"])
def test_fetch_without_masks_valid_or_obs(world, form):
    import torch

    index = torch.from_numpy(INDEX).cuda()
    mb, src = world.minibatches(4, form=form, masks=False, valid=False)
    out = prefilled(mb, len(INDEX))
    mb.fetch(index, out=out)
    check(world, out, src, INDEX, "no masks, no valid")
    inside = (INDEX >= 0) & (INDEX < M)
    assert (out.masks.cpu().numpy()[inside] == 0x1F).all() and (out.valid.cpu().numpy()[inside] == 4).all()
    mb, src = world.minibatches(4, form=form, obs0=True)
    out = prefilled(mb, len(INDEX), want_obs=False)                      # a source with obs, an output without
    mb.fetch(index, out=out)
    check(world, out, dict(src, obs=None), INDEX, "no obs output")
    mb, src = world.minibatches(4, obs=False)
    out = mb.fetch(index)
    assert out.obs is None
    check(world, out, src, INDEX, "no obs source")
    fresh = mb.fetch(index[:1])                                          # B = 1, allocated by the call
    check(world, fresh, src, INDEX[:1], "B = 1")


# ---------------------------------------------------------------------------------------------------------------- next
@pytest.mark.parametrize("B", [4, 15, 16, 64])
@pytest.mark.parametrize("form", ["rows", "compact"])
def test_next_walks_the_epochs(world, form, B):
    mb, src = world.minibatches(B, form=form, obs0=True)
    per_epoch = -(-M // B)
    assert mb.minibatches_per_epoch == per_epoch
    state = np.zeros(4, np.int64)
    out = prefilled(mb, B)
    seen = []
    for d in range((5 * per_epoch + 1) // 2):                            # two and a half epochs
        assert mb.state.tolist() == state.tolist()
        index = draw_spec(M, B, SEED, state)
        advance_spec(state, B, M)
        assert mb.next(out=out) is out
        check(world, out, src, index, f"next {form} B={B} draw {d}")
        seen.append(out.index.cpu().numpy().copy())
    assert mb.state.tolist() == state.tolist()
    for epoch in range(2):                                               # the union of an epoch's indices is exactly [0, M)
        got = np.concatenate(seen[epoch * per_epoch:(epoch + 1) * per_epoch])
        assert sorted(got[got >= 0].tolist()) == list(range(M)) and (got[got < 0] == -1).all()
        assert (got >= 0).sum() == M and not (got[:M] < 0).any()         # padding only at the end of the last draw
    mb.rewind()
    assert mb.state.tolist() == [0, 0, 0, 0]
    same(mb.next().index, seen[0], "after rewind()")
    mb.rewind(2 ** 40 + 7)
    assert mb.state.tolist() == [2 ** 40 + 7, 0, 0, 0]
    same(mb.next().index, draw_spec(M, B, SEED, [2 ** 40 + 7, 0]), "after rewind(epoch)")


def test_state_outside_its_range_reads_nothing_wild(world):
    import torch

    mb, src = world.minibatches(4, obs0=True)
    for cursor in (-1, -2 ** 63, M, M + 1, 2 ** 62, 2 ** 63 - 1):
        mb.state.copy_(torch.tensor([7, cursor, 0, 0], dtype=torch.int64))
        out = mb.next(out=prefilled(mb, 4))
        check(world, out, src, np.full(4, -1, np.int64), f"cursor {cursor}")
        assert mb.state.tolist() == [8, 0, 0, 0]
    mb.state.copy_(torch.tensor([-1, 12, 0, 0], dtype=torch.int64))      # epoch 2^64 - 1, then 0
    index = draw_spec(M, 4, SEED, [-1, 12])
    assert (index[:3] >= 0).all() and index[3] == -1
    check(world, mb.next(), src, index, "epoch -1")
    assert mb.state.tolist() == [0, 0, 0, 0]


def test_captured_next_advances_with_every_replay(world):
    import torch

    b = world.batch
    side = torch.cuda.Stream()
    b.use_stream(side)
    try:
        torch.cuda.synchronize()
        with torch.cuda.stream(side):
            mb, src = world.minibatches(4, form="compact", obs0=True)
            twin, _ = world.minibatches(4, form="compact", obs0=True)
            out = prefilled(mb, 4)
            side.synchronize()
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph, stream=side):
                mb.next(out=out)
            side.synchronize()
            assert mb.state.tolist() == [0, 0, 0, 0]                     # a capture runs nothing
            for r in range(10):
                graph.replay()
                want = twin.next()
                side.synchronize()
                for k in FIELDS:
                    same(getattr(out, k), getattr(want, k), f"replay {r}: {k}")
                assert mb.state.tolist() == twin.state.tolist()
            assert mb.state.tolist() == [2, 8, 0, 0]
    finally:
        b.use_stream(None)


# ---------------------------------------------------------------------------------------------------------------- refusals
def test_wrong_tensors_raise_value_error(world):
    import torch
    from collectivecrossing_amd import OnPolicyBatch, RolloutMinibatches

    b, N, L = world.batch, world.N, world.L
    for bad in (lambda: RolloutMinibatches(object(), 3, 4), lambda: RolloutMinibatches(b, 0, 4), lambda: RolloutMinibatches(b, 2.5, 4),
                lambda: RolloutMinibatches(b, "x", 4), lambda: RolloutMinibatches(b, (1 << 31) // E + 1, 4),
                lambda: RolloutMinibatches(b, 3, 0), lambda: RolloutMinibatches(b, 3, (1 << 31) // N + 1)):
        with pytest.raises(ValueError):
            bad()
    mb = RolloutMinibatches(b, num_steps=K, batch_size=4)
    with pytest.raises(ValueError):
        mb.next()                                                        # no source yet
    kw, _ = world.source()
    d = world.dev
    wrong = [dict(kw, obs=d["rows"][:2]), dict(kw, obs=d["rows"].double()), dict(kw, obs=d["rows"].cpu()),
             dict(kw, obs=d["rows"][..., :5]), dict(kw, obs=d["compact"], obs0=d["rows0"]), dict(kw, obs=None, obs0=d["rows0"]),
             dict(kw, obs=d["rows"].transpose(0, 1)), dict(kw, actions=d["masks"].float()), dict(kw, actions=None),
             dict(kw, logp=d["logp"].double()), dict(kw, advantages=d["advantages"][:, :4]), dict(kw, returns=None),
             dict(kw, masks=d["masks"].int()), dict(kw, valid=d["valid"][0]), dict(kw, obs0=d["rows0"][:4]),
             dict(kw, logp=d["logp"].cpu().numpy())]
    misplaced = torch.empty(K * E * N * L + 1, device="cuda")[1:].view(K, E, N, L)
    wrong.append(dict(kw, obs=misplaced))                                # 4 mod 8: not even the odd-N alignment
    for n, bad in enumerate(wrong):
        with pytest.raises(ValueError):
            mb.set_source(**bad)
            pytest.fail(f"set_source refusal {n} did not raise")
    mb.set_source(**kw)
    good = mb.alloc()
    outs = [OnPolicyBatch(*[getattr(good, k) if k != f else t for k in FIELDS])
            for f, t in (("obs", good.obs[:3]), ("actions", good.logp), ("logp", good.logp.double()), ("advantages", None),
                         ("returns", good.returns.cpu()), ("masks", good.masks[:, :1]), ("valid", good.index), ("index", good.index.int()))]
    for n, bad in enumerate(outs + [object(), mb.alloc(5)]):
        with pytest.raises(ValueError):
            mb.next(out=bad)
            pytest.fail(f"out refusal {n} did not raise")
    index = torch.zeros(4, dtype=torch.int64, device="cuda")
    for n, bad in enumerate((lambda: mb.fetch(index.int()), lambda: mb.fetch(index.cpu()), lambda: mb.fetch(index[:0]),
                             lambda: mb.fetch(index.view(2, 2)), lambda: mb.fetch([0, 1]), lambda: mb.fetch(index, out=mb.alloc(5)),
                             lambda: mb.permutation(-1), lambda: mb.permutation(1.5), lambda: mb.permutation(2 ** 63),
                             lambda: mb.permutation(0, out=torch.zeros(M + 1, dtype=torch.int64, device="cuda")),
                             lambda: mb.permutation(0, out=torch.zeros(M, dtype=torch.int32, device="cuda")),
                             lambda: mb.rewind(-1), lambda: mb.rewind("x"))):
        with pytest.raises(ValueError):
            bad()
            pytest.fail(f"refusal {n} did not raise")
    nob = RolloutMinibatches(b, num_steps=K, batch_size=4)
    nob.set_source(**dict(kw, obs=None))
    with pytest.raises(ValueError):
        nob.next(out=good)                                               # an obs output without an obs source
    torch.cuda.synchronize()
    assert mb.state.tolist() == [0, 0, 0, 0]                             # a refused call enqueues nothing


def test_the_library_refuses_before_any_launch(world):
    import torch
    from collectivecrossing_amd import _abi

    b, N, L = world.batch, world.N, world.L
    lib, h, d = b._lib, b._h, world.dev
    B = 4
    state = torch.zeros(4, dtype=torch.int64, device="cuda")
    index = torch.zeros(B, dtype=torch.int64, device="cuda")
    out = {k: torch.full_like(t, 0x5A) for k, t in vars(world.minibatches(B)[0].alloc()).items()}
    src = dict(obs0=d["rows0"], obs=d["rows"], **{k: d[k] for k in ("actions", "logp", "advantages", "returns", "masks", "valid")})
    before = {k: t.clone() for k, t in out.items()}

    def ptr(t, shift=0):
        return None if t is None else t.data_ptr() + shift

    def call(fn="next", handle=h, Kv=K, compact=0, Bv=B, st=state, idx=index, **over):
        s = {k: ptr(t) for k, t in src.items()}
        o = {k: ptr(t) for k, t in out.items()}
        for k, v in over.items():
            (s if k in s else o)[k[4:] if k.startswith("out_") else k] = v
        srcs = [s[k] for k in ("obs0", "obs", "actions", "logp", "advantages", "returns", "masks", "valid")]
        outs = [o[k] for k in FIELDS]
        if fn == "next":
            return lib.ccx_minibatch_next(handle, Kv, compact, *srcs, ptr(st), Bv, *outs)
        return lib.ccx_minibatch_fetch(handle, Kv, compact, *srcs, Bv, ptr(idx), *outs)

    row_align = 16 if N % 2 == 0 else 8
    cases = [(dict(handle=None), "NULL handle"), (dict(actions=None), "NULL source"), (dict(logp=None), "NULL source"),
             (dict(advantages=None), "NULL source"), (dict(returns=None), "NULL source"), (dict(out_actions=None), "NULL output"),
             (dict(out_index=None), "NULL output"), (dict(out_valid=None), "NULL output"), (dict(st=None), "NULL state"),
             (dict(fn="fetch", idx=None), "NULL index"), (dict(Kv=0), "K = 0"), (dict(Kv=(1 << 31) // E + 1), "out of range"),
             (dict(Kv=1 << 62), "out of range"), (dict(Bv=0), "batch = 0"), (dict(Bv=(1 << 31) // N + 1), "batch"), (dict(obs=None), "needs obs_steps"),
             (dict(obs=ptr(d["rows"], row_align // 2)), "observation rows"), (dict(obs0=ptr(d["rows0"], row_align // 2)), "observation rows"),
             (dict(out_obs=ptr(out["obs"], row_align // 2)), "observation rows"),
             (dict(compact=1, obs=ptr(d["compact"], 8), obs0=ptr(d["compact0"])), "compact"),
             (dict(compact=1, obs=ptr(d["compact"]), obs0=ptr(d["compact0"], 8)), "compact"),
             (dict(st=state[1:].view(torch.uint8)[4:]), "state and index"), (dict(out_index=ptr(out["index"], 4)), "state and index"),
             (dict(fn="fetch", idx=index.view(torch.uint8)[4:]), "state and index"), (dict(logp=ptr(d["logp"], 2)), "4-byte"),
             (dict(out_returns=ptr(out["returns"], 1)), "4-byte")]
    for kw, word in cases:
        assert call(**kw) == _abi.EINVAL, (kw, word)
        assert word in lib.ccx_last_error().decode(), (word, lib.ccx_last_error())
    perm = torch.full((M,), 0x5A, dtype=torch.int64, device="cuda")
    for args, word in (((None, M, 0, perm.data_ptr()), "NULL handle"), ((h, M, 0, None), "NULL out"), ((h, 0, 0, perm.data_ptr()), "M = 0"),
                       ((h, 1 << 31, 0, perm.data_ptr()), "out of range"), ((h, M - 1, 0, perm.data_ptr() + 4), "8-byte")):
        assert lib.ccx_minibatch_permutation(*args) == _abi.EINVAL, word
        assert word in lib.ccx_last_error().decode(), (word, lib.ccx_last_error())
    torch.cuda.synchronize()
    assert state.tolist() == [0, 0, 0, 0] and (perm == 0x5A).all()
    for k, t in out.items():
        assert torch.equal(t, before[k]), k                              # nothing was launched
    assert call() == _abi.OK and call(fn="fetch") == _abi.OK             # and the same arguments unchanged are accepted
    torch.cuda.synchronize()
    assert state.tolist() == [0, B, 0, 0]


# ---------------------------------------------------------------------------------------------------------------- end to end
def test_ppo_loss_on_a_gathered_minibatch(world):
    """The loss on the minibatch ``next`` wrote equals the loss on the ``index_select``-ed one bit for bit, padding included:
    B = 16 of M = 15, so one row is the EMPTY one, which ``valid`` = 0 takes out."""
    import torch

    b, N, d = world.batch, world.N, world.dev
    mb, src = world.minibatches(16, form="rows", obs0=True)
    out = mb.next()
    index = out.index.clone()
    assert int((index < 0).sum()) == 1 and index[-1] == -1
    at = index.clamp(min=0)
    pad = (index < 0)[:, None]
    flat = {k: d[k].reshape(M, N) for k in ("actions", "logp", "advantages", "returns", "masks", "valid")}
    sel = {k: torch.index_select(t, 0, at) for k, t in flat.items()}
    sel["actions"] = torch.where(pad, torch.full_like(sel["actions"], 255), sel["actions"])
    sel["valid"] = torch.where(pad, torch.zeros_like(sel["valid"]), sel["valid"])
    sel["masks"] = torch.where(pad, torch.full_like(sel["masks"], 0x10), sel["masks"])
    for k in ("logp", "advantages", "returns"):
        sel[k] = torch.where(pad, torch.zeros_like(sel[k]), sel[k])
    torch.manual_seed(7)
    logits, values = torch.randn((16, N, 5), device="cuda"), torch.randn((16, N), device="cuda")
    hyper = dict(clip=0.2, vf_coef=0.5, ent_coef=0.01)
    got = b.ppo_loss(logits, values, out.actions, out.logp, out.advantages, out.returns, masks=out.masks, valid=out.valid, **hyper)
    want = b.ppo_loss(logits, values, sel["actions"], sel["logp"], sel["advantages"], sel["returns"], masks=sel["masks"],
                      valid=sel["valid"], **hyper)
    same(got.stats, want.stats, "ppo_loss stats")
    assert float(got.stats[6]) == float((sel["valid"] != 0).sum()) > 0   # the rows that count: the padding is not among them
