"""Two rounds of a small PPO iteration with deep heads on the device against the per-op specs composed on the CPU, every
array of both rounds bit for bit: a ``16-32`` tanh actor and a ``16-32`` relu critic (``DeepMlpHead``, O = 5 and O = 1),
``head.sample_actions`` in the collection loop, ``compute_gae`` on the critic's own values, ``ppo_loss``, the device backward
of both heads and ONE ``DeviceAdam`` over the twelve tensors; the second round collects under the parameters the first one
left and continues the optimiser's state.  E = 8, N = 8, K = 4: an update sees 256 rows.  Run with explicit library calls
on static buffers and through ``loss.backward()`` with ``backward="device"`` heads: the same rule.

The reference composes tests/_mlp_deep_spec.py with the specs and the oracle batch that tests/_learner_chain.py composes
for the one-hidden-layer heads (its helpers are imported, not changed).  Comparisons go in chain order, so a failure names
the first link that differs."""

import numpy as np
import pytest
from _adam_spec import adam_step_spec, new_state, state_bytes
from _gae_spec import gae_spec
from _learner_chain import EF_RESET, N, POOL_SEED0, POOL_SIZE, SEED, _masks, _oracle_batch, chain_config
from _mlp_deep_spec import NAMES, RELU, TANH, deep_backward_spec, deep_spec
from _ppo_loss_spec import masked_moments_spec, ppo_loss_backward_spec, ppo_loss_spec
from _sample_spec import sample_spec

pytestmark = pytest.mark.gpu

F32 = np.float32
E, K, H1, H2, ROUNDS = 8, 4, 16, 32, 2
GAMMA, LAM, LR = 0.99, 0.95, 3e-3
HYPER = dict(clip=0.2, vf_coef=0.5, ent_coef=0.01)
ADAM_KW = dict(weight_decay=0.01, max_grad_norm=2.5)                      # the second round's norm is clipped, the first one's is not
START_STEP_COUNT = np.arange(E, dtype=np.int32) % 5 + 7                   # max_steps = 12: envs are cut in the first round already
TORCH_SEED = 20
GRAD_ORDER = tuple(f"{head}.{name}" for head in ("actor", "critic") for name in NAMES)
STEP_KEYS = ("rows", "masks", "actions", "logp", "reward", "agent_flags", "env_flags", "final_obs")


def _np(t) -> np.ndarray:
    return t.detach().cpu().numpy()


def same(got, want, msg):
    """Equal dtype, shape and bytes (the sign of a zero included)."""
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, (msg, got.dtype, want.dtype, got.shape, want.shape)
    np.testing.assert_array_equal(got.view(np.uint8), want.view(np.uint8), err_msg=msg)


# ------------------------------------------------------------------------------------------------- the reference
def _deep(x, p, activation):
    y = deep_spec(x.reshape(-1, x.shape[-1]), *p, activation)[0]
    return y.reshape(x.shape[:-1] + (y.shape[-1],))


def reference(actor, critic):
    """The two rounds from the initial parameters (six arrays each): a list of per-round dicts."""
    actor, critic = ([np.array(p, F32, copy=True) for p in h] for h in (actor, critic))
    oracle, params, ob = _oracle_batch(chain_config(), E)
    ob.set_state(step_count=START_STEP_COUNT)
    rows = ob.observe()
    weights = actor + critic                                              # the same arrays: Adam updates in place
    ms, vs, state = [np.zeros_like(p) for p in weights], [np.zeros_like(p) for p in weights], new_state()
    rounds = []
    for _ in range(ROUNDS):
        hist = {k: [] for k in STEP_KEYS}
        for _ in range(K):
            masks = _masks(oracle, params, ob)
            logits = _deep(rows, actor, TANH)
            acts, logp, _ = sample_spec(logits, masks, ob.terminated, ob.truncated, ob.step_count.copy(), ob.episode.copy(), seed=SEED)
            step_obs, reward, af, ef = ob.rollout(acts[None], auto_reset=True)
            reset = (ef[0] & EF_RESET) != 0
            for k, v in zip(STEP_KEYS, (rows, masks, acts, logp, reward[0], af[0], ef[0], step_obs[0])):
                hist[k].append(v)
            rows = np.where(reset[:, None, None], ob.observe(), step_obs[0])          # reset_obs="next"
        r = {k: np.stack(v) for k, v in hist.items()}
        r["last_rows"] = rows
        r["values"], r["last_values"] = _deep(r["rows"], critic, RELU)[..., 0], _deep(rows, critic, RELU)[..., 0]
        reset = (r["env_flags"] & EF_RESET) != 0
        r["final_values"] = np.where(reset[..., None], _deep(r["final_obs"], critic, RELU)[..., 0], F32(0.0)).astype(F32)
        adv, ret, valid = gae_spec(r["reward"], r["agent_flags"], r["env_flags"], r["values"], r["last_values"], r["final_values"], GAMMA, LAM)
        norm = masked_moments_spec(adv, valid)
        r.update(advantages=adv, returns=ret, valid=valid, norm=norm)
        x = r["rows"].reshape(-1, r["rows"].shape[-1])
        M = x.shape[0]
        logits, a1, a2 = deep_spec(x, *actor, TANH)
        vals, c1, c2 = deep_spec(x, *critic, RELU)
        args = (logits, vals[:, 0], r["actions"].reshape(M), r["logp"].reshape(M), adv.reshape(M), ret.reshape(M), r["masks"].reshape(M),
                valid.reshape(M), norm[1:3])
        r["stats"] = ppo_loss_spec(*args, **HYPER)
        gl, gv = ppo_loss_backward_spec(*args, **HYPER, stats=r["stats"])
        ga = deep_backward_spec(x, a1, a2, gl, actor[2], actor[4], TANH)
        gc = deep_backward_spec(x, c1, c2, gv[:, None], critic[2], critic[4], RELU)
        r["grads"] = [ga[k] for k in NAMES] + [gc[k] for k in NAMES]
        r["adam_stats"] = adam_step_spec(weights, r["grads"], ms, vs, state, LR, **ADAM_KW)
        for k, v in (("params", weights), ("m", ms), ("v", vs)):
            r[k] = [np.array(t, F32, copy=True) for t in v]
        r["state_bytes"] = state_bytes(state)
        rounds.append(r)
    return rounds


# ------------------------------------------------------------------------------------------------- the device run
class World:
    """A batch of its own on a side stream, the two heads and the optimiser; closed by the test."""

    def __init__(self, backward="torch"):
        import torch

        from collectivecrossing_amd import DeepMlpHead, DeviceAdam
        from collectivecrossing_amd.batched import BatchedCollectiveCrossing

        assert torch.cuda.is_available(), "gpu tests need an MI355X"
        self.env = env = BatchedCollectiveCrossing(chain_config(), E)
        assert env.num_agents == N
        self.side = torch.cuda.Stream()
        env.use_stream(self.side)
        torch.cuda.synchronize()
        with torch.cuda.stream(self.side), torch.no_grad():
            env.make_reset_pool(seed0=POOL_SEED0, size=POOL_SIZE)
            env.reset_from_pool()
            env.synchronize()
            env.set_state(step_count=START_STEP_COUNT)
            env.set_rng_seed(SEED)
            torch.manual_seed(TORCH_SEED)
            self.actor = DeepMlpHead(env, H1, H2, backward=backward)
            self.critic = DeepMlpHead(env, H1, H2, O=1, activation="relu", backward=backward)
            self.opt = DeviceAdam(env, [*self.actor.parameters(), *self.critic.parameters()], lr=LR, **ADAM_KW)
            self.obs, self.masks = env.observe(), env.action_masks()

    def heads(self):
        self.side.synchronize()
        return [[_np(getattr(h, n)) for n in NAMES] for h in (self.actor, self.critic)]

    def close(self):
        self.env.use_stream(None)
        self.env.close()


def collect(w):
    """K actor steps: ``head.sample_actions`` + a one-step rollout on [s:s+1] slabs, from where the last round stopped."""
    import torch

    from collectivecrossing_amd import SampleResult
    from collectivecrossing_amd.batched import RolloutResult

    env, dev = w.env, w.env.device
    col = dict(traj=env.alloc_rollout(K, want_final=True), actions=torch.empty((K, E, N), dtype=torch.uint8, device=dev),
               logp=torch.empty((K, E, N), device=dev), masks=torch.empty((K, E, N), dtype=torch.uint8, device=dev),
               rows=torch.empty((K, E, N, env.obs_len), device=dev))
    for s in range(K):
        col["rows"][s] = w.obs
        col["masks"][s] = w.masks
        w.actor.sample_actions(w.obs, w.masks, out=SampleResult(col["actions"][s], col["logp"][s], None))
        slab = RolloutResult(**{k: None if t is None else t[s:s + 1] for k, t in vars(col["traj"]).items()})
        w.obs = env.rollout(col["actions"][s:s + 1], auto_reset=True, reset_obs="next", out=slab, masks_out=w.masks).obs[0]
    return col


def values_and_advantages(w, col):
    import torch

    env, traj, critic = w.env, col["traj"], w.critic
    with torch.no_grad():
        values = critic(col["rows"]).squeeze(-1).contiguous()
        last_values = critic(traj.obs[K - 1]).squeeze(-1).contiguous()
        reset = (traj.env_flags & EF_RESET) != 0
        final_values = torch.zeros((K, E, N), device=env.device)
        final_values[reset] = critic(traj.final_obs[reset].contiguous()).squeeze(-1)
        gae = env.compute_gae(traj, values, last_values, final_values, gamma=GAMMA, lam=LAM)
        norm = env.masked_moments(gae.advantages, gae.valid)
    return dict(values=values, last_values=last_values, final_values=final_values, gae=gae, norm=norm)


def check_round(w, col, va, ref, tag):
    """The links in front of the update: the collection, then values, advantages and their moments."""
    w.side.synchronize()
    traj = col["traj"]
    for s in range(K):
        for k in ("rows", "masks", "actions", "logp"):
            same(_np(col[k])[s], ref[k][s], f"{tag}: {k} of step {s}")
    for k in ("reward", "agent_flags", "env_flags"):
        same(_np(getattr(traj, k)), ref[k], f"{tag}: {k}")
    reset = (ref["env_flags"] & EF_RESET) != 0
    same(_np(traj.final_obs)[reset], ref["final_obs"][reset], f"{tag}: final_obs at EF_RESET")
    same(_np(traj.obs)[-1], ref["last_rows"], f"{tag}: the rows behind the last step")
    for k in ("values", "last_values", "final_values"):
        same(_np(va[k]), ref[k], f"{tag}: {k}")
    for k in ("advantages", "returns", "valid"):
        same(_np(getattr(va["gae"], k)), ref[k], f"{tag}: {k}")
    same(_np(va["norm"]), ref["norm"], f"{tag}: norm")


def check_update(w, stats, grads, ref, tag):
    w.side.synchronize()
    opt = w.opt
    same(_np(stats), ref["stats"], f"{tag}: the loss stats")
    for g, want, name in zip(grads, ref["grads"], GRAD_ORDER):
        same(_np(g), want, f"{tag}: gradient {name}")
    same(_np(opt.stats), ref["adam_stats"], f"{tag}: Adam's stats (norm, scale, skipped, rate)")
    for k, got in (("params", opt.params), ("m", opt.m), ("v", opt.v)):
        for t, want, name in zip(got, ref[k], GRAD_ORDER):
            same(_np(t), want, f"{tag}: {k} {name} after the step")
    same(_np(opt.state), ref["state_bytes"], f"{tag}: the optimiser's state bytes")


@pytest.fixture(scope="module")
def chain_ref(oracle):
    """The reference from the initial parameters of the device's freshly made heads; run once."""
    w = World()
    try:
        init = w.heads()
    finally:
        w.close()
    rounds = reference(*init)
    acts = np.concatenate([r["actions"].reshape(-1) for r in rounds])
    resets = np.concatenate([(r["env_flags"] & EF_RESET).reshape(-1) for r in rounds])
    scales = [float(r["adam_stats"][1]) for r in rounds]
    restricted = sum(int((r["masks"] != 0x1F).sum()) for r in rounds)
    print(f"deep chain: actions drawn {sorted(set(acts.tolist()))}, env-steps with a reset {int((resets != 0).sum())}, restricted masks "
          f"{restricted}, clip scales {scales}")
    # what the two rounds exercise: every action, auto-resets of SOME envs inside both rounds (the draw key's episode moves, GAE
    # is cut and takes final_values), restricted masks, one step with the norm clipped and one without.  (No slot is dead in
    # eight steps of these episodes: dead slots under the fused launches are tests/test_gpu_mlp_deep.py's.)
    assert set(acts.tolist()) == {0, 1, 2, 3, 4} and (resets != 0).any() and (resets == 0).any() and restricted > 0
    assert all((r["env_flags"] & EF_RESET).any() for r in rounds) and scales[0] == 1.0 and scales[1] < 1.0
    assert any((a.view(np.uint32) != b.view(np.uint32)).any() for a, b in zip(rounds[0]["params"], rounds[1]["params"]))
    return dict(init=init, rounds=rounds)


def test_two_rounds_with_explicit_calls(chain_ref):
    import torch

    w = World()
    try:
        for got, want in zip(w.heads(), chain_ref["init"]):
            for g, t in zip(got, want):
                same(g, t, "the heads are made alike in every test")
        env, actor, critic, opt, dev = w.env, w.actor, w.critic, w.opt, w.env.device
        lead = (K, E, N)
        with torch.cuda.stream(w.side), torch.no_grad():
            new = lambda n: torch.empty(lead + (n,), device=dev)          # noqa: E731
            logits, a1, a2, vals, c1, c2 = new(5), new(H1), new(H2), new(1), new(H1), new(H2)
            loss = env.alloc_ppo_loss(lead)
            ga, gc = actor.alloc_param_grads(lead), critic.alloc_param_grads(lead)
            grads = [*ga.grads(), *gc.grads()]
            for i, ref in enumerate(chain_ref["rounds"]):
                col = collect(w)
                va = values_and_advantages(w, col)
                check_round(w, col, va, ref, f"round {i}")
                gae = va["gae"]
                actor(col["rows"], out=logits, hidden1_out=a1, hidden2_out=a2)
                critic(col["rows"], out=vals, hidden1_out=c1, hidden2_out=c2)
                args = (logits, vals.squeeze(-1), col["actions"], col["logp"], gae.advantages, gae.returns)
                kw = dict(masks=col["masks"], valid=gae.valid, norm=va["norm"], **HYPER)
                env.ppo_loss(*args, **kw, out=loss)
                gl, gv = env.ppo_loss_backward(*args, **kw, stats=loss.stats, out=loss)
                actor.param_grads(col["rows"], a1, a2, gl, out=ga)
                critic.param_grads(col["rows"], c1, c2, gv.unsqueeze(-1), out=gc)
                opt.step(grads=grads)
                check_update(w, loss.stats, grads, ref, f"round {i}")
        assert opt.counts() == (ROUNDS, 0)
    finally:
        w.close()


def test_two_rounds_through_autograd(chain_ref):
    """The same two rounds with ``backward="device"`` heads, ``r.loss.backward()`` and ``opt.step()`` on the ``.grad``."""
    import torch

    w = World(backward="device")
    try:
        env, opt = w.env, w.opt
        with torch.cuda.stream(w.side):
            for i, ref in enumerate(chain_ref["rounds"]):
                with torch.no_grad():
                    col = collect(w)
                va = values_and_advantages(w, col)
                check_round(w, col, va, ref, f"round {i}")
                gae = va["gae"]
                opt.zero_grad(set_to_none=True)                          # (a fresh .grad: nothing is added onto old bits)
                r = env.ppo_loss(w.actor(col["rows"]), w.critic(col["rows"]).squeeze(-1), col["actions"], col["logp"], gae.advantages,
                                 gae.returns, masks=col["masks"], valid=gae.valid, norm=va["norm"], **HYPER)
                r.loss.backward()
                opt.step()
                check_update(w, r.stats, [p.grad for p in opt.params], ref, f"round {i}, autograd")
    finally:
        w.close()
