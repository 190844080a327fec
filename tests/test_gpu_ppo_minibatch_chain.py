"""The whole iteration of examples/ppo_minibatches.py on the device against the composed CPU reference of
tests/_rainbow_chain.py (``ppo_minibatch_reference``), bit for bit: the collection with a real actor across auto-resets, the
critic's values, GAE and the moments as in tests/test_gpu_learner_chain.py, then ``RolloutMinibatches.set_source(..., obs0=)``
and ONE captured update graph with ``mb.next`` inside, replayed eight times.  What is compared here and nowhere else: the
device's cursor walking two epochs whose last minibatch is partly EMPTY (index -1, action 255, valid 0) straight into
``ppo_loss``, the backward and Adam; ``obs0`` and the rollout's own ``obs`` answering for the row each step ACTED ON; the
epoch entering the permutation; and the compact source giving the rows source's parameters.

The heads are made with ``env.mlp_head`` and the ``linear_init`` parameters of tests/test_rainbow_chain_reference.py are copied
into them, so the reference is the one whose coverage the CPU test asserts (asserted again here, once per module)."""

import numpy as np
import pytest
from _learner_chain import (EF_RESET, GRAD_ORDER, H, N, POOL_SEED0, POOL_SIZE, PPO, PPO_INIT_SEEDS, SEED, START_STEP_COUNT, chain_config,
                            ppo_lr)
from _mlp_spec import linear_init
from _rainbow_chain import PPO_MB, PPO_MB_KEYS, assert_ppo_minibatch_coverage, ppo_minibatch_reference, same, same_lists

pytestmark = pytest.mark.gpu

L = 6 + 4 * N
FORMS = ("rows", "compact")


def _np(t) -> np.ndarray:
    return t.detach().cpu().numpy()


@pytest.fixture(scope="module")
def refs(oracle):
    """The two references from the committed ``linear_init`` parameters; run once."""
    init = [linear_init(L, H, 5, seed=PPO_INIT_SEEDS[0]), linear_init(L, H, 1, seed=PPO_INIT_SEEDS[1])]
    out = {form: ppo_minibatch_reference(*init, form) for form in FORMS}
    for k, v in out["rows"]["facts"].items():
        print(f"ppo minibatches {k}: {v}")
    for ref in out.values():
        ref["init"] = init
        assert_ppo_minibatch_coverage(ref)
    return out


def compact_of_rows(rows):
    import torch

    return torch.stack([rows[:, 1, 6:10]] + [rows[:, 0, 6 + 4 * j:10 + 4 * j] for j in range(1, rows.shape[-2])], dim=1).contiguous()


class World:
    """A batch of its own on a side stream, the two heads with the committed parameters and the optimiser."""

    def __init__(self, init):
        import torch

        from collectivecrossing_amd.batched import BatchedCollectiveCrossing

        assert torch.cuda.is_available(), "gpu tests need an MI355X"
        self.env = env = BatchedCollectiveCrossing(chain_config(), PPO["E"])
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
            self.actor = env.mlp_head(H)
            self.critic = env.mlp_head(H, O=1, activation="relu")
            for head, par in zip((self.actor, self.critic), init):
                for t, a in zip((head.w1t, head.b1, head.w2, head.b2), par):
                    t.copy_(torch.from_numpy(a))
            self.opt = env.adam([*self.actor.parameters(), *self.critic.parameters()], lr=ppo_lr(0), weight_decay=PPO["WEIGHT_DECAY"],
                                max_grad_norm=PPO_MB["MAX_GRAD_NORM"])

    def final(self, mb):
        self.side.synchronize()
        opt = self.opt
        return dict(params=[_np(p) for p in opt.params], m=[_np(t) for t in opt.m], v=[_np(t) for t in opt.v],
                    state_bytes=_np(opt.state), mb_state=_np(mb.state))

    def close(self):
        self.env.use_stream(None)
        self.env.close()


def collect(w, compact: bool):
    """The collection of examples/ppo_minibatches.py: ``traj.obs[s]`` is the row BEHIND step s, ``obs0`` the one step 0 acted on."""
    import torch

    from collectivecrossing_amd import SampleResult
    from collectivecrossing_amd.batched import RolloutResult

    env = w.env
    E, K, dev = PPO["E"], PPO["K"], env.device
    traj = env.alloc_rollout(K, want_obs=True, want_compact=compact, want_final=True)
    col = dict(traj=traj, actions=torch.empty((K, E, N), dtype=torch.uint8, device=dev), logp=torch.empty((K, E, N), device=dev),
               masks=torch.empty((K, E, N), dtype=torch.uint8, device=dev))
    col["obs0"], masks = env.observe().clone(), env.action_masks()
    obs = col["obs0"]
    for s in range(K):
        col["masks"][s] = masks
        env.mlp_sample_actions(w.actor, obs, masks, out=SampleResult(col["actions"][s], col["logp"][s], None))
        slab = RolloutResult(**{k: None if t is None else t[s:s + 1] for k, t in vars(traj).items()})
        obs = env.rollout(col["actions"][s:s + 1], auto_reset=True, reset_obs="next", out=slab, want_compact=compact, masks_out=masks).obs[0]
    return col


def values_and_advantages(w, col):
    import torch

    env, traj, critic = w.env, col["traj"], w.critic
    K, E = PPO["K"], PPO["E"]
    values = torch.empty((K, E, N), device=env.device)
    values[0] = critic(col["obs0"]).squeeze(-1)
    values[1:] = critic(traj.obs[:K - 1]).squeeze(-1)
    last_values = critic(traj.obs[K - 1]).squeeze(-1).contiguous()
    reset = (traj.env_flags & EF_RESET) != 0
    final_values = torch.zeros((K, E, N), device=env.device)
    final_values[reset] = critic(traj.final_obs[reset].contiguous()).squeeze(-1)
    gae = env.compute_gae(traj, values, last_values, final_values, gamma=PPO["GAMMA"], lam=PPO["LAM"])
    return dict(values=values, last_values=last_values, final_values=final_values, gae=gae, norm=env.masked_moments(gae.advantages, gae.valid))


def check_inputs(col, va, ref, form):
    """Everything ``set_source`` is given, and what it was made from."""
    traj = col["traj"]
    same(_np(col["obs0"]), ref["rows"][0], "obs0: the rows step 0 acts on")
    same(_np(traj.obs)[:-1], ref["rows"][1:], "the rollout's own obs: the rows behind every step but the last")
    same(_np(traj.obs)[-1], ref["last_rows"], "the rows behind the last step")
    for k in ("masks", "actions", "logp"):
        same(_np(col[k]), ref[k], k)
    for k in ("reward", "agent_flags", "env_flags"):
        same(_np(getattr(traj, k)), ref[k], k)
    if form == "compact":
        same(_np(traj.obs_compact), ref["source"]["obs"], "the rollout's compact records")
    for k in ("values", "last_values", "final_values"):
        same(_np(va[k]), ref[k], k)
    for k in ("advantages", "returns", "valid"):
        same(_np(getattr(va["gae"], k)), ref[k], k)
    same(_np(va["norm"]), ref["norm"], "norm")


def run_updates(w, col, va, ref, form, captured, check):
    """The eight updates of examples/ppo_minibatches.py on static buffers, ``mb.next`` inside: eager, or ONE captured graph
    replayed eight times; the rate changes after the fourth.  ``check``: every link after every step."""
    import torch

    from collectivecrossing_amd import RolloutMinibatches

    env, actor, critic, opt, gae, norm, traj = w.env, w.actor, w.critic, w.opt, va["gae"], va["norm"], col["traj"]
    dev = env.device
    mb = RolloutMinibatches(env, num_steps=PPO["K"], batch_size=PPO_MB["B"])
    obs, obs0 = (traj.obs_compact, compact_of_rows(col["obs0"])) if form == "compact" else (traj.obs, col["obs0"])
    mb.set_source(obs, col["actions"], col["logp"], gae.advantages, gae.returns, masks=col["masks"], valid=gae.valid, obs0=obs0)
    assert mb.minibatches_per_epoch == ref["per_epoch"] == 4
    batch = mb.alloc()
    lead = (mb.batch_size, N)
    logits, hid_a = torch.empty(lead + (5,), device=dev), torch.empty(lead + (H,), device=dev)
    vals, hid_c = torch.empty(lead + (1,), device=dev), torch.empty(lead + (H,), device=dev)
    loss = env.alloc_ppo_loss(lead)
    ga, gc = env.alloc_mlp_backward(actor, lead), env.alloc_mlp_backward(critic, lead)
    grads = [ga.w1t, ga.b1, ga.w2, ga.b2, gc.w1t, gc.b1, gc.w2, gc.b2]

    def update():                                                        # library launches only, the gather included
        mb.next(out=batch)
        actor(batch.obs, out=logits, hidden_out=hid_a)
        critic(batch.obs, out=vals, hidden_out=hid_c)
        args = (logits, vals.squeeze(-1), batch.actions, batch.logp, batch.advantages, batch.returns)
        kw = dict(masks=batch.masks, valid=batch.valid, norm=norm, **PPO["HYPER"])
        env.ppo_loss(*args, **kw, out=loss)
        gl, gv = env.ppo_loss_backward(*args, **kw, stats=loss.stats, out=loss)
        env.mlp_backward(actor, batch.obs, hid_a, gl, out=ga)
        env.mlp_backward(critic, batch.obs, hid_c, gv.unsqueeze(-1), out=gc)
        opt.step(grads=grads)

    step = update
    if captured:
        w.side.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=w.side):
            update()
        step = graph.replay
    for i in range(PPO_MB["EPOCHS"] * mb.minibatches_per_epoch):
        if i == PPO["LR_CHANGE_AFTER"]:
            opt.lr = ppo_lr(i)
        step()
        if check:
            w.side.synchronize()
            same(_np(batch.index), ref["index"][i], f"update {i}: batch.index")
            for k in PPO_MB_KEYS:
                same(_np(getattr(batch, k)), ref["mb"][i][k], f"update {i}: minibatch {k}")
            same(_np(loss.stats), ref["stats"][i], f"update {i}: the loss stats")
            same_lists([_np(g) for g in grads], ref["grads"][i], GRAD_ORDER, f"update {i}: gradient")
            same(_np(opt.stats), ref["adam_stats"][i], f"update {i}: Adam's stats (norm, scale, skipped, rate)")
    got = w.final(mb)
    assert opt.counts() == (8, 0)
    return got


def check_final(got, ref, tag):
    for k in ("params", "m", "v"):
        same_lists(got[k], ref[k], GRAD_ORDER, f"{tag}: {k} after the last step")
    same(got["state_bytes"], ref["state_bytes"], f"{tag}: the optimiser's 64 state bytes")
    same(got["mb_state"], ref["mb_state"], f"{tag}: the minibatch state")
    assert got["mb_state"].tolist() == [PPO_MB["EPOCHS"], 0, 0, 0]


@pytest.mark.parametrize("form", FORMS)
def test_ppo_minibatch_iteration_against_the_reference(refs, form):
    """The captured run ends in the reference's state; its eager twin is checked after every step.  The compact form's final
    parameters are also the rows form's."""
    import torch

    ref = refs[form]
    w, e = World(ref["init"]), World(ref["init"])
    try:
        with torch.cuda.stream(e.side), torch.no_grad():
            col = collect(e, form == "compact")
            va = values_and_advantages(e, col)
            e.side.synchronize()
            check_inputs(col, va, ref, form)
            eager = run_updates(e, col, va, ref, form, captured=False, check=True)
        check_final(eager, ref, f"{form}, eager")
        with torch.cuda.stream(w.side), torch.no_grad():
            col = collect(w, form == "compact")
            captured = run_updates(w, col, values_and_advantages(w, col), ref, form, captured=True, check=False)
        check_final(captured, ref, f"{form}, captured")
        same_lists(captured["params"], refs["rows"]["params"], GRAD_ORDER, f"{form}: the rows form's final parameters")
    finally:
        w.close()
        e.close()
