#!/usr/bin/env python3
"""The iteration of ppo_device_update.py with the network the usual PPO baseline trains: a `64-64 tanh` actor and critic
(include/ccx.h: CCX_MLP_DEEP, `DeepMlpHead`).  The actor step is ONE launch (`head.sample_actions`), and a minibatch update is
ONE captured graph made of library launches only -- both heads' forward with both hiddens, `ppo_loss`, `ppo_loss_backward`,
two `param_grads(out=)` and one `opt.step(grads=)` over the twelve tensors.  Before the first optimiser step the stored rows
are re-evaluated as one `[K, E, N, L]` batch: the new log-probabilities equal the sampler's bit for bit, so the printed
maximum of |logp_new - logp_old| is 0 and the first ratio is exactly 1.  The whole iteration runs twice from the same
seeds; the parameters and the optimiser's m and v are equal bit for bit."""

import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

import torch  # noqa: E402

from collectivecrossing_amd import BatchedCollectiveCrossing, CollectiveCrossingConfig, DeepMlpHead, DeviceAdam, SampleResult  # noqa: E402
from collectivecrossing_amd._abi import EF_RESET  # noqa: E402
from collectivecrossing_amd.batched import RolloutResult  # noqa: E402
from collectivecrossing_amd.truncated_configs import MaxStepsTruncatedConfig  # noqa: E402

config = CollectiveCrossingConfig(
    width=12, height=8, division_y=4, tram_door_left=5, tram_door_right=7, tram_length=9,
    num_boarding_agents=5, num_exiting_agents=3, exiting_destination_area_y=0,
    boarding_destination_area_y=8, truncated_config=MaxStepsTruncatedConfig(max_steps=40))
EPOCHS, MINIBATCHES = 3, 4
HYPER = dict(clip=0.2, vf_coef=0.5, ent_coef=0.01)


def iteration(E, K):
    """One PPO iteration from fixed seeds; returns (parameters, m, v) of actor and critic, the last stats, the optimiser's
    counts and the maximum of |logp_new - logp_old| over the agent-steps that count, before the first step."""
    env = BatchedCollectiveCrossing(config, E)
    side = torch.cuda.Stream()
    env.use_stream(side)                                             # a capture needs a stream of its own
    torch.cuda.synchronize()
    with torch.cuda.stream(side), torch.no_grad():
        env.make_reset_pool(seed0=0, size=4096)
        env.reset_from_pool()
        env.set_rng_seed(2024)
        N, L = env.num_agents, env.obs_len
        torch.manual_seed(0)
        actor = DeepMlpHead(env, 64, 64)
        critic = DeepMlpHead(env, 64, 64, O=1)
        opt = DeviceAdam(env, [*actor.parameters(), *critic.parameters()], lr=3e-4, max_grad_norm=0.5)

        # ---- collect: one launch from the observation rows to the actions
        traj = env.alloc_rollout(K, want_final=True)
        acts = torch.empty((K, E, N), dtype=torch.uint8, device=env.device)
        logp_old = torch.empty((K, E, N), device=env.device)
        masks_old = torch.empty((K, E, N), dtype=torch.uint8, device=env.device)
        rows = torch.empty((K, E, N, L), device=env.device)
        obs, masks = env.observe(), env.action_masks()
        for s in range(K):
            rows[s] = obs
            masks_old[s] = masks
            actor.sample_actions(obs, masks, out=SampleResult(acts[s], logp_old[s], None))
            slab = RolloutResult(**{k: None if t is None else t[s:s + 1] for k, t in vars(traj).items()})
            obs = env.rollout(acts[s:s + 1], auto_reset=True, reset_obs="next", out=slab, masks_out=masks).obs[0]

        # ---- values and advantages
        values = critic(rows).squeeze(-1).contiguous()
        last_values = critic(traj.obs[K - 1]).squeeze(-1).contiguous()
        reset = (traj.env_flags & EF_RESET) != 0
        final_values = torch.zeros((K, E, N), device=env.device)
        final_values[reset] = critic(traj.final_obs[reset].contiguous()).squeeze(-1)
        gae = env.compute_gae(traj, values, last_values, final_values, gamma=0.99, lam=0.95)
        norm = env.masked_moments(gae.advantages, gae.valid)

        # ---- the stored rows under the same parameters, as ONE batch of another shape: the same bits
        logp_new = env.evaluate_actions(actor(rows), acts, masks_old, want_entropy=False).logp
        gap = float((logp_new - logp_old)[gae.valid != 0].abs().max())

        # ---- the update's static buffers: a minibatch of whole steps, [K / MINIBATCHES, E, N, ...]
        lead = (K // MINIBATCHES, E, N)
        source = dict(obs=rows, acts=acts, logp=logp_old, adv=gae.advantages, ret=gae.returns, masks=masks_old, valid=gae.valid)
        mb = {k: torch.empty((lead[0],) + tuple(t.shape[1:]), dtype=t.dtype, device=env.device) for k, t in source.items()}
        new = lambda n: torch.empty(lead + (n,), device=env.device)  # noqa: E731
        logits, a1, a2, vals, c1, c2 = new(5), new(64), new(64), new(1), new(64), new(64)
        loss = env.alloc_ppo_loss(lead)
        ga, gc = actor.alloc_param_grads(lead), critic.alloc_param_grads(lead)
        grads = [*ga.grads(), *gc.grads()]

        def update():                                                # library launches only
            actor(mb["obs"], out=logits, hidden1_out=a1, hidden2_out=a2)
            critic(mb["obs"], out=vals, hidden1_out=c1, hidden2_out=c2)
            args = (logits, vals.squeeze(-1), mb["acts"], mb["logp"], mb["adv"], mb["ret"])
            kw = dict(masks=mb["masks"], valid=mb["valid"], norm=norm, **HYPER)
            env.ppo_loss(*args, **kw, out=loss)
            gl, gv = env.ppo_loss_backward(*args, **kw, stats=loss.stats, out=loss)
            actor.param_grads(mb["obs"], a1, a2, gl, out=ga)
            critic.param_grads(mb["obs"], c1, c2, gv.unsqueeze(-1), out=gc)
            opt.step(grads=grads)

        side.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            update()

        # ---- the update: per minibatch a gather into the static buffers, then ONE replay
        for epoch in range(EPOCHS):
            for steps in torch.randperm(K, device=env.device).chunk(MINIBATCHES):
                for k, t in source.items():
                    torch.index_select(t, 0, steps, out=mb[k])
                graph.replay()
        side.synchronize()
        out = ([p.detach().clone() for p in opt.params], [t.clone() for t in opt.m], [t.clone() for t in opt.v])
        stats, counts = loss.stats.tolist(), opt.counts()
    env.use_stream(None)
    env.close()
    return out, stats, counts, gap


def main(num_envs=1024, iterations=2, steps=64):
    """Runs the iteration ``iterations`` times from the same seeds; returns (the gap of the first run, whether every run
    left the same bits)."""
    runs = [iteration(num_envs, steps) for _ in range(iterations)]
    first, stats, counts, gap = runs[0]
    loss, policy, value, entropy, kl, cf, n, _ = stats
    print(f"64-64 tanh actor and critic, {num_envs} envs x {steps} steps: max |logp_new - logp_old| before the first optimiser step = {gap}")
    print(f"after {EPOCHS} epochs x {MINIBATCHES} minibatches, each ONE replayed graph: loss {loss:.4f} (policy {policy:.4f}, value {value:.4f}, "
          f"entropy {entropy:.4f}, approx_kl {kl:.5f}, clip_frac {cf:.3f}, {int(n)} agent-steps in the last minibatch)")
    assert gap == 0.0 and counts[0] + counts[1] == EPOCHS * MINIBATCHES
    assert all(torch.isfinite(t).all() for group in first for t in group)
    equal = True
    for other in runs[1:]:
        for name, a, b in zip(("parameters", "m", "v"), first, other[0]):
            same = all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(a, b))
            print(f"two runs from the same seeds: the {sum(t.numel() for t in a)} values of {name} are {'equal bit for bit' if same else 'DIFFERENT'}")
            equal = equal and same
    assert equal, "the update is pinned by its seeds, the optimiser step included"
    return gap, equal


if __name__ == "__main__":
    main()
