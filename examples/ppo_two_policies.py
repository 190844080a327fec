#!/usr/bin/env python3
"""The iteration of ppo_device_update.py with the two policies the reference's training script trains -- "boarding" and
"exiting", each with its own actor and critic (include/ccx.h: CCX_SIDES).  The actor loop is `actors.sample_actions` ->
`rollout`: ONE launch for both networks, on the observation rows as the rollout wrote them.  The loss is per side:
`ppo_loss` once per side with `valid & side` (the side is a u8 [N] mask broadcast in torch), normalised by that side's
`masked_moments`; rows of the other side get exactly +0.0 gradients by `ppo_loss`'s own selection rule, so the two gradient
arrays are joined by a select.  ONE `DeviceAdam` holds all sixteen tensors (one global gradient norm, one clip for both
sides; two optimisers would clip each side on its own).  A minibatch update is ONE captured graph, replayed EPOCHS x
MINIBATCHES times on static buffers.  Before the first optimiser step the whole [K, E, N, L] batch is re-evaluated:
approx_kl and clip_frac are exactly 0 for both sides.  The whole iteration runs twice from the same seeds; the parameters
and the optimiser's m and v are equal bit for bit."""

import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

import torch  # noqa: E402

from collectivecrossing_amd import BatchedCollectiveCrossing, CollectiveCrossingConfig, SampleResult, SideHeads  # noqa: E402
from collectivecrossing_amd._abi import EF_RESET  # noqa: E402
from collectivecrossing_amd.batched import RolloutResult  # noqa: E402
from collectivecrossing_amd.truncated_configs import MaxStepsTruncatedConfig  # noqa: E402

config = CollectiveCrossingConfig(
    width=12, height=8, division_y=4, tram_door_left=5, tram_door_right=7, tram_length=9,
    num_boarding_agents=5, num_exiting_agents=3, exiting_destination_area_y=0,
    boarding_destination_area_y=8, truncated_config=MaxStepsTruncatedConfig(max_steps=40))
E, K, EPOCHS, MINIBATCHES = 1024, 64, 3, 4
HYPER = dict(clip=0.2, vf_coef=0.5, ent_coef=0.01)
SIDES = ("boarding", "exiting")


def iteration():
    """One PPO iteration from fixed seeds; returns (parameters, m, v), the last stats per side, the optimiser's counts and
    (approx_kl, clip_frac) per side before the first step."""
    env = BatchedCollectiveCrossing(config, E)
    stream = torch.cuda.Stream()
    env.use_stream(stream)                                           # a capture needs a stream of its own
    torch.cuda.synchronize()
    with torch.cuda.stream(stream), torch.no_grad():
        env.make_reset_pool(seed0=0, size=4096)
        env.reset_from_pool()
        env.set_rng_seed(2024)
        N, L, dev = env.num_agents, env.obs_len, env.device
        torch.manual_seed(0)
        actors = SideHeads(env, {s: env.mlp_head(64) for s in SIDES})
        critics = SideHeads(env, {s: env.mlp_head(64, O=1) for s in SIDES})
        opt = env.adam([*actors.parameters(), *critics.parameters()], lr=3e-4, max_grad_norm=0.5)
        side_of = [actors.slot_mask(i) for i in range(len(SIDES))]    # u8 [N] each

        # ---- collect: both policies in one launch per step
        traj = env.alloc_rollout(K, want_final=True)
        acts = torch.empty((K, E, N), dtype=torch.uint8, device=dev)
        logp_old = torch.empty((K, E, N), device=dev)
        masks_old = torch.empty((K, E, N), dtype=torch.uint8, device=dev)
        rows = torch.empty((K, E, N, L), device=dev)
        obs, masks = env.observe(), env.action_masks()
        for s in range(K):
            rows[s] = obs
            masks_old[s] = masks
            actors.sample_actions(obs, masks, out=SampleResult(acts[s], logp_old[s], None))
            slab = RolloutResult(**{k: None if t is None else t[s:s + 1] for k, t in vars(traj).items()})
            obs = env.rollout(acts[s:s + 1], auto_reset=True, reset_obs="next", out=slab, masks_out=masks).obs[0]

        # ---- values and advantages
        values = critics(rows).squeeze(-1).contiguous()
        last_values = critics(traj.obs[K - 1]).squeeze(-1).contiguous()
        reset = (traj.env_flags & EF_RESET) != 0
        final_values = torch.zeros((K, E, N), device=dev)
        final_values[reset] = critics(traj.final_obs[reset].contiguous()).squeeze(-1)
        gae = env.compute_gae(traj, values, last_values, final_values, gamma=0.99, lam=0.95)
        valid_of = [(gae.valid * m).contiguous() for m in side_of]    # valid & side, u8 [K, E, N]
        norm_of = [env.masked_moments(gae.advantages, v) for v in valid_of]

        # ---- before the first step: the stored logp is reproduced bit for bit, for both sides
        logits_all = actors(rows)                                    # ONE call on [K, E, N, L]
        before = []
        for v, nm in zip(valid_of, norm_of):
            st = env.ppo_loss(logits_all, values, acts, logp_old, gae.advantages, gae.returns, masks=masks_old, valid=v, norm=nm,
                              **HYPER).stats
            before.append((float(st[4]), float(st[5])))

        # ---- the update's static buffers: a minibatch of whole steps, [K / MINIBATCHES, E, N, ...]
        lead = (K // MINIBATCHES, E, N)
        source = dict(obs=rows, acts=acts, logp=logp_old, adv=gae.advantages, ret=gae.returns, masks=masks_old,
                      valid0=valid_of[0], valid1=valid_of[1])
        mb = {k: torch.empty((lead[0],) + tuple(t.shape[1:]), dtype=t.dtype, device=dev) for k, t in source.items()}
        logits, hid_a = torch.empty(lead + (5,), device=dev), torch.empty(lead + (64,), device=dev)
        vals, hid_c = torch.empty(lead + (1,), device=dev), torch.empty(lead + (64,), device=dev)
        losses = [env.alloc_ppo_loss(lead) for _ in SIDES]
        gl, gv = torch.empty(lead + (5,), device=dev), torch.empty(lead, device=dev)
        first_side = side_of[0].bool()
        ga, gc = actors.alloc_backward(lead), critics.alloc_backward(lead)
        grads = [t for o in ga + gc for t in (o.w1t, o.b1, o.w2, o.b2)]

        def update():
            actors(mb["obs"], out=logits, hidden_out=hid_a)
            critics(mb["obs"], out=vals, hidden_out=hid_c)
            args = (logits, vals.squeeze(-1), mb["acts"], mb["logp"], mb["adv"], mb["ret"])
            parts = []
            for i, loss in enumerate(losses):                        # per side: its rows, its normalisation
                kw = dict(masks=mb["masks"], valid=mb[f"valid{i}"], norm=norm_of[i], **HYPER)
                env.ppo_loss(*args, **kw, out=loss)
                parts.append(env.ppo_loss_backward(*args, **kw, stats=loss.stats, out=loss))
            torch.where(first_side[:, None], parts[0][0], parts[1][0], out=gl)   # a select: each side keeps its own bits
            torch.where(first_side, parts[0][1], parts[1][1], out=gv)
            actors.backward_into(mb["obs"], hid_a, gl, out=ga)
            critics.backward_into(mb["obs"], hid_c, gv.unsqueeze(-1), out=gc)
            opt.step(grads=grads)

        stream.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=stream):
            update()

        # ---- the update: per minibatch a gather into the static buffers, then ONE replay
        for epoch in range(EPOCHS):
            for steps in torch.randperm(K, device=dev).chunk(MINIBATCHES):
                for k, t in source.items():
                    torch.index_select(t, 0, steps, out=mb[k])
                graph.replay()
        stream.synchronize()
        out = ([p.detach().clone() for p in opt.params], [t.clone() for t in opt.m], [t.clone() for t in opt.v])
        stats, counts = [loss.stats.tolist() for loss in losses], opt.counts()
    env.use_stream(None)
    env.close()
    return out, stats, counts, before


first, stats, counts, before = iteration()
second, _, _, before2 = iteration()
for side, (kl, cf) in zip(SIDES, before):
    print(f"before the first optimiser step, {side}: approx_kl {kl!r}, clip_frac {cf!r} over the whole [K, E, N] batch")
    assert kl == 0.0 and cf == 0.0, "the re-evaluated logits must reproduce the stored logp bit for bit"
for side, (loss, policy, value, entropy, kl, cf, n, _) in zip(SIDES, stats):
    print(f"{side}, last minibatch of {EPOCHS} epochs x {MINIBATCHES} minibatches (each ONE replayed graph): loss {loss:.4f} (policy "
          f"{policy:.4f}, value {value:.4f}, entropy {entropy:.4f}, approx_kl {kl:.5f}, clip_frac {cf:.3f}, {int(n)} agent-steps)")
print(f"optimiser steps on the device: {counts[0]} taken, {counts[1]} skipped")
assert counts == (EPOCHS * MINIBATCHES, 0) and before == before2
assert all(torch.isfinite(t).all() for group in first for t in group)
for name, a, b in zip(("parameters", "m", "v"), first, second):
    same = all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(a, b))
    print(f"two runs from the same seeds: the {sum(t.numel() for t in a)} values of {name} are {'equal bit for bit' if same else 'DIFFERENT'}")
    assert same, "the update is pinned by its seeds, the optimiser step included"
