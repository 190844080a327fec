"""Whole iterations of a categorical (C51) double-DQN with prioritised n-step replay on the CPU, composed from the per-op
specs.  TEST INFRASTRUCTURE ONLY: what tests/test_gpu_c51_chain.py holds the device to, bit for bit, and what
tests/test_c51_chain_reference.py checks for coverage and sensitivity.  NumPy and the CPU oracle only: no torch, nothing of
the library but the lowered config; the helpers of tests/_rainbow_chain.py and tests/_learner_chain.py are imported, not restated.

``c51_reference``: the loop of examples/c51_dqn.py with two deviations.  (1) The network is FIVE device heads ``mlp_head(H, O=A)``
with A = 8 atoms, head k giving the atom logits of action k, online and target alike: the ``[..., 5, A]`` logits are exact
copies of the five outputs, the backward hands ``grad_logits[..., k, :]`` to ``mlp_backward`` of head k, and ONE Adam steps on
the 20 parameter tensors -- so every link is bit-defined and the loop closes.  A = 8 is the device head's limit
(``ccx_mlp::kMaxO``), not a choice about C51: the per-op tests own the atom counts.  (2) The replay is the Rainbow loop's --
``PrioritizedReplay`` over ``NStepReplay`` over a ring -- as the docstrings of ``CategoricalQ.loss`` intend: ``discount``,
``valid`` and ``masks_next`` come from the n-step fetch, ``weights`` from the prioritised draw, and ``row_loss`` goes back into
``update_priorities``.  The environment set-up is the Rainbow loop's too (``chain_config()``, E = 8, a ring of 6 steps, n = 3,
two warm-up steps, the user terminated table, the hand truncation before TRUNC_ROUND, the envs put back with ``mark_cut()``
before EVENT_ROUND, annealed ``epsilon`` and ``beta``, staggered step counters), because the n-step and priority paths only do
interesting things under it.  All N agents share the five heads: one loss over all rows of a minibatch.

An actor step: observe -> five online heads -> ``q_values`` -> ``q_actions`` -> rollout -> push.  An update: the prioritised
draw and n-step fetch; online at ``obs`` (with hidden activations), target at ``next_obs``, online at ``next_obs``; the
categorical loss (double-Q, ``masks_next``, ``valid``, ``weights``, per-row ``discount``) with ``row_loss`` and ``proj``; its
backward; five ``mlp_backward``; Adam; ``update_priorities(index, row_loss)``; every TARGET_EVERY rounds the target copy.
``mutate=`` switches ONE wire to a plausible wrong one (C51_MUTATIONS).

[VMIN, VMAX] = [-3, 4] (dz = 1): under ``chain_config()`` the n-step rewards of the rows that count run from about -3.3 to 5.0
(a step costs about 0.1 to 1.2, an arrival brings 5), so they reach beyond both ends, and a row that ends with ``done`` puts its
whole mass at the position of its reward, which lands exactly on an atom where that reward is 0."""

from __future__ import annotations

import numpy as np
from _adam_spec import adam_step_spec, new_state, state_bytes
from _c51_spec import c51_loss_backward_spec, c51_loss_spec, dist, expected, q_values_spec, support
from _learner_chain import EF_RESET, H, N, SEED, _copy, _masks, _oracle_batch, chain_config, compact_of_rows
from _mlp_backward_spec import NAMES, mlp_backward_spec
from _mlp_spec import TANH, linear_init, mlp_spec
from _nstep_spec import cut_push_spec, mark_cut_spec, new_cut, nstep_fetch_spec
from _prio_spec import new_pstate, push_leaf_spec, update_spec
from _prio_spec import sample_spec as prio_sample_spec
from _qlearn_spec import greedy_spec, legal_bits, q_actions_spec
from _rainbow_chain import MB_KEYS, RAINBOW, RAINBOW_START_STEP_COUNT, hand_truncation, rainbow_beta, rainbow_epsilon, terminated_tables
from _replay_spec import new_ring, push_spec
from _reset_obs_spec import row_consts

F32 = np.float32

# Everything of the Rainbow loop's set-up but the network and the loss.  MAX_GRAD_NORM lies inside the range of the twelve
# gradient norms (printed by tests/test_c51_chain_reference.py).
C51 = dict({k: RAINBOW[k] for k in ("E", "RING_STEPS", "N_STEP", "WARMUP", "ROUNDS", "BATCH", "TARGET_EVERY", "ANNEAL", "EPS", "BETA",
                                    "ALPHA", "PRIO_EPS", "GAMMA", "LR", "EVENT_ROUND", "TRUNC_ROUND")},
           ATOMS=8, VMIN=-3.0, VMAX=4.0, MAX_GRAD_NORM=0.3)
HEADS = 5                                         # one device head per action
C51_INIT_SEEDS = (11, 12, 13, 14, 15)             # linear_init seeds of the five heads
C51_START_STEP_COUNT = RAINBOW_START_STEP_COUNT
C51_GRAD_ORDER = tuple(f"head{k}.{n}" for k in range(HEADS) for n in NAMES)
# what a round leaves behind, in chain order: a comparison that walks them names the first link that differs
C51_LINKS = (("actions", "explored", "index", "weights", "leaf_drawn") + tuple(f"mb.{k}" for k in MB_KEYS)
             + ("logits", "next_target", "next_online", "stats", "row_loss", "proj", "grad_logits")
             + tuple(f"grad.{g}" for g in C51_GRAD_ORDER) + ("adam_stats", "leaf", "pstate", "cut"))
C51_MUTATIONS = ("priorities_never_updated", "priorities_from_weighted_loss", "single_q", "scalar_gamma", "weights_all_one",
                 "masks_of_the_state", "atoms_major", "stale_proj", "acts_on_target", "heads_in_reverse")
C51_DRAW_SIDE_MUTATIONS = ("priorities_never_updated", "priorities_from_weighted_loss", "weights_all_one")


def c51_init():
    """The committed initial parameters: five ``linear_init`` heads (L, H, O = A)."""
    return [linear_init(6 + 4 * N, H, C51["ATOMS"], seed=s) for s in C51_INIT_SEEDS]


def heads_forward(x, heads):
    """(logits f32 [..., 5, A], hidden: five f32 [..., H]) of rows x [..., L]: head k's outputs are the atom logits of action k."""
    flat = x.reshape(-1, x.shape[-1])
    ys, hs = zip(*(mlp_spec(flat, *p, TANH) for p in heads))
    return (np.ascontiguousarray(np.stack(ys, axis=1)).reshape(x.shape[:-1] + (HEADS, ys[0].shape[-1])),
            [h.reshape(x.shape[:-1] + (h.shape[-1],)) for h in hs])


def atoms_major(logits):
    """The wrong reading of the buffer: as [..., A, 5], action = the fast axis."""
    return np.ascontiguousarray(np.swapaxes(logits.reshape(logits.shape[:-2] + logits.shape[:-3:-1]), -1, -2))


def c51_reference(online, mutate=None):
    """The loop from the initial online parameters, a list of five (w1t, b1, w2, b2) with O = A; the target starts as a copy.
    Returns per actor step ``actions`` / ``explored`` (WARMUP + ROUNDS of them), per round ``epsilon``, ``beta`` and
    ``rounds[u]``: a dict of every array of C51_LINKS; the final ``params``, ``target``, ``m``, ``v``, ``state_bytes``,
    ``ring_state``, ``leaf``, ``pstate``, ``cut``; ``facts``."""
    assert mutate is None or mutate in C51_MUTATIONS, mutate
    C = C51
    E, S, B, n, A = C["E"], C["RING_STEPS"], C["BATCH"], C["N_STEP"], C["ATOMS"]
    span = dict(vmin=C["VMIN"], vmax=C["VMAX"])
    config = chain_config()
    oracle, params_c, ob = _oracle_batch(config, E)
    ob.set_state(step_count=C51_START_STEP_COUNT)
    ob.set_user_tables(None, terminated_tables(config))
    consts = row_consts(params_c)
    heads = [_copy(p) for p in online]
    assert len(heads) == HEADS and all(p[2].shape == (A, H) for p in heads)
    target = [_copy(p) for p in heads]
    flat = [p for h in heads for p in h]
    ms, vs, state = [np.zeros_like(p) for p in flat], [np.zeros_like(p) for p in flat], new_state()
    ring, cut = new_ring(S, E, N), new_cut(S, E)
    leaf, pstate = np.zeros(S * E, np.int32), new_pstate()
    masks_state = np.zeros((S * E, N), np.uint8)          # the legal set of the state a record's action was chosen in
    out = dict(actions=[], explored=[], epsilon=[], beta=[], rounds=[], head=[], copies=[], details=[], leaf_before=[])
    obs_c = compact_of_rows(ob.observe())
    last_proj = None

    def actor_step(eps):
        nonlocal obs_c
        rows = ob.observe()
        masks = _masks(oracle, params_c, ob)
        logits, _ = heads_forward(rows, target if mutate == "acts_on_target" else heads)
        acts, explored = q_actions_spec(q_values_spec(logits, **span), masks, ob.terminated, ob.truncated, ob.step_count.copy(),
                                        ob.episode.copy(), seed=SEED, epsilon=F32(eps))
        step_obs, reward, af, ef = ob.rollout(acts[None], auto_reset=True)
        reset = (ef[0] & EF_RESET) != 0
        next_rows = np.where(reset[:, None, None], ob.observe(), step_obs[0])        # reset_obs="next"
        next_c, final_c = compact_of_rows(next_rows), compact_of_rows(step_obs[0])
        masks_next = _masks(oracle, params_c, ob)
        head = int(ring["state"][0])
        masks_state[(head % S) * E:(head % S) * E + E] = masks
        push_spec(ring, obs_c, acts[None], reward, af, ef, next_c[None], final_c[None], masks_next[None])
        cut_push_spec(cut, int(ring["state"][0]), S, E, ef)
        push_leaf_spec(leaf, pstate, head, 1, S, E)
        obs_c = next_c
        out["actions"].append(acts)
        out["explored"].append(explored)

    for _ in range(C["WARMUP"]):
        actor_step(C["EPS"][0])
    for u in range(C["ROUNDS"]):
        if u == C["TRUNC_ROUND"]:                                                    # out of band: a user truncation by hand
            ob.set_state(truncated=hand_truncation(ob.truncated))
        if u == C["EVENT_ROUND"]:                                                    # out of band, between two replays
            ob.reset_from_pool()
            mark_cut_spec(cut, int(ring["state"][0]), S, E)
            obs_c = compact_of_rows(ob.observe())
        eps, beta = float(F32(rainbow_epsilon(u))), float(F32(rainbow_beta(u)))
        actor_step(eps)
        drawn = prio_sample_spec(leaf, pstate, SEED, B, N, beta, stratified=True)
        index = drawn["index"]
        mb = nstep_fetch_spec(ring, cut, index, n, C["GAMMA"], consts)
        logits, hid = heads_forward(mb["obs"], heads)
        nt, _ = heads_forward(mb["next_obs"], target)
        no, _ = heads_forward(mb["next_obs"], heads)
        seen = tuple(atoms_major(a) for a in (logits, nt, no)) if mutate == "atoms_major" else (logits, nt, no)
        weights = np.ones_like(drawn["weights"]) if mutate == "weights_all_one" else drawn["weights"]
        kw = dict(next_online=None if mutate == "single_q" else seen[2],
                  masks_next=masks_state[index] if mutate == "masks_of_the_state" else mb["masks_next"], valid=mb["valid"],
                  weights=weights, **span)
        kw.update(dict(gamma=C["GAMMA"]) if mutate == "scalar_gamma" else dict(discount=mb["discount"]))
        stats, row_loss, proj, det = c51_loss_spec(seen[0], mb["actions"], mb["reward"], mb["done"], seen[1], **kw, details=True)
        row_loss, proj = row_loss.reshape(B, N), proj.reshape(B, N, A)
        given = last_proj if mutate == "stale_proj" and last_proj is not None else proj
        last_proj = proj
        gl = c51_loss_backward_spec(seen[0], mb["actions"], given, mb["valid"], weights, stats).reshape(B, N, HEADS, A)
        x = mb["obs"].reshape(B * N, -1)
        grads = []
        for k, p in enumerate(heads):
            gk = np.ascontiguousarray(gl[:, :, HEADS - 1 - k if mutate == "heads_in_reverse" else k]).reshape(B * N, A)
            g = mlp_backward_spec(x, hid[k].reshape(B * N, H), gk, p[2], TANH)
            grads += [g[name] for name in NAMES]
        adam_stats = adam_step_spec(flat, grads, ms, vs, state, C["LR"], max_grad_norm=C["MAX_GRAD_NORM"])
        out["leaf_before"].append((leaf.copy(), int(pstate[0])))
        if mutate != "priorities_never_updated":
            td = (row_loss * weights).astype(F32) if mutate == "priorities_from_weighted_loss" else row_loss
            update_spec(leaf, pstate, index, td, C["ALPHA"], C["PRIO_EPS"])
        copied = (u + 1) % C["TARGET_EVERY"] == 0
        if copied:
            target = [_copy(p) for p in heads]
        rnd = dict(actions=out["actions"][-1], explored=out["explored"][-1], index=index, weights=drawn["weights"],
                   leaf_drawn=drawn["leaf_drawn"], logits=logits, next_target=nt, next_online=no, stats=stats, row_loss=row_loss,
                   proj=proj, grad_logits=gl, adam_stats=adam_stats, leaf=leaf.copy(), pstate=pstate.copy(), cut=cut.copy())
        rnd.update({f"mb.{k}": mb[k] for k in MB_KEYS})
        rnd.update({f"grad.{g}": a for g, a in zip(C51_GRAD_ORDER, grads)})
        assert set(rnd) == set(C51_LINKS)
        for k, v in (("epsilon", eps), ("beta", beta), ("rounds", rnd), ("head", int(ring["state"][0])), ("copies", copied),
                     ("details", det)):
            out[k].append(v)
    out.update(params=_copy(flat), target=[np.array(p, copy=True) for h in target for p in h], m=_copy(ms), v=_copy(vs),
               state_bytes=state_bytes(state), ring_state=ring["state"].copy(), leaf=leaf.copy(), pstate=pstate.copy(), cut=cut.copy())
    out["facts"] = c51_facts(out) if mutate is None else None
    return out


def c51_facts(r) -> dict:
    """What the run exercised, per round unless said otherwise: the conditions ``assert_c51_coverage`` asserts."""
    C = C51
    A, n, w = C["ATOMS"], C["N_STEP"], C["WARMUP"]
    dz, z, top = support(A, C["VMIN"], C["VMAX"])
    vmin, vmax = F32(C["VMIN"]), F32(C["VMAX"])
    f = {k: [] for k in ("counting", "not_counting", "done", "bootstrapped", "span_short", "span_full", "discounts", "distinct_weights",
                         "reward_above_vmax", "reward_below_vmin", "atom_clamped_at_vmax", "atom_clamped_at_vmin", "on_an_atom_inside",
                         "double_q_differs", "unmasked_argmax_illegal", "leaves_above_max_leaf", "leaves_below_max_leaf")}
    for rnd, t, (leaf_before, max_leaf) in zip(r["rounds"], r["details"], r["leaf_before"]):
        c, cut = t["counts"], t["cut"]
        boot = c & ~cut
        reward = rnd["mb.reward"].reshape(-1).astype(F32)
        disc, sp = rnd["mb.discount"].reshape(-1), rnd["mb.span"].reshape(-1)
        lo = np.where(cut, reward, (reward + (disc * z[0]).astype(F32)).astype(F32))
        hi = np.where(cut, reward, (reward + (disc * z[A - 1]).astype(F32)).astype(F32))
        mass = t["p"][:, :A] != 0
        b = t["b"][:, :A]
        legal = legal_bits(rnd["mb.masks_next"], (len(c),))
        e, s = dist(rnd["next_target"].reshape(-1, 5, A), A)[1:]
        by_target = greedy_spec(expected(e, s, z, A), legal)
        unmasked = greedy_spec(t["qsel"], np.ones_like(legal))
        named = np.unique(rnd["index"][rnd["index"] >= 0])
        written = rnd["leaf"][named].astype(np.int64)
        for k, v in (("counting", c.sum()), ("not_counting", (~c).sum()), ("done", (c & (rnd["mb.done"].reshape(-1) != 0)).sum()),
                     ("bootstrapped", boot.sum()), ("span_short", (c & (sp < n)).sum()), ("span_full", (c & (sp == n)).sum()),
                     ("distinct_weights", len(np.unique(rnd["weights"]))),
                     ("reward_above_vmax", (c & (reward > vmax)).sum()), ("reward_below_vmin", (c & (reward < vmin)).sum()),
                     ("atom_clamped_at_vmax", (c & (hi > vmax)).sum()), ("atom_clamped_at_vmin", (c & (lo < vmin)).sum()),
                     ("on_an_atom_inside", (c & (mass & (b == np.floor(b)) & (b > 0) & (b < top)).any(-1)).sum()),
                     ("double_q_differs", (boot & (by_target != t["kstar"])).sum()),
                     ("unmasked_argmax_illegal", (boot & ~legal[np.arange(len(c)), unmasked]).sum()),
                     ("leaves_above_max_leaf", (written > max_leaf).sum()), ("leaves_below_max_leaf", (written < max_leaf).sum())):
            f[k].append(int(v))
        f["discounts"].append(sorted({float(d) for d in disc[c]}))
    live = [a != 255 for a in r["actions"][w:]]
    f.update(explored=[int(e.sum()) for e in r["explored"][w:]],
             greedy=[int((l & (e == 0)).sum()) for l, e in zip(live, r["explored"][w:])],
             ring_heads=r["head"], ring_steps=C["RING_STEPS"], copies=r["copies"], epsilons=r["epsilon"], betas=r["beta"],
             adam_norms=[float(x["adam_stats"][0]) for x in r["rounds"]], adam_scales=[float(x["adam_stats"][1]) for x in r["rounds"]],
             adam_skipped=[float(x["adam_stats"][2]) for x in r["rounds"]],
             losses=[float(x["stats"][0]) for x in r["rounds"]], bad_actions=[float(x["stats"][7]) for x in r["rounds"]])
    return f


def assert_c51_coverage(r) -> None:
    f, rounds = r["facts"], C51["ROUNDS"]
    assert all(c > 0 for c in f["counting"]) and all(c > 0 for c in f["not_counting"]), f      # in EVERY minibatch
    assert sum(f["done"]) > 0 and all(c > 0 for c in f["bootstrapped"]), f
    assert sum(f["span_short"]) > 0 and sum(f["span_full"]) > 0, f
    assert len({d for ds in f["discounts"] for d in ds}) >= 2, f
    assert any(d > 1 for d in f["distinct_weights"]), f
    assert sum(f["reward_above_vmax"]) > 0 and sum(f["reward_below_vmin"]) > 0, f              # the reward alone, whatever follows
    assert sum(f["atom_clamped_at_vmax"]) > 0 and sum(f["atom_clamped_at_vmin"]) > 0, f
    assert sum(f["on_an_atom_inside"]) > 0, f                                                  # not merely by a clamp
    assert sum(f["double_q_differs"][2:]) > 0 and sum(f["unmasked_argmax_illegal"]) > 0, f
    assert all(e > 0 for e in f["explored"]) and all(g > 0 for g in f["greedy"]), f
    assert sum(f["leaves_above_max_leaf"]) > 0 and sum(f["leaves_below_max_leaf"]) > 0, f
    assert any(s < 1.0 for s in f["adam_scales"]) and any(s == 1.0 for s in f["adam_scales"]) and not any(f["adam_skipped"]), f
    assert max(f["ring_heads"]) > f["ring_steps"], f                                           # the head passes the capacity
    assert len(set(f["epsilons"])) == rounds and len(set(f["betas"])) == rounds and not any(f["bad_actions"]), f
    assert any(f["copies"][:-2]) and np.isfinite(f["losses"]).all(), f
