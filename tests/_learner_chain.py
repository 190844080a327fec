"""Whole learner iterations on the CPU, composed from the per-op specs.  TEST INFRASTRUCTURE ONLY: what
tests/test_gpu_learner_chain.py holds the device to, bit for bit, and what tests/test_learner_chain_reference.py checks for
coverage.  NumPy and the CPU oracle only: no torch, nothing of the library but the lowered config.

``ppo_reference``: one PPO iteration -- collection with a real actor network across auto-resets (``reset_obs="next"``), the
critic's values, GAE with ``final_values``, the advantage moments, and EPOCHS x MINIBATCHES updates through loss, backward and
Adam, the parameters fed back from step to step.  ``dqn_reference``: the loop of examples/dqn_replay_ring.py -- per-side
heads, epsilon-greedy actions, the replay ring, double-DQN TD loss per side, Adam, the target copy.  Each link is the spec
its own test file compares the device with; nothing is restated here but the wiring.  Both return every intermediate array,
the final state and ``facts``: what the run exercised (the coverage conditions of tests/test_learner_chain_reference.py)."""

from __future__ import annotations

import numpy as np
from _action_masks import spec_masks
from _adam_spec import adam_step_spec, new_state, state_bytes
from _gae_spec import gae_spec
from _mlp_backward_spec import NAMES, mlp_backward_spec
from _mlp_spec import RELU, TANH, mlp_spec
from _ppo_loss_spec import masked_moments_spec, ppo_loss_backward_spec, ppo_loss_spec
from _qlearn_spec import q_actions_spec, td_loss_backward_spec, td_loss_spec
from _replay_spec import fetch_spec, filled_spec, new_ring, push_spec, sample_index_spec
from _reset_obs_spec import make_config, row_consts
from _sample_spec import sample_spec

F32 = np.float32
EF_RESET = 0x04
AF_TERMINATED, AF_TRUNCATED, AF_LIVE = 0x01, 0x02, 0x04
SEED = 0x0123_4567_89AB_CDEF                      # set_rng_seed on both sides
N, H = 8, 16
POOL_SEED0, POOL_SIZE = 5, 64


def chain_config():
    """The N = 8 config of the actor-loop tests (tests/test_gpu_sample.py, tests/test_gpu_qlearn.py): 12 x 8 cells, five
    boarding and three exiting agents, individual termination, truncation after 12 steps."""
    return make_config(N, max_steps=12)


# The PPO iteration.  E envs, K steps; a minibatch is K / MINIBATCHES = 6 whole steps = 6 * 12 * 8 = 576 rows: two full
# 256-row blocks and a tail of 64, so mlp_backward's block chains and the tree's final step are both in play.
# START_STEP_COUNT staggers the envs' step counters before the first step (``set_state(step_count=)`` on both sides): with
# max_steps = 12 every env would otherwise be truncated in the same two steps, and no step would restart only SOME envs.
# MAX_GRAD_NORM and the seeds were chosen on the CPU so that the coverage conditions of
# tests/test_learner_chain_reference.py hold for ``linear_init`` parameters (PPO_INIT_SEEDS) and for the GPU test's
# torch-initialised heads (TORCH_SEED): the gradient norms of the eight steps lie between 4.9 and 9.5 for both, so 6.3
# clips at least three of the steps and leaves at least three alone.
PPO = dict(E=12, K=24, EPOCHS=2, MINIBATCHES=4, GAMMA=0.99, LAM=0.95, PERM_SEED=7, LR=(3e-3, 1e-3), LR_CHANGE_AFTER=4,
           WEIGHT_DECAY=0.01, MAX_GRAD_NORM=6.3, HYPER=dict(clip=0.2, vf_coef=0.5, ent_coef=0.01))
PPO_INIT_SEEDS = (30, 31)                         # linear_init seeds of actor and critic
DQN_INIT_SEEDS = (3, 4)                           # linear_init seeds of the boarding and the exiting head
TORCH_SEED = 20                                   # torch.manual_seed before the GPU tests make their heads
START_STEP_COUNT = np.arange(PPO["E"], dtype=np.int32) % 5
GRAD_ORDER = tuple(f"{head}.{name}" for head in ("actor", "critic") for name in NAMES)

# The DQN loop.  A ring of 4 steps of E = 8 envs: 2 warm-up steps and a push before each update, so the first minibatch is
# drawn from 3 of the 4 steps, the second from a full ring, and from the third round on the ring has wrapped.  40 env-steps a minibatch: 320 rows per forward, more than one
# 256-row block; 200 and 120 gathered rows per side.  The envs' step counters start staggered (DQN_START_STEP_COUNT, as for PPO), so
# records that end an episode (``final_compact``, masks 0x1F) are pushed and drawn in most rounds.
DQN = dict(E=8, RING_STEPS=4, WARMUP=2, ROUNDS=10, BATCH=40, TARGET_EVERY=4, ANNEAL=12, EPS=(0.9, 0.05), GAMMA=0.99,
           HUBER_DELTA=1.0, LR=1e-3, MAX_GRAD_NORM=2.3)
DQN_START_STEP_COUNT = (np.arange(DQN["E"], dtype=np.int32) % 4) * 3
SIDES = ("boarding", "exiting")


def dqn_epsilon(u: int) -> float:
    """The rate of round u: the formula of examples/dqn_replay_ring.py."""
    start, end = DQN["EPS"]
    return max(end, start - (start - end) * u / max(1, DQN["ANNEAL"]))


def ppo_minibatches():
    """EPOCHS x MINIBATCHES int64 arrays of step indices: a permutation of the K steps per epoch from NumPy's generator,
    handed to both sides."""
    rng = np.random.default_rng(PPO["PERM_SEED"])
    out = []
    for _ in range(PPO["EPOCHS"]):
        out += [np.ascontiguousarray(c, np.int64) for c in np.split(rng.permutation(PPO["K"]), PPO["MINIBATCHES"])]
    return out


def ppo_lr(step: int) -> float:
    """The rate in force at optimiser step ``step`` (0-based)."""
    return PPO["LR"][0] if step < PPO["LR_CHANGE_AFTER"] else PPO["LR"][1]


def _oracle_batch(config, E):
    from oracle import oracle

    from collectivecrossing_amd.params import lower_config

    params = lower_config(config)
    ob = oracle.OracleBatch(params, E)
    ob.set_reset_pool(oracle.seeded_placements(params, np.arange(POOL_SEED0, POOL_SEED0 + POOL_SIZE, dtype=np.uint64)))
    ob.reset_from_pool()
    return oracle, params, ob


def _masks(oracle, params, ob):
    return spec_masks(oracle, params, ob.x, ob.y, ob.active, ob.terminated, ob.truncated)


def _head(x, p, activation):
    """(y [..., O], hidden [..., H]) of rows x [..., L] under the parameters p = (w1t, b1, w2, b2)."""
    y, h = mlp_spec(x.reshape(-1, x.shape[-1]), *p, activation)
    return y.reshape(x.shape[:-1] + (y.shape[-1],)), h.reshape(x.shape[:-1] + (h.shape[-1],))


def _copy(params):
    return [np.array(p, F32, copy=True) for p in params]


# ---------------------------------------------------------------------------------------------------------------------
# PPO
# ---------------------------------------------------------------------------------------------------------------------
def ppo_collect(actor):
    """The K steps: dict of [K, ...] arrays (rows, masks, actions, logp, reward, agent_flags, env_flags, final_obs, the draw
    key's step_count / episode) and ``last_rows`` [E, N, L], the rows behind the last step."""
    E, K = PPO["E"], PPO["K"]
    oracle, params, ob = _oracle_batch(chain_config(), E)
    ob.set_state(step_count=START_STEP_COUNT)
    rows = ob.observe()
    hist = {k: [] for k in ("rows", "masks", "actions", "logp", "reward", "agent_flags", "env_flags", "final_obs", "step_count",
                            "episode")}
    for _ in range(K):
        masks = _masks(oracle, params, ob)
        logits, _ = _head(rows, actor, TANH)
        step_count, episode = ob.step_count.copy(), ob.episode.copy()
        acts, logp, _ = sample_spec(logits, masks, ob.terminated, ob.truncated, step_count, episode, seed=SEED)
        step_obs, reward, af, ef = ob.rollout(acts[None], auto_reset=True)
        reset = (ef[0] & EF_RESET) != 0
        for k, v in (("rows", rows), ("masks", masks), ("actions", acts), ("logp", logp), ("reward", reward[0]),
                     ("agent_flags", af[0]), ("env_flags", ef[0]), ("final_obs", step_obs[0]), ("step_count", step_count),
                     ("episode", episode)):
            hist[k].append(v)
        rows = np.where(reset[:, None, None], ob.observe(), step_obs[0])             # reset_obs="next"
    out = {k: np.stack(v) for k, v in hist.items()}
    out["last_rows"] = rows
    return out


def ppo_values(col, critic):
    """values [K, E, N] on the rows the steps acted on, last_values [E, N] on the rows behind the last step, final_values
    [K, E, N]: the critic on ``final_obs`` at EF_RESET envs, +0.0 elsewhere."""
    values = _head(col["rows"], critic, RELU)[0][..., 0]
    last_values = _head(col["last_rows"], critic, RELU)[0][..., 0]
    reset = (col["env_flags"] & EF_RESET) != 0
    final_values = np.where(reset[..., None], _head(col["final_obs"], critic, RELU)[0][..., 0], F32(0.0)).astype(F32)
    return values, last_values, final_values


def ppo_update_gradients(x, mb, actor, critic, norm):
    """One minibatch's loss and gradients under the current parameters: (stats f32 [8], the eight gradients in GRAD_ORDER,
    grad_logits, grad_values)."""
    M = x.shape[0]
    logits, hid_a = mlp_spec(x, *actor, TANH)
    vals, hid_c = mlp_spec(x, *critic, RELU)
    flat = {k: mb[k].reshape(M) for k in ("actions", "logp", "advantages", "returns", "masks", "valid")}
    args = (logits, vals[:, 0], flat["actions"], flat["logp"], flat["advantages"], flat["returns"], flat["masks"], flat["valid"],
            norm[1:3])                                                               # masked_moments' [4] is (n, mean, std, 0)
    stats = ppo_loss_spec(*args, **PPO["HYPER"])
    gl, gv = ppo_loss_backward_spec(*args, **PPO["HYPER"], stats=stats)
    ga = mlp_backward_spec(x, hid_a, gl, actor[2], TANH)
    gc = mlp_backward_spec(x, hid_c, gv[:, None], critic[2], RELU)
    return stats, [ga[k] for k in NAMES] + [gc[k] for k in NAMES], gl, gv


def ppo_reference(actor, critic):
    """One PPO iteration from the initial parameters ``actor`` / ``critic`` = (w1t, b1, w2, b2) each.  Returns a dict:
    the collection's arrays, values / last_values / final_values, advantages / returns / valid, norm, ``minibatches`` (the
    step indices), per update ``stats`` [8], ``grads`` (eight arrays, GRAD_ORDER), ``adam_stats`` [4], and the final
    ``params`` / ``m`` / ``v`` (eight arrays each) and ``state_bytes``; ``facts``: see :func:`ppo_facts`."""
    actor, critic = _copy(actor), _copy(critic)
    col = ppo_collect(actor)
    values, last_values, final_values = ppo_values(col, critic)
    gae_args = (col["reward"], col["agent_flags"], col["env_flags"], values, last_values)
    adv, ret, valid = gae_spec(*gae_args, final_values, PPO["GAMMA"], PPO["LAM"])
    norm = masked_moments_spec(adv, valid)
    source = dict(rows=col["rows"], actions=col["actions"], logp=col["logp"], advantages=adv, returns=ret, masks=col["masks"],
                  valid=valid)
    params = actor + critic                                                          # the same arrays: Adam updates in place
    ms, vs, state = [np.zeros_like(p) for p in params], [np.zeros_like(p) for p in params], new_state()
    updates = dict(stats=[], grads=[], adam_stats=[], changed=[])
    minibatches = ppo_minibatches()
    for step, steps in enumerate(minibatches):
        mb = {k: v[steps] for k, v in source.items()}
        x = mb["rows"].reshape(-1, mb["rows"].shape[-1])
        stats, grads, _, _ = ppo_update_gradients(x, mb, actor, critic, norm)
        before = _copy(params)
        adam_stats = adam_step_spec(params, grads, ms, vs, state, ppo_lr(step), weight_decay=PPO["WEIGHT_DECAY"],
                                    max_grad_norm=PPO["MAX_GRAD_NORM"])
        updates["stats"].append(stats)
        updates["grads"].append(grads)
        updates["adam_stats"].append(adam_stats)
        updates["changed"].append([bool((a.view(np.uint32) != b.view(np.uint32)).any()) for a, b in zip(params, before)])
    out = dict(col, values=values, last_values=last_values, final_values=final_values, advantages=adv, returns=ret, valid=valid,
               norm=norm, minibatches=minibatches, **updates, params=_copy(params), m=_copy(ms), v=_copy(vs),
               state_bytes=state_bytes(state), rows_per_minibatch=PPO["K"] // PPO["MINIBATCHES"] * PPO["E"] * N)
    out["advantages_without_final"] = gae_spec(*gae_args, None, PPO["GAMMA"], PPO["LAM"])[0]
    out["facts"] = ppo_facts(out)
    return out


def ppo_facts(r) -> dict:
    """What the iteration exercised: the conditions tests/test_learner_chain_reference.py asserts."""
    af, ef, acts = r["agent_flags"], r["env_flags"], r["actions"]
    reset = (ef & EF_RESET) != 0
    live = acts != 255
    cut = ((af & AF_LIVE) != 0) & ((af & AF_TERMINATED) == 0) & reset[..., None]
    counts = [int(s[6]) for s in r["stats"]]
    scales = [float(s[1]) for s in r["adam_stats"]]
    lrs = [float(s[3]) for s in r["adam_stats"]]
    return dict(
        terminated_agent_steps=int(((af & AF_TERMINATED) != 0).sum()), truncated_agent_steps=int(((af & AF_TRUNCATED) != 0).sum()),
        steps_with_a_partial_reset=int((reset.any(1) & ~reset.all(1)).sum()), dead_slots=int((~live).sum()),
        actions_drawn=sorted(int(a) for a in np.unique(acts[live])), restricted_masks=int((r["masks"][live] != 0x1F).sum()),
        max_episode_in_a_key=int((r["episode"][:, :, None] * live).max()), minibatch_counts=counts,
        cut_rows_with_final_values=int((cut & (r["final_values"] != 0)).sum()),
        cut_rows_whose_advantage_needs_final_values=int((cut & (r["advantages"] != r["advantages_without_final"])).sum()),
        adam_scales=scales, adam_skipped=[float(s[2]) for s in r["adam_stats"]], adam_lrs=lrs,
        every_tensor_changed_in_every_step=all(all(c) for c in r["changed"]))


def assert_ppo_coverage(r) -> None:
    f, rows = r["facts"], r["rows_per_minibatch"]
    assert f["terminated_agent_steps"] > 0 and f["truncated_agent_steps"] > 0, f
    assert f["steps_with_a_partial_reset"] > 0 and f["dead_slots"] > 0, f
    assert f["actions_drawn"] == [0, 1, 2, 3, 4] and f["restricted_masks"] > 0 and f["max_episode_in_a_key"] > 0, f
    assert rows == 576 and all(0 < c < rows for c in f["minibatch_counts"]), f
    assert f["cut_rows_with_final_values"] > 0 and f["cut_rows_whose_advantage_needs_final_values"] > 0, f
    assert len(f["adam_scales"]) == 8 and sum(s < 1.0 for s in f["adam_scales"]) >= 2 and sum(s == 1.0 for s in f["adam_scales"]) >= 2, f
    assert not any(f["adam_skipped"]) and f["every_tensor_changed_in_every_step"], f
    at = PPO["LR_CHANGE_AFTER"]
    assert f["adam_lrs"] == [float(F32(ppo_lr(s))) for s in range(8)] and f["adam_lrs"][at - 1] != f["adam_lrs"][at], f


# ---------------------------------------------------------------------------------------------------------------------
# DQN
# ---------------------------------------------------------------------------------------------------------------------
def compact_of_rows(rows):
    """Compact records [..., N, 4] of DefaultObservation rows [..., N, L]: slot j >= 1 as row 0 sees it, slot 0 as row 1."""
    n = rows.shape[-2]
    return np.ascontiguousarray(np.stack([rows[..., 1, 6:10]] + [rows[..., 0, 6 + 4 * j:10 + 4 * j] for j in range(1, n)], axis=-2))


def side_slots(num_boarding: int):
    return [list(range(num_boarding)), list(range(num_boarding, N))]


def sides_forward(x, heads, slots):
    """SideHeads on rows x [..., N, L]: by definition each head's MlpHead outputs at its own slots.  (q, hidden); q has the
    heads' O columns (5: Q-values; 6: a dueling head's advantages and state value)."""
    q = np.zeros(x.shape[:-1] + (heads[0][2].shape[0],), F32)
    hid = np.zeros(x.shape[:-1] + (H,), F32)
    for p, sl in zip(heads, slots):
        q[..., sl, :], hid[..., sl, :] = _head(np.ascontiguousarray(x[..., sl, :]), p, TANH)
    return q, hid


def dqn_reference(online):
    """The loop from the initial online parameters, a list of two (w1t, b1, w2, b2) in the order of SIDES; the target starts
    as a copy.  Returns per actor step ``actions`` / ``explored`` (WARMUP + ROUNDS of them), per round ``epsilon``,
    ``index``, the fetched minibatch ``mb``, ``td_stats`` (two [8]), ``grads`` (eight arrays, ``online.parameters()`` order),
    ``adam_stats``; and the final ``params``, ``target``, ``m``, ``v``, ``state_bytes``, ``ring_state``; ``facts``."""
    E, S, B = DQN["E"], DQN["RING_STEPS"], DQN["BATCH"]
    config = chain_config()
    oracle, params_c, ob = _oracle_batch(config, E)
    ob.set_state(step_count=DQN_START_STEP_COUNT)
    nb = config.num_boarding_agents
    slots = side_slots(nb)
    consts = row_consts(params_c)
    heads = [_copy(p) for p in online]
    target = [_copy(p) for p in heads]
    flat = [p for h in heads for p in h]
    ms, vs, state = [np.zeros_like(p) for p in flat], [np.zeros_like(p) for p in flat], new_state()
    ring = new_ring(S, E, N)
    first_side = np.array([a in slots[0] for a in range(N)])
    side_u8 = [np.array([a in sl for a in range(N)], np.uint8) for sl in slots]
    out = dict(actions=[], explored=[], epsilon=[], index=[], mb=[], td_stats=[], grads=[], adam_stats=[], filled=[], copies=[],
               target_differs=[], head=[], drawn_resets=[])
    obs_c = compact_of_rows(ob.observe())
    reset_slots = np.zeros(S * E, bool)

    def actor_step(eps):
        nonlocal obs_c
        rows = ob.observe()
        masks = _masks(oracle, params_c, ob)
        q, _ = sides_forward(rows, heads, slots)
        acts, explored = q_actions_spec(q, masks, ob.terminated, ob.truncated, ob.step_count.copy(), ob.episode.copy(), seed=SEED,
                                        epsilon=F32(eps))
        step_obs, reward, af, ef = ob.rollout(acts[None], auto_reset=True)
        reset = (ef[0] & EF_RESET) != 0
        next_rows = np.where(reset[:, None, None], ob.observe(), step_obs[0])        # reset_obs="next"
        assert (next_rows == ob.observe()).all(), "observe() of the stepped state is the rollout's last row block"
        next_c, final_c = compact_of_rows(next_rows), compact_of_rows(step_obs[0])
        masks_next = _masks(oracle, params_c, ob)
        head = int(ring["state"][0])
        reset_slots[(head % S) * E:(head % S) * E + E] = reset
        push_spec(ring, obs_c, acts[None], reward, af, ef, next_c[None], final_c[None], masks_next[None])
        obs_c = next_c
        out["actions"].append(acts)
        out["explored"].append(explored)

    for _ in range(DQN["WARMUP"]):
        actor_step(DQN["EPS"][0])
    for u in range(DQN["ROUNDS"]):
        eps = float(F32(dqn_epsilon(u)))
        actor_step(eps)
        out["epsilon"].append(eps)
        out["head"].append(int(ring["state"][0]))
        out["filled"].append(filled_spec(int(ring["state"][0]), S, E))
        index = sample_index_spec(ring, SEED, B)
        mb = fetch_spec(ring, index, consts)
        q, hid = sides_forward(mb["obs"], heads, slots)
        qt, _ = sides_forward(mb["next_obs"], target, slots)
        qo, _ = sides_forward(mb["next_obs"], heads, slots)
        args = (q, mb["actions"], mb["reward"], mb["done"], qt, qo, mb["masks_next"])
        stats, gq_side = [], []
        for side in side_u8:
            valid = (mb["valid"] * side[None, :]).astype(np.uint8)                   # valid & side (0 / 4 times 0 / 1)
            st, _ = td_loss_spec(*args, valid=valid, gamma=DQN["GAMMA"], huber_delta=DQN["HUBER_DELTA"])
            stats.append(st)
            gq_side.append(td_loss_backward_spec(*args, valid=valid, gamma=DQN["GAMMA"], huber_delta=DQN["HUBER_DELTA"],
                                                 stats=st).reshape(B, N, 5))
        gq = np.where(first_side[None, :, None], gq_side[0], gq_side[1])             # each side keeps its own bits
        grads = []
        for p, sl in zip(heads, slots):
            g = mlp_backward_spec(*(np.ascontiguousarray(a[:, sl]).reshape(B * len(sl), -1) for a in (mb["obs"], hid, gq)), p[2], TANH)
            grads += [g[k] for k in NAMES]
        out["target_differs"].append(bool((qt.view(np.uint32) != qo.view(np.uint32)).any()))
        adam_stats = adam_step_spec(flat, grads, ms, vs, state, DQN["LR"], max_grad_norm=DQN["MAX_GRAD_NORM"])
        copied = (u + 1) % DQN["TARGET_EVERY"] == 0
        if copied:
            target = [_copy(p) for p in heads]
        out["copies"].append(copied)
        out["drawn_resets"].append(int(reset_slots[index].sum()))
        for k, v in (("index", index), ("mb", mb), ("td_stats", stats), ("grads", grads), ("adam_stats", adam_stats)):
            out[k].append(v)
    out.update(params=_copy(flat), target=[np.array(p, copy=True) for h in target for p in h], m=_copy(ms), v=_copy(vs),
               state_bytes=state_bytes(state), ring_state=ring["state"].copy(), capacity=S * E, consts=consts)
    out["facts"] = dqn_facts(out)
    return out


def dqn_facts(r) -> dict:
    w = DQN["WARMUP"]
    live = [a != 255 for a in r["actions"][w:]]
    return dict(
        ring_heads=r["head"], ring_steps=DQN["RING_STEPS"], filled=r["filled"], capacity=r["capacity"],
        side_counts=[[int(s[6]) for s in pair] for pair in r["td_stats"]],
        explored_per_round=[int(e.sum()) for e in r["explored"][w:]],
        greedy_per_round=[int((l & (e == 0)).sum()) for l, e in zip(live, r["explored"][w:])],
        epsilons=r["epsilon"], copies=r["copies"], target_differs=r["target_differs"], drawn_records_that_end_an_episode=r["drawn_resets"],
        adam_skipped=[float(s[2]) for s in r["adam_stats"]], adam_scales=[float(s[1]) for s in r["adam_stats"]])


def assert_dqn_coverage(r) -> None:
    f = r["facts"]
    assert max(f["ring_heads"]) > f["ring_steps"], f                                 # the head passes the capacity: the ring wraps
    assert any(x < f["capacity"] for x in f["filled"]) and any(x == f["capacity"] for x in f["filled"]), f
    assert all(c > 0 for pair in f["side_counts"] for c in pair), f
    assert all(e > 0 for e in f["explored_per_round"]) and all(g > 0 for g in f["greedy_per_round"]), f
    assert len(set(f["epsilons"])) == DQN["ROUNDS"], f                               # every round has its own f32 rate
    first = f["copies"].index(True)
    assert first + 1 < DQN["ROUNDS"] and f["target_differs"][first], f              # a copy between two updates, and it matters
    assert sum(f["drawn_records_that_end_an_episode"]) > 0 and not any(f["adam_skipped"]), f
