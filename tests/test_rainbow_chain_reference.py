"""The composed CPU references of tests/_rainbow_chain.py, run once from ``linear_init`` parameters: that their inputs exercise
what tests/test_gpu_rainbow_chain.py and tests/test_gpu_ppo_minibatch_chain.py are meant to exercise (conditions, not
measurements); that every plausible wiring mistake (``mutate=``) changes the result, so a device making it could not pass the
comparison; and two checks against something that is not made of the project's specs -- the first Rainbow update's eight
gradients against torch f64 autograd of the textbook computation, and its new leaves against the priority rule in f64.

Chosen on the CPU so that the reference alone meets every condition (tests/_rainbow_chain.py holds the values): ``linear_init``
seeds 3 / 4 for the two dueling heads and 30 / 31 for actor and critic, ``set_rng_seed(0x0123456789ABCDEF)``, a ring of 6 steps
with n = 3, the hand truncation before round 3 and the envs put back before round 7, ``max_grad_norm`` 2.0 (the twelve
gradient norms lie between 1.4 and 5.2) and 6.9 for PPO (the eight lie between 5.9 and 7.7)."""

import numpy as np
import pytest
from _learner_chain import H, N, PPO_INIT_SEEDS, SIDES, side_slots
from _mlp_spec import linear_init
from _prio_spec import ONE_FIXED, POW_REL_BOUND
from _rainbow_chain import (DRAW_SIDE_MUTATIONS, MUTATIONS, PPO_MUTATIONS, RAINBOW, RAINBOW_GRAD_ORDER, RAINBOW_INIT_SEEDS,
                            assert_ppo_minibatch_coverage, assert_rainbow_coverage, first_difference, ppo_minibatch_reference,
                            rainbow_reference)

L = 6 + 4 * N


def rainbow_init():
    return [linear_init(L, H, RAINBOW["O"], seed=s) for s in RAINBOW_INIT_SEEDS]


def ppo_init():
    return linear_init(L, H, 5, seed=PPO_INIT_SEEDS[0]), linear_init(L, H, 1, seed=PPO_INIT_SEEDS[1])


def differ(a, b) -> bool:
    return any(x.tobytes() != y.tobytes() for x, y in zip(a, b))


@pytest.fixture(scope="module")
def rainbow(oracle):
    return rainbow_reference(rainbow_init())


@pytest.fixture(scope="module")
def ppo_mb(oracle):
    return ppo_minibatch_reference(*ppo_init(), "rows")


# ------------------------------------------------------------------------------------------------------------ coverage
def test_the_rainbow_loop_exercises_what_the_gpu_test_compares(rainbow):
    for k, v in rainbow["facts"].items():
        print(f"rainbow {k}: {v}")
    assert_rainbow_coverage(rainbow)
    R = RAINBOW
    assert rainbow["ring_state"].tolist() == [R["WARMUP"] + R["ROUNDS"], 0, 0, 0] and int(rainbow["pstate"][1]) == R["ROUNDS"]
    assert all(np.isfinite(p).all() for group in (rainbow["params"], rainbow["target"], rainbow["m"], rainbow["v"]) for p in group)
    assert differ(rainbow["params"], rainbow["target"])                  # the target is the online network of the last copy
    assert (rainbow["leaf"] > 0).all() and rainbow["cut"].any() and not rainbow["cut"].all()


def test_the_ppo_minibatch_iteration_exercises_what_the_gpu_test_compares(ppo_mb):
    for k, v in ppo_mb["facts"].items():
        print(f"ppo minibatches {k}: {v}")
    assert_ppo_minibatch_coverage(ppo_mb)
    assert all(np.isfinite(p).all() for group in (ppo_mb["params"], ppo_mb["m"], ppo_mb["v"]) for p in group)
    assert ppo_mb["state_bytes"][16:24].view(np.int64)[0] == 8 and not ppo_mb["state_bytes"][24:].any()
    # the EMPTY tail: index -1, actions 255, valid 0, and rows of the all-zero compact record
    tail = ppo_mb["mb"][3]
    assert (tail["index"][48:] == -1).all() and (tail["actions"][48:] == 255).all() and not tail["valid"][48:].any()
    assert (tail["index"][:48] >= 0).all()


def test_the_compact_source_gives_the_rows_sources_iteration(ppo_mb, oracle):
    compact = ppo_minibatch_reference(*ppo_init(), "compact")
    assert compact["source"]["obs"].shape[-1] == 4 and ppo_mb["source"]["obs"].shape[-1] == L
    for i, (a, b) in enumerate(zip(compact["mb"], ppo_mb["mb"])):
        assert all(a[k].tobytes() == b[k].tobytes() for k in a), f"update {i}"
    assert not differ(compact["params"], ppo_mb["params"]) and not differ(compact["v"], ppo_mb["v"])


# ------------------------------------------------------------------------------------------------------------ sensitivity
@pytest.mark.parametrize("mutation", MUTATIONS)
def test_a_wrong_wire_in_the_rainbow_loop_changes_the_result(rainbow, mutation):
    wrong = rainbow_reference(rainbow_init(), mutate=mutation)
    first = first_difference(rainbow, wrong)
    print(f"rainbow mutation {mutation}: first array that changed: {first}")
    assert first is not None and differ(rainbow["params"], wrong["params"]), mutation
    if mutation in DRAW_SIDE_MUTATIONS:
        u0 = int(first.split(":")[0].split()[1])
        later = [u for u in range(u0 + 1, RAINBOW["ROUNDS"])
                 if any(rainbow["rounds"][u][k].tobytes() != wrong["rounds"][u][k].tobytes() for k in ("index", "weights"))]
        print(f"rainbow mutation {mutation}: later rounds whose index or weights differ: {later}")
        assert later, mutation


@pytest.mark.parametrize("mutation", PPO_MUTATIONS)
def test_a_wrong_wire_in_the_ppo_minibatches_changes_the_result(ppo_mb, mutation):
    wrong = ppo_minibatch_reference(*ppo_init(), "rows", mutate=mutation)
    first = next((f"update {i}: {k}" for i in range(8) for k in ("index", "obs")
                  if ppo_mb["mb"][i][k].tobytes() != wrong["mb"][i][k].tobytes()), None)
    print(f"ppo minibatch mutation {mutation}: first array that changed: {first}")
    assert first is not None and differ(ppo_mb["params"], wrong["params"]), mutation


# ------------------------------------------------------------------------------------------------------------ yardsticks
def test_the_first_rainbow_gradient_against_torch_f64_autograd(rainbow):
    """The composition is not only self-consistent: the eight gradients of the first update against autograd of the textbook
    computation in torch f64 on the same fetched minibatch, weights and initial parameters (online == target) -- dueling
    combine, masked double-Q argmax, ``r + discount (1 - done) Q_target``, Huber loss, an importance-weighted mean over each
    side's counting rows.  The yardstick is the one of tests/test_learner_chain_reference.py: the f32 torch module's own
    error against f64, times 4."""
    import torch

    rnd, init = rainbow["rounds"][0], rainbow_init()
    slots = side_slots(5)
    t = {k: torch.from_numpy(np.ascontiguousarray(rnd[k])) for k in ("mb.obs", "mb.next_obs", "mb.actions", "mb.reward", "mb.done",
                                                                      "mb.valid", "mb.masks_next", "mb.discount", "weights")}
    legal = (((t["mb.masks_next"].to(torch.int64) | 0x10)[..., None] >> torch.arange(5)) & 1).bool()
    delta = RAINBOW["HUBER_DELTA"]

    def gradients(dtype):
        par = [[torch.from_numpy(p).to(dtype).requires_grad_(True) for p in head] for head in init]

        def q_of(x, sl, p):
            w1t, b1, w2, b2 = p
            va = torch.tanh(x[:, sl].to(dtype) @ w1t + b1) @ w2.t() + b2
            return va[..., 5:6] + (va[..., :5] - va[..., :5].mean(-1, keepdim=True))

        total, counts = 0.0, []
        for sl, p in zip(slots, par):
            q = q_of(t["mb.obs"], sl, p)
            with torch.no_grad():
                q_next = q_of(t["mb.next_obs"], sl, p)                                  # online == target in the first round
                kstar = q_next.masked_fill(~legal[:, sl], -torch.inf).argmax(-1, keepdim=True)
                boot = q_next.gather(-1, kstar)[..., 0]
                y = t["mb.reward"][:, sl].to(dtype) + t["mb.discount"][:, sl].to(dtype) * (1 - (t["mb.done"][:, sl] != 0).to(dtype)) * boot
            a = t["mb.actions"][:, sl]
            c = (t["mb.valid"][:, sl] != 0) & (a <= 4)
            d = q.gather(-1, a.clamp(max=4).to(torch.int64)[..., None])[..., 0] - y
            h = torch.where(d.abs() <= delta, 0.5 * d * d, delta * (d.abs() - 0.5 * delta))
            total = total + (t["weights"][:, sl].to(dtype) * h)[c].sum() / c.sum()
            counts.append(int(c.sum()))
        total.backward()
        return counts, [p.grad.double().numpy() for head in par for p in head]

    counts, g64 = gradients(torch.float64)
    _, g32 = gradients(torch.float32)
    assert counts == [int(rnd[f"td_stats.{s}"][6]) for s in SIDES]
    for name, a, b in zip(RAINBOW_GRAD_ORDER, g32, g64):
        ours = rnd[f"grad.{name}"]
        err, yard = float(np.abs(ours.astype(np.float64) - b).max()), float(np.abs(a - b).max())
        print(f"first rainbow update, grad {name}: max |reference - f64| = {err:.3e}, max |f32 torch - f64| = {yard:.3e}, "
              f"ratio {err / yard if yard else float('nan'):.3f}, max |f64| = {float(np.abs(b).max()):.3e}")
        assert ours.shape == b.shape and np.abs(b).max() > 0 and err <= 4.0 * yard, name


def test_the_first_updates_leaves_against_the_priority_rule_in_f64(rainbow):
    """``floor(65536 (max |td| + eps)^alpha)`` in f64 over both sides' ``td_error`` and all agents, the maximum over a record's
    duplicates.  The allowance is derived, not measured: 1 for the floor, plus POW_REL_BOUND relative (tests/_prio_spec.py)."""
    rnd = rainbow["rounds"][0]
    td = np.maximum(*(np.abs(rnd[f"td_error.{s}"].astype(np.float64)).max(-1) for s in SIDES))     # [B]
    p = 65536.0 * (td + RAINBOW["PRIO_EPS"]) ** RAINBOW["ALPHA"]
    want, slack = {}, {}
    for i, v in zip(rnd["index"].tolist(), p.tolist()):
        if v >= want.get(i, -1.0):
            want[i], slack[i] = v, 1.0 + POW_REL_BOUND * v
    leaf = rnd["leaf"].astype(np.float64)
    worst = max(abs(leaf[i] - np.floor(want[i])) / slack[i] for i in want)
    print(f"first rainbow update: {len(want)} leaves written, worst |leaf - floor(f64 rule)| / allowance = {worst:.3f}; "
          f"leaves {int(leaf[list(want)].min())} .. {int(leaf[list(want)].max())}")
    assert len(want) < len(rnd["index"]) and worst <= 1.0                # (duplicates among the drawn records)
    pushed = rainbow["rounds"][0]["leaf_drawn"]
    assert (pushed == ONE_FIXED).all()                                   # before the first update every leaf is max_leaf = 1.0
    untouched = np.setdiff1d(np.flatnonzero(rnd["leaf"]), np.array(list(want)))
    assert (rnd["leaf"][untouched] == ONE_FIXED).all() and int(rnd["pstate"][0]) == int(leaf.max()) > ONE_FIXED
