"""The composed CPU reference of tests/_c51_chain.py, run once from ``linear_init`` parameters: that its inputs exercise what
tests/test_gpu_c51_chain.py is meant to exercise (conditions, not measurements); that every plausible wiring mistake
(``mutate=``) changes the result, so a device making it could not pass the comparison; and two checks against something that is
not made of the project's specs -- the first update's twenty gradients against torch f64 autograd of the textbook computation,
and its new leaves against the priority rule in f64.

Chosen on the CPU so that the reference alone meets every condition (tests/_c51_chain.py holds the values): ``linear_init``
seeds 11 .. 15 for the five heads, ``set_rng_seed(0x0123456789ABCDEF)``, the Rainbow loop's ring, n, hand truncation and event,
the support [-3, 4] with 8 atoms, ``max_grad_norm`` 0.3 (the twelve gradient norms lie between 0.24 and 0.38).  Every
condition the issue names is met by these short episodes; two are read as follows.  "Leaves written above and below the leaf
of a fresh push": against ``max_leaf`` at the time of the write, which IS the leaf of the next push -- the first update raises
it from 1.0 (a row's cross-entropy starts near log 8), every later round writes below it.  "A position exactly on an atom":
counted only INSIDE the support, on an atom that carries mass, not where a clamp put it."""

import numpy as np
import pytest
from _c51_chain import (C51, C51_DRAW_SIDE_MUTATIONS, C51_GRAD_ORDER, C51_LINKS, C51_MUTATIONS, HEADS, assert_c51_coverage, c51_init,
                        c51_reference)
from _learner_chain import N
from _prio_spec import ONE_FIXED, POW_REL_BOUND
from _rainbow_chain import first_difference


def differ(a, b) -> bool:
    return any(x.tobytes() != y.tobytes() for x, y in zip(a, b))


@pytest.fixture(scope="module")
def c51(oracle):
    return c51_reference(c51_init())


# ------------------------------------------------------------------------------------------------------------ coverage
def test_the_c51_loop_exercises_what_the_gpu_test_compares(c51):
    for k, v in c51["facts"].items():
        print(f"c51 {k}: {v}")
    assert_c51_coverage(c51)
    C = C51
    assert c51["ring_state"].tolist() == [C["WARMUP"] + C["ROUNDS"], 0, 0, 0] and int(c51["pstate"][1]) == C["ROUNDS"]
    assert len(c51["params"]) == 4 * HEADS == len(C51_GRAD_ORDER) == 20
    assert all(np.isfinite(p).all() for group in (c51["params"], c51["target"], c51["m"], c51["v"]) for p in group)
    assert differ(c51["params"], c51["target"])                          # the target is the online network of the last copy
    assert (c51["leaf"] > 0).all() and c51["cut"].any() and not c51["cut"].all()
    for rnd in c51["rounds"]:                                            # the layout the backward is taken apart in
        assert rnd["logits"].shape == rnd["grad_logits"].shape == (C["BATCH"], N, HEADS, C["ATOMS"])
        taken = np.arange(HEADS)[None, None, :] == rnd["mb.actions"][:, :, None]
        assert not rnd["grad_logits"][~taken].any() and rnd["grad_logits"][taken].any()
        assert all(rnd[f"grad.head{k}.w2"].any() for k in range(HEADS))  # every head is stepped in every round


# ------------------------------------------------------------------------------------------------------------ sensitivity
@pytest.mark.parametrize("mutation", C51_MUTATIONS)
def test_a_wrong_wire_in_the_c51_loop_changes_the_result(c51, mutation):
    wrong = c51_reference(c51_init(), mutate=mutation)
    first = first_difference(c51, wrong, C51_LINKS)
    print(f"c51 mutation {mutation}: first array that changed: {first}")
    assert first is not None and differ(c51["params"], wrong["params"]), mutation
    if mutation in C51_DRAW_SIDE_MUTATIONS:
        u0 = int(first.split(":")[0].split()[1])
        later = [u for u in range(u0 + 1, C51["ROUNDS"])
                 if any(c51["rounds"][u][k].tobytes() != wrong["rounds"][u][k].tobytes() for k in ("index", "weights"))]
        print(f"c51 mutation {mutation}: later rounds whose index or weights differ: {later}")
        assert later, mutation


# ------------------------------------------------------------------------------------------------------------ yardsticks
def test_the_first_c51_gradient_against_torch_f64_autograd(c51):
    """The composition is not only self-consistent: the twenty gradients of the first update against autograd of the textbook
    computation in torch f64 on the same fetched minibatch, weights and initial parameters (online == target) -- five
    two-layer heads, softmax expectations on the support, masked double-Q argmax, ``r + discount (1 - done) z`` clamped, the
    floor / ceil projection with two ``index_add_`` (examples/c51_dqn.py ``torch_c51_loss``), cross-entropy, an
    importance-weighted mean over the counting rows.  The yardstick is the one of tests/test_rainbow_chain_reference.py: the
    f32 torch computation's own error against f64, times 4 -- after both were seen to choose the same bootstrap action on
    every counting row (a condition on the chosen seeds: a different action is a different function)."""
    import torch

    rnd, init = c51["rounds"][0], c51_init()
    A, vmin, vmax = C51["ATOMS"], C51["VMIN"], C51["VMAX"]
    dz = (vmax - vmin) / (A - 1)
    t = {k: torch.from_numpy(np.ascontiguousarray(rnd[k]).reshape((-1,) + rnd[k].shape[2:]))
         for k in ("mb.obs", "mb.next_obs", "mb.actions", "mb.reward", "mb.done", "mb.valid", "mb.masks_next", "mb.discount", "weights")}
    rows = t["mb.actions"].numel()
    each = torch.arange(rows)
    legal = (((t["mb.masks_next"].to(torch.int64) | 0x10)[:, None] >> torch.arange(5)) & 1).bool()
    a = t["mb.actions"].to(torch.int64).clamp(max=4)
    counts = (t["mb.valid"] != 0) & (t["mb.actions"] <= 4)

    def gradients(dtype):
        par = [[torch.from_numpy(p).to(dtype).requires_grad_(True) for p in head] for head in init]
        z = torch.tensor(vmin, dtype=dtype) + torch.arange(A, dtype=dtype) * dz

        def net(x):                                                      # [rows, 5, A]
            return torch.stack([torch.tanh(x.to(dtype) @ w1t + b1) @ w2.t() + b2 for w1t, b1, w2, b2 in par], dim=1)

        logits = net(t["mb.obs"])
        with torch.no_grad():
            nxt = net(t["mb.next_obs"])                                  # online == target in the first round
            kstar = (torch.softmax(nxt, -1) * z).sum(-1).masked_fill(~legal, -torch.inf).argmax(-1)
            p = torch.softmax(nxt[each, kstar], -1)
            live = (t["mb.done"] == 0).to(dtype)
            tz = (t["mb.reward"].to(dtype)[:, None] + (t["mb.discount"].to(dtype) * live)[:, None] * z).clamp(vmin, vmax)
            b = ((tz - vmin) / dz).clamp(0, A - 1)
            lo, hi = b.floor().long(), b.ceil().long()
            offset = (each * A)[:, None]
            proj = torch.zeros(rows * A, dtype=dtype)
            proj.index_add_(0, (lo + offset).reshape(-1), (p * (hi.to(dtype) - b + (lo == hi).to(dtype))).reshape(-1))
            proj.index_add_(0, (hi + offset).reshape(-1), (p * (b - lo.to(dtype))).reshape(-1))
            proj = proj.view(rows, A)
        ce = -(proj * torch.log_softmax(logits[each, a], -1)).sum(-1)
        loss = (t["weights"].to(dtype) * ce)[counts].sum() / counts.sum()
        loss.backward()
        return kstar.numpy(), float(loss.detach()), [q.grad.double().numpy() for head in par for q in head]

    k64, loss64, g64 = gradients(torch.float64)
    k32, _, g32 = gradients(torch.float32)
    boot = (counts & (t["mb.done"] == 0)).numpy()
    assert boot.sum() > 200 and (k64[boot] == k32[boot]).all(), "the f32 and the f64 run choose different bootstrap actions"
    assert int(counts.sum()) == int(rnd["stats"][6])
    print(f"first c51 update: {int(counts.sum())} counting rows, loss {float(rnd['stats'][0]):.7f} against f64 {loss64:.7f}")
    worst = 0.0
    for name, g_32, g_64 in zip(C51_GRAD_ORDER, g32, g64):
        ours = rnd[f"grad.{name}"]
        err, yard = float(np.abs(ours.astype(np.float64) - g_64).max()), float(np.abs(g_32 - g_64).max())
        worst = max(worst, err / yard)
        print(f"first c51 update, grad {name}: max |reference - f64| = {err:.3e}, max |f32 torch - f64| = {yard:.3e}, "
              f"ratio {err / yard if yard else float('nan'):.3f}, max |f64| = {float(np.abs(g_64).max()):.3e}")
        assert ours.shape == g_64.shape and np.abs(g_64).max() > 0 and err <= 4.0 * yard, name
    print(f"first c51 update: worst ratio over the 20 gradients {worst:.3f} (allowed 4)")


def test_the_first_updates_leaves_against_the_priority_rule_in_f64(c51):
    """``floor(65536 (max row_loss + eps)^alpha)`` in f64 over all agents of a record, the maximum over a record's duplicates.
    The allowance is derived, not measured: 1 for the floor, plus POW_REL_BOUND relative (tests/_prio_spec.py)."""
    rnd = c51["rounds"][0]
    td = np.abs(rnd["row_loss"].astype(np.float64)).max(-1)                                        # [B]
    p = 65536.0 * (td + C51["PRIO_EPS"]) ** C51["ALPHA"]
    want, slack = {}, {}
    for i, v in zip(rnd["index"].tolist(), p.tolist()):
        if v >= want.get(i, -1.0):
            want[i], slack[i] = v, 1.0 + POW_REL_BOUND * v
    leaf = rnd["leaf"].astype(np.float64)
    worst = max(abs(leaf[i] - np.floor(want[i])) / slack[i] for i in want)
    print(f"first c51 update: {len(want)} leaves written, worst |leaf - floor(f64 rule)| / allowance = {worst:.3f}; "
          f"leaves {int(leaf[list(want)].min())} .. {int(leaf[list(want)].max())}")
    assert len(want) < len(rnd["index"]) and worst <= 1.0                # (duplicates among the drawn records)
    assert (rnd["leaf_drawn"] == ONE_FIXED).all()                        # before the first update every leaf is max_leaf = 1.0
    untouched = np.setdiff1d(np.flatnonzero(rnd["leaf"]), np.array(list(want)))
    assert (rnd["leaf"][untouched] == ONE_FIXED).all() and int(rnd["pstate"][0]) == int(leaf.max()) > ONE_FIXED
