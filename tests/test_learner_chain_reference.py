"""The composed CPU references of tests/_learner_chain.py, run once from ``linear_init`` parameters: that their inputs
exercise what tests/test_gpu_learner_chain.py is meant to exercise (conditions, not measurements), and one check against
something that is not made of the project's specs -- the first PPO update's gradient against torch f64 autograd of the
textbook clipped-surrogate loss.

Chosen on the CPU so that the reference alone meets every condition below (tests/_learner_chain.py holds the values):
``linear_init`` seeds 30 / 31 for actor and critic and 3 / 4 for the two DQN heads, ``set_rng_seed(0x0123456789ABCDEF)``, the
step permutation from ``default_rng(7)``, ``max_grad_norm = 6.3`` (the eight gradient norms lie between 5.3 and 9.5), step
counters staggered at the start so that envs restart in different steps, and for the DQN ring 2 warm-up steps: with a ring
of 4 steps and a push before every update, a third warm-up step would fill the ring before the first minibatch is drawn."""

import numpy as np
import pytest
from _learner_chain import (DQN, DQN_INIT_SEEDS, GRAD_ORDER, N, PPO, PPO_INIT_SEEDS, assert_dqn_coverage, assert_ppo_coverage,
                            dqn_reference, ppo_reference)
from _mlp_spec import linear_init

L, H = 6 + 4 * N, 16


@pytest.fixture(scope="module")
def ppo(oracle):
    return ppo_reference(linear_init(L, H, 5, seed=PPO_INIT_SEEDS[0]), linear_init(L, H, 1, seed=PPO_INIT_SEEDS[1]))


@pytest.fixture(scope="module")
def dqn(oracle):
    return dqn_reference([linear_init(L, H, 5, seed=s) for s in DQN_INIT_SEEDS])


def test_the_ppo_iteration_exercises_what_the_gpu_test_compares(ppo):
    for k, v in ppo["facts"].items():
        print(f"ppo {k}: {v}")
    print("ppo gradient norms:", [float(s[0]) for s in ppo["adam_stats"]])
    assert ppo["rows"].shape == (PPO["K"], PPO["E"], N, L) and len(ppo["minibatches"]) == 8
    assert sorted(np.concatenate(ppo["minibatches"][:4]).tolist()) == list(range(PPO["K"]))
    assert_ppo_coverage(ppo)
    assert all(np.isfinite(p).all() for group in (ppo["params"], ppo["m"], ppo["v"]) for p in group)
    assert ppo["state_bytes"][16:24].view(np.int64)[0] == 8 and not ppo["state_bytes"][24:].any()


def test_the_dqn_loop_exercises_what_the_gpu_test_compares(dqn):
    for k, v in dqn["facts"].items():
        print(f"dqn {k}: {v}")
    assert_dqn_coverage(dqn)
    assert dqn["ring_state"].tolist() == [DQN["WARMUP"] + DQN["ROUNDS"], DQN["ROUNDS"], 0, 0]
    assert all(np.isfinite(p).all() for group in (dqn["params"], dqn["target"], dqn["m"], dqn["v"]) for p in group)
    # the target is the online network of the last copy, not of the end: the two differ after the last two updates
    assert any((a != b).any() for a, b in zip(dqn["params"], dqn["target"]))


def test_the_first_ppo_gradient_against_torch_f64_autograd(ppo):
    """The composition is not only self-consistent: the eight gradients of the first update against autograd of the textbook
    loss in torch f64 on the same rows and initial parameters.  The yardstick is the one of tests/test_gpu_mlp.py and
    tests/test_gpu_mlp_backward.py: the f32 torch module's own error against f64, times 4."""
    import torch

    steps = ppo["minibatches"][0]
    init = [linear_init(L, H, 5, seed=PPO_INIT_SEEDS[0]), linear_init(L, H, 1, seed=PPO_INIT_SEEDS[1])]
    take = {k: torch.from_numpy(np.ascontiguousarray(ppo[k][steps])).reshape((-1,) + ppo[k].shape[3:])
            for k in ("rows", "actions", "logp", "advantages", "returns", "masks", "valid")}
    counts = (take["valid"] != 0) & (take["actions"] != 255)
    assert int(counts.sum()) == int(ppo["stats"][0][6])
    legal = (((take["masks"].to(torch.int64) | 0x10)[:, None] >> torch.arange(5)) & 1).bool()
    hyper = PPO["HYPER"]

    def gradients(dtype):
        par = [[torch.from_numpy(p).to(dtype).requires_grad_(True) for p in head] for head in init]
        x = take["rows"].to(dtype)
        (w1t, b1, w2, b2), (c1t, cb1, c2, cb2) = par
        logits = torch.tanh(x @ w1t + b1) @ w2.t() + b2
        values = (torch.relu(x @ c1t + cb1) @ c2.t() + cb2)[:, 0]
        lsm = torch.log_softmax(logits.masked_fill(~legal, -torch.inf), -1)
        logp = lsm.gather(1, take["actions"].clamp(max=4).to(torch.int64)[:, None])[:, 0]
        entropy = -(torch.where(legal, lsm.exp() * lsm.masked_fill(~legal, 0.0), torch.zeros((), dtype=dtype))).sum(-1)
        ratio = (logp - take["logp"].to(dtype)).exp()
        mean, std = float(ppo["norm"][1]), float(ppo["norm"][2])
        an = (take["advantages"].to(dtype) - mean) / (std + 1e-8)
        surr = torch.minimum(ratio * an, ratio.clamp(1.0 - hyper["clip"], 1.0 + hyper["clip"]) * an)
        n = counts.sum()
        policy = -(surr[counts].sum() / n)
        value = ((values - take["returns"].to(dtype)) ** 2)[counts].sum() / n
        loss = policy + hyper["vf_coef"] * value - hyper["ent_coef"] * (entropy[counts].sum() / n)
        loss.backward()
        return float(loss.detach()), [p.grad.double().numpy() for head in par for p in head]

    loss64, g64 = gradients(torch.float64)
    _, g32 = gradients(torch.float32)
    # the loss itself, as a guard on the wiring (which of norm's four numbers is the mean, which mask bit is which action): a
    # mean of 570 terms, each a handful of f32 roundings (6e-8 relative) of numbers no larger than the loss -- 1e-6 is 16 ulp
    assert abs(float(ppo["stats"][0][0]) - loss64) <= 1e-6 * max(1.0, abs(loss64)), (float(ppo["stats"][0][0]), loss64)
    for name, ours, a, b in zip(GRAD_ORDER, ppo["grads"][0], g32, g64):
        err, yard = float(np.abs(ours.astype(np.float64) - b).max()), float(np.abs(a - b).max())
        print(f"first update, grad {name}: max |reference - f64| = {err:.3e}, max |f32 torch - f64| = {yard:.3e}, "
              f"ratio {err / yard if yard else float('nan'):.3f}, max |f64| = {float(np.abs(b).max()):.3e}")
        assert ours.shape == b.shape and np.abs(b).max() > 0 and err <= 4.0 * yard, name
