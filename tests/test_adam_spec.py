"""The NumPy statement of CCX_ADAM (tests/_adam_spec.py) against torch in f64 on the CPU: ``clip_grad_norm_`` followed by
``torch.optim.AdamW`` (decay on) or ``torch.optim.Adam`` (decay off) on the same f32 gradients, 50 steps of the two-head set,
some of them clipped.  The maxima it prints, doubled, are the bounds of _adam_spec.py.  No GPU."""

import numpy as np
import pytest
import torch
from _adam_spec import (ADAM_M_BOUND, ADAM_PARAM_BOUND, ADAM_PARAM_BOUND_DECAY, ADAM_V_BOUND, TWO_HEADS, adam_step_spec,
                        new_state, padded_squares, sum_of_squares)
from _ppo_loss_spec import tree_sum, tree_sum_loop

STEPS = 50
LR, BETAS, EPS, MAX_NORM = 3e-4, (0.9, 0.999), 1e-8, 0.5


def _gradients(seed):
    """Per step a gradient list whose norm lies on either side of MAX_NORM from step to step."""
    rng = np.random.default_rng(seed)
    steps = []
    for s in range(STEPS):
        size = np.exp(rng.uniform(np.log(0.001), np.log(0.05)))           # norm of 5 476 such elements: 0.07 .. 3.7
        steps.append([(rng.standard_normal(n) * size).astype(np.float32) for n in TWO_HEADS])
    return steps


def _rel(got, want):
    return max(float(np.max(np.abs(g.astype(np.float64) - w) / np.maximum(1.0, np.abs(w)))) for g, w in zip(got, want))


@pytest.mark.parametrize("weight_decay", (0.0, 0.01))
def test_fifty_steps_against_torch_in_f64(weight_decay):
    rng = np.random.default_rng(7)
    start = [(rng.standard_normal(n) * 0.3).astype(np.float32) for n in TWO_HEADS]
    grad_steps = _gradients(11)
    # the reference
    ref = [torch.nn.Parameter(torch.from_numpy(p.astype(np.float64))) for p in start]
    cls = torch.optim.AdamW if weight_decay else torch.optim.Adam
    opt = cls(ref, lr=LR, betas=BETAS, eps=EPS, weight_decay=weight_decay)
    # the spec
    params = [p.copy() for p in start]
    ms, vs = [np.zeros_like(p) for p in params], [np.zeros_like(p) for p in params]
    state = new_state()
    clipped, worst = 0, dict(param=0.0, m=0.0, v=0.0, gn_ulps=0.0)
    for grads in grad_steps:
        for p, g in zip(ref, grads):
            p.grad = torch.from_numpy(g.astype(np.float64))
        norm64 = float(torch.nn.utils.clip_grad_norm_(ref, MAX_NORM))
        opt.step()
        stats = adam_step_spec(params, grads, ms, vs, state, LR, *BETAS, EPS, weight_decay, MAX_NORM)
        assert stats[2] == 0.0
        clipped += int(stats[1] < 1.0)
        assert (stats[1] < 1.0) == (norm64 + 1e-6 > MAX_NORM) or abs(norm64 - MAX_NORM) < 1e-5
        worst["gn_ulps"] = max(worst["gn_ulps"], abs(float(stats[0]) - norm64) / float(np.spacing(np.float32(norm64))))
        worst["param"] = max(worst["param"], _rel(params, [p.detach().numpy() for p in ref]))
        worst["m"] = max(worst["m"], _rel(ms, [opt.state[p]["exp_avg"].numpy() for p in ref]))
        worst["v"] = max(worst["v"], _rel(vs, [opt.state[p]["exp_avg_sq"].numpy() for p in ref]))
    print(f"weight_decay {weight_decay}: {clipped} of {STEPS} steps clipped; max |err| / max(1, |f64|): parameters {worst['param']:.3e}, "
          f"m {worst['m']:.3e}, v {worst['v']:.3e}; gn within {worst['gn_ulps']:.3f} f32 ulp of the f64 norm")
    assert 5 <= clipped <= STEPS - 5
    assert state["step"] == STEPS and state["skipped"] == 0
    assert worst["gn_ulps"] <= 1.0
    assert worst["param"] <= (ADAM_PARAM_BOUND_DECAY if weight_decay else ADAM_PARAM_BOUND)
    assert worst["m"] <= ADAM_M_BOUND and worst["v"] <= ADAM_V_BOUND


def test_the_tree_is_the_loss_tree_on_the_padded_sequence():
    rng = np.random.default_rng(3)
    grads = [rng.standard_normal(n).astype(np.float32) for n in (257, 1, 64, 300)]
    seq = padded_squares(grads)
    assert seq.size == (2 + 1 + 1 + 2) * 256 and not seq[257:512].any() and not seq[513:768].any()
    S = sum_of_squares(grads)
    assert np.float64(S).view(np.uint64) == np.float64(tree_sum(seq)).view(np.uint64) == np.float64(tree_sum_loop(seq)).view(np.uint64)
    exact = sum(float(np.sum(g.astype(np.float64) ** 2)) for g in grads)
    assert abs(float(S) - exact) <= 1e-13 * exact
