"""The NumPy spec of CCX_MLP_DEEP (tests/_mlp_deep_spec.py) against the specs of CCX_MLP through the two identities of the
rule, and the accuracy numbers include/ccx.h and the README quote: the rule of csrc/ccx_mlp_deep.h (compiled for the host;
tests/test_mlp_deep_host_rule.py shows it equal to the NumPy spec) against the textbook composition in torch f64 on the same
f32 inputs -- x, the six parameters and grad_y; autograd gives the six gradients, so the f64 side forms its own hiddens and
relu masks -- at L = 38, O = 5 with 64-64 and with 256-256, torch.nn.Linear's initial weights, observation-like rows, both
activations, M = 20 000.  The recorded bounds are the measured maxima doubled, for the inputs the samples did not hit.
No GPU."""

import numpy as np
import pytest
import torch
from _mlp_backward_spec import mlp_backward_spec
from _mlp_deep_host_rule import compiler, host_backward, host_forward, load
from _mlp_deep_spec import (DEEP_GRAD_BOUNDS, DEEP_LOGIT_ABS_BOUNDS, NAMES, RELU, TANH, bits32c, deep_backward_spec, deep_init,
                            deep_spec, make_deep_backward_case, make_deep_case)
from _mlp_spec import mlp_spec

F32 = np.float32
L, O, M = 38, 5, 20_000


@pytest.mark.parametrize("act", (TANH, RELU))
@pytest.mark.parametrize("L_, H1, H2, O_", ((7, 16, 32, 5), (5, 48, 16, 6), (3, 64, 64, 1)))
def test_forward_identity_on_the_spec_side(L_, H1, H2, O_, act):
    """deep(x) == mlp(L := H1, H := H2; x := h1, w1t := w2t, b1 := b2, w2 := w3, b2 := b3) with h1 = mlp(x, w1t, b1)'s hidden."""
    c = make_deep_case(61, L_, H1, H2, O_, seed=H1 + H2, adversarial=True)
    y, h1, h2 = deep_spec(c["x"], *(c[n] for n in NAMES), act)
    _, want_h1 = mlp_spec(c["x"], c["w1t"], c["b1"], np.ones((2, H1), F32), np.ones(2, F32), act)
    want_y, want_h2 = mlp_spec(want_h1, c["w2t"], c["b2"], c["w3"], c["b3"], act)
    for got, want in ((y, want_y), (h1, want_h1), (h2, want_h2)):
        np.testing.assert_array_equal(bits32c(got), bits32c(want))
    assert np.isnan(y).any() and np.isfinite(y).any()


@pytest.mark.parametrize("act", (TANH, RELU))
@pytest.mark.parametrize("L_, H1, H2, O_", ((7, 16, 32, 5), (5, 48, 16, 6)))
def test_backward_identities_on_the_spec_side(L_, H1, H2, O_, act):
    """The last two layers are CCX_MLP's backward on (hidden1, hidden2, grad_y, w3); the first is CCX_MLP's rule with
    O := H2 (CCX_MLP_WIDE: the same spec, general in O) on (x, hidden1, grad_a2, w2t transposed)."""
    c = make_deep_backward_case(259, L_, H1, H2, O_, act, seed=H1 + O_)
    got = deep_backward_spec(c["x"], c["hidden1"], c["hidden2"], c["grad_y"], c["w2t"], c["w3"], act)
    last = mlp_backward_spec(c["hidden1"], c["hidden2"], c["grad_y"], c["w3"], act)
    for mine, theirs in (("w2t", "w1t"), ("b2", "b1"), ("w3", "w2"), ("b3", "b2"), ("ga2", "ga")):
        np.testing.assert_array_equal(bits32c(got[mine]), bits32c(last[theirs]), err_msg=mine)
    first = mlp_backward_spec(c["x"], c["hidden1"], got["ga2"], np.ascontiguousarray(c["w2t"].T), act)
    for mine, theirs in (("w1t", "w1t"), ("b1", "b1"), ("ga1", "ga")):
        np.testing.assert_array_equal(bits32c(got[mine]), bits32c(first[theirs]), err_msg=mine)
    for name in NAMES:
        assert np.isfinite(got[name]).all() and got[name].any(), name


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    cxx = compiler()
    if cxx is None:
        pytest.skip("no host C++ compiler (c++, clang++ or ROCm's clang++)")
    return load(cxx, tmp_path_factory.mktemp("mlp_deep_spec"))


def _f64_composition(p, x, gy, act):
    """(y, the six gradients in the kernel's layout) in torch f64 on the same f32 inputs, by autograd."""
    t = {k: torch.tensor(np.asarray(v, np.float64), requires_grad=True) for k, v in p.items()}
    fn = torch.relu if act == RELU else torch.tanh
    h1 = fn(torch.tensor(x.astype(np.float64)) @ t["w1t"] + t["b1"])
    h2 = fn(h1 @ t["w2t"] + t["b2"])
    y = h2 @ t["w3"].t() + t["b3"]
    y.backward(torch.tensor(gy.astype(np.float64)))
    return y.detach().numpy(), {k: t[k].grad.numpy() for k in NAMES}


@pytest.fixture(scope="module", params=((64, 64), (256, 256)), ids=("64-64", "256-256"))
def measured(host, request):
    H1, H2 = request.param
    worst_y, worst = 0.0, dict.fromkeys(NAMES, 0.0)
    for seed, act in ((0, TANH), (1, RELU)):
        p = deep_init(L, H1, H2, O, seed)
        rng = np.random.default_rng(300 + seed)
        x = rng.integers(0, 21, size=(M, L)).astype(F32)                 # observation-like rows: small whole numbers
        gy = rng.standard_normal((M, O)).astype(F32)
        y, h1, h2 = host_forward(host, x, *(p[n] for n in NAMES), act)
        got = host_backward(host, x, h1, h2, gy, p["w2t"], p["w3"], act)
        want_y, want = _f64_composition(p, x, gy, act)
        worst_y = max(worst_y, float(np.abs(y.astype(np.float64) - want_y).max()))
        for name in NAMES:
            err = np.abs(got[name].astype(np.float64) - want[name]) / np.maximum(1.0, np.abs(want[name]))
            worst[name] = max(worst[name], float(err.max()))
    return (H1, H2), worst_y, worst


def test_logits_against_the_f64_composition(measured):
    key, worst, _ = measured
    bound = DEEP_LOGIT_ABS_BOUNDS[key]
    print(f"logits (L = 38, {key[0]}-{key[1]}, O = 5, M = 20000): max |err| against the f64 composition = {worst:.3e} (bound {bound:.1e})")
    assert worst <= bound
    assert bound <= 2.0 * worst * 1.05                                    # the recorded bound is the doubled maximum, no more


def test_gradients_against_the_f64_composition(measured):
    key, _, worst = measured
    bounds = DEEP_GRAD_BOUNDS[key]
    for name in NAMES:
        print(f"grad_{name} (L = 38, {key[0]}-{key[1]}, O = 5, M = 20000): max |err| / max(1, |f64|) = {worst[name]:.3e} "
              f"(bound {bounds[name]:.1e})")
    for name in NAMES:
        assert worst[name] <= bounds[name], name
        assert bounds[name] <= 2.0 * worst[name] * 1.05, name
