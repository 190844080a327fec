"""The accuracy numbers include/ccx.h and the README quote for CCX_MLP_WIDE: the rule of csrc/ccx_mlp_wide.h (compiled for
the host; tests/test_mlp_wide_host_rule.py shows it equal to the NumPy specs) against the f64 compositions of
tests/_mlp_spec.py and tests/_mlp_backward_spec.py on the same f32 inputs, at the shape of a C51 head for the 8-agent batch:
L = 38, H = 64, O = 255, torch.nn.Linear's initial weights, observation-like rows, M = 20 000.  The recorded bounds are the
measured maxima doubled, for the inputs the samples did not hit.  No GPU."""

import numpy as np
import pytest
from _mlp_backward_spec import NAMES
from _mlp_backward_spec import reference_f64 as backward_f64
from _mlp_spec import RELU, TANH, linear_init
from _mlp_spec import reference_f64 as forward_f64
from _mlp_wide_host_rule import compiler, host_backward, host_forward, load

F32 = np.float32
L, H, O, M = 38, 64, 255, 20_000

# max |err| of the logits, absolute; max |err| / max(1, |f64 value|) of the four gradients
WIDE_LOGIT_ABS_BOUND = 4.8e-6
WIDE_GRAD_BOUNDS = dict(w1t=5.3e-4, b1=1.1e-4, w2=1.2e-7, b2=1.14e-7)


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    cxx = compiler()
    if cxx is None:
        pytest.skip("no host C++ compiler (c++, clang++ or ROCm's clang++)")
    return load(cxx, tmp_path_factory.mktemp("mlp_wide_spec"))


@pytest.fixture(scope="module")
def measured(host):
    worst_y, worst = 0.0, dict.fromkeys(NAMES, 0.0)
    for seed, act in ((0, TANH), (1, RELU)):
        w1t, b1, w2, b2 = linear_init(L, H, O, seed)
        rng = np.random.default_rng(300 + seed)
        x = rng.integers(0, 21, size=(M, L)).astype(F32)                 # observation-like rows: small whole numbers
        y, hidden = host_forward(host, x, w1t, b1, w2, b2, act)
        worst_y = max(worst_y, float(np.abs(y.astype(np.float64) - forward_f64(x, w1t, b1, w2, b2, act)).max()))
        gy = rng.standard_normal((M, O)).astype(F32)
        got, want = host_backward(host, x, hidden, gy, w2, act), backward_f64(x, hidden, gy, w2, act)
        for name in NAMES:
            err = np.abs(got[name].astype(np.float64) - want[name]) / np.maximum(1.0, np.abs(want[name]))
            worst[name] = max(worst[name], float(err.max()))
    return worst_y, worst


def test_logits_against_the_f64_composition(measured):
    worst = measured[0]
    print(f"logits (L = 38, H = 64, O = 255, M = 20000): max |err| against the f64 composition = {worst:.3e} (bound {WIDE_LOGIT_ABS_BOUND:.1e})")
    assert worst <= WIDE_LOGIT_ABS_BOUND
    assert WIDE_LOGIT_ABS_BOUND <= 2.0 * worst * 1.05                     # the recorded bound is the doubled maximum, no more


def test_gradients_against_the_f64_composition(measured):
    worst = measured[1]
    for name in NAMES:
        print(f"grad_{name} (L = 38, H = 64, O = 255, M = 20000): max |err| / max(1, |f64|) = {worst[name]:.3e} "
              f"(bound {WIDE_GRAD_BOUNDS[name]:.1e})")
    for name in NAMES:
        assert worst[name] <= WIDE_GRAD_BOUNDS[name], name
        assert WIDE_GRAD_BOUNDS[name] <= 2.0 * worst[name] * 1.05, name
