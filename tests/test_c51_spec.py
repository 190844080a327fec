"""The NumPy spec of CCX_C51 (tests/_c51_spec.py) against the textbook in torch f64 -- softmax, expected values, masked
argmax, the floor / ceil projection with ``index_add_``, the cross-entropy averaged over the rows that count, autograd -- on
the same inputs; the maxima of |err| / max(1, |f64 value|) are printed and, doubled, are the bounds the header quotes.  And the
identities of the rule that hold exactly.  No GPU."""

import numpy as np
import pytest
import torch
from _c51_spec import (ATOMS, C51_GRAD_BOUND, C51_LOSS_BOUND, C51_PROJ_BOUND, C51_Q_BOUND, C51_ROW_LOSS_BOUND, C51_VARIANTS,
                       EXCLUDED_CAP, c51_args, c51_loss_backward_spec, c51_loss_spec, dist, make_c51_case, q_values_spec, support)
from _qlearn_spec import legal_bits

VMIN, VMAX = -10.0, 10.0
M_ROWS = 3000


def textbook(kw, gamma, vmin=VMIN, vmax=VMAX):
    """(q [M, 5], kstar, near-tie rows, and a closure: valid -> (loss, row_loss, proj, n * grad_logits)), all f64."""
    f64 = torch.float64
    lg = torch.from_numpy(np.nan_to_num(kw["logits"]).astype(np.float64))
    M, _, A = lg.shape
    z = torch.linspace(vmin, vmax, A, dtype=f64)
    dz = (vmax - vmin) / (A - 1)
    a = torch.from_numpy(kw["actions"].astype(np.int64)).clamp(max=4)
    r = torch.from_numpy(np.nan_to_num(kw["reward"]))
    disc = torch.full((M,), float(np.float32(gamma)), dtype=f64) if kw["discount"] is None else \
        torch.from_numpy(np.nan_to_num(kw["discount"]).astype(np.float64))
    cut = torch.from_numpy(kw["done"] != 0) | (disc == 0)
    nt = torch.from_numpy(np.nan_to_num(kw["next_target"]).astype(np.float64))
    sel = nt if kw["next_online"] is None else torch.from_numpy(np.nan_to_num(kw["next_online"]).astype(np.float64))
    legal = torch.from_numpy(legal_bits(kw["masks_next"], (M,)))
    qs = (torch.softmax(sel, -1) * z).sum(-1).masked_fill(~legal, -np.inf)
    top2 = qs.topk(2, -1).values
    near = ((top2[:, 0] - top2[:, 1]) < 1e-4) & ~cut
    kstar = qs.argmax(-1)
    rows = torch.arange(M)
    p = torch.softmax(nt[rows, kstar], -1)
    t = torch.where(cut[:, None], r[:, None].expand(M, A), r[:, None] + disc[:, None] * z[None, :]).clamp(vmin, vmax)
    b = ((t - vmin) / dz).clamp(0, A - 1)
    lo, hi = b.floor(), b.ceil()
    p = torch.where(cut[:, None], torch.full_like(p, 1.0 / A), p)        # (a cut target: any distribution, all of it lands on b(r))
    m = torch.zeros(M, A, dtype=f64)
    m.scatter_add_(1, lo.long(), p * (hi - b + (lo == hi).to(f64)))
    m.scatter_add_(1, hi.long(), p * (b - lo))
    q = (torch.softmax(lg, -1) * z).sum(-1)

    def rest(valid):
        counts = torch.from_numpy(((valid != 0) if valid is not None else np.ones(M, bool)) & (kw["actions"] <= 4))
        x = lg.clone().requires_grad_()
        logp = torch.log_softmax(x[rows, a], -1)
        ce = -(m * logp).sum(-1)
        w = torch.ones(M, dtype=f64) if kw["weights"] is None else torch.from_numpy(np.nan_to_num(kw["weights"]).astype(np.float64))
        n = counts.sum()
        loss = torch.where(counts, w * ce, torch.zeros_like(ce)).sum() / n
        (g,) = torch.autograd.grad(loss, x)
        return float(loss), torch.where(counts, ce, torch.zeros_like(ce)).detach().numpy(), \
            torch.where(counts[:, None], m, torch.zeros_like(m)).numpy(), (g * n).numpy(), counts.numpy()
    return q.numpy(), kstar.numpy(), near.numpy(), rest


def _err(got, want):
    want = np.asarray(want, np.float64)
    return float(np.max(np.abs(np.asarray(got, np.float64) - want) / np.maximum(1.0, np.abs(want)), initial=0.0))


@pytest.mark.parametrize("A", ATOMS)
def test_spec_against_f64(A):
    case = make_c51_case(M_ROWS, A, seed=100 + A, special=False)
    worst = dict(proj=0.0, loss=0.0, row_loss=0.0, q=0.0, grad=0.0)
    left_out = rows_seen = 0
    for variant in C51_VARIANTS:
        kw = c51_args(case, *variant)
        gamma = 0.97
        q64, kstar64, near, rest = textbook(kw, gamma)
        valid = np.ones(M_ROWS, np.uint8) if kw["valid"] is None else kw["valid"]
        counted = (valid != 0) & (kw["actions"] <= 4)
        left_out += int((near & counted).sum())
        rows_seen += int(counted.sum())
        kw2 = dict(kw, valid=np.where(near, 0, valid).astype(np.uint8))
        loss64, rl64, proj64, grad64, counts = rest(kw2["valid"])
        stats, row_loss, proj, t = c51_loss_spec(**kw2, gamma=gamma, vmin=VMIN, vmax=VMAX, details=True) if kw2["discount"] is None \
            else c51_loss_spec(**kw2, vmin=VMIN, vmax=VMAX, details=True)
        live = counts & ~t["cut"]
        assert (t["kstar"][live] == kstar64[live]).all(), "beyond the near ties the two sides choose the same bootstrap action"
        grad = c51_loss_backward_spec(kw2["logits"], kw2["actions"], proj, kw2["valid"], kw2["weights"], stats)
        ok = np.isfinite(kw["logits"]).all((-1, -2))
        worst["q"] = max(worst["q"], _err(q_values_spec(kw["logits"][ok], VMIN, VMAX), q64[ok]))
        worst["proj"] = max(worst["proj"], _err(proj, proj64))
        worst["loss"] = max(worst["loss"], _err(stats[0], loss64))
        worst["row_loss"] = max(worst["row_loss"], _err(row_loss, rl64))
        worst["grad"] = max(worst["grad"], _err(grad.astype(np.float64) * float(stats[6]), grad64))
        assert abs(float(proj[counts].sum(-1).max()) - 1.0) < 1e-5 and abs(float(proj[counts].sum(-1).min()) - 1.0) < 1e-5
    print(f"A = {A}: " + ", ".join(f"{k} {v:.3e}" for k, v in worst.items()) + f"; left out {left_out} of {rows_seen} rows")
    assert left_out <= EXCLUDED_CAP * rows_seen
    assert worst["proj"] <= C51_PROJ_BOUND and worst["loss"] <= C51_LOSS_BOUND and worst["row_loss"] <= C51_ROW_LOSS_BOUND
    assert worst["q"] <= C51_Q_BOUND and worst["grad"] <= C51_GRAD_BOUND


def test_the_bounds_are_the_ones_the_documents_quote():
    from pathlib import Path

    root = Path(__file__).resolve().parent.parent
    for text in ((root / "include" / "ccx.h").read_text(), (root / "README.md").read_text()):
        text = " ".join(text.replace("`", "").replace(" * ", " ").split())
        for name, bound in (("proj", C51_PROJ_BOUND), ("loss", C51_LOSS_BOUND), ("row_loss", C51_ROW_LOSS_BOUND),
                            ("grad_logits (times n)", C51_GRAD_BOUND)):
            assert f"{name} within {bound:.1e}" in text, (name, bound)
        assert f"within {C51_Q_BOUND:.1e}" in text


# ---------------------------------------------------------------------------------------------------------------------
# identities that hold exactly: vmin = -8, vmax = 8, A = 33, dz = 0.5
# ---------------------------------------------------------------------------------------------------------------------
def _exact_case(M=200, seed=9):
    rng = np.random.default_rng(seed)
    A = 33
    lg, nt, no = ((rng.standard_normal((M, 5, A)) * 2.0).astype(np.float32) for _ in range(3))
    kw = dict(logits=lg, actions=rng.integers(0, 5, size=M).astype(np.uint8), reward=np.zeros(M), done=np.zeros(M, np.uint8),
              next_target=nt, next_online=no, masks_next=rng.integers(0, 32, size=M).astype(np.uint8))
    return kw, A


def test_zero_reward_and_unit_discount_project_the_target_onto_itself():
    kw, A = _exact_case()
    dz, z, _ = support(A, -8.0, 8.0)
    assert dz == np.float32(0.5) and z[A - 1] == np.float32(8.0)
    _stats, _rl, proj, t = c51_loss_spec(**kw, gamma=1.0, vmin=-8.0, vmax=8.0, details=True)
    _d, e, S = dist(kw["next_target"][np.arange(len(proj)), t["kstar"]], A)
    p = (e / S[:, None]).astype(np.float32)[:, :A]
    np.testing.assert_array_equal(proj.view(np.uint32), p.view(np.uint32))


def test_unit_reward_shifts_the_target_by_two_atoms():
    kw, A = _exact_case()
    kw["reward"][:] = 1.0
    _stats, _rl, proj, t = c51_loss_spec(**kw, gamma=1.0, vmin=-8.0, vmax=8.0, details=True)
    _d, e, S = dist(kw["next_target"][np.arange(len(proj)), t["kstar"]], A)
    p = (e / S[:, None]).astype(np.float32)[:, :A]
    np.testing.assert_array_equal(proj[:, 2:A - 1].view(np.uint32), p[:, :A - 3].view(np.uint32))
    assert not proj[:, :2].view(np.uint32).any()


def test_rewards_beyond_the_support_put_all_mass_on_the_edge_atom():
    kw, A = _exact_case()
    kw["reward"][::2], kw["reward"][1::2] = 100.0, -100.0
    _stats, _rl, proj, _t = c51_loss_spec(**kw, gamma=0.5, vmin=-8.0, vmax=8.0, details=True)
    assert (np.abs(proj[::2, A - 1] - 1.0) < 1e-6).all() and not proj[::2, :A - 1].any()
    assert (np.abs(proj[1::2, 0] - 1.0) < 1e-6).all() and not proj[1::2, 1:].any()
