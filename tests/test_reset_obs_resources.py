"""Register budgets of the CCX_RESET_OBS kernels, read from the code objects inside libccx.so (no GPU needed): the fix-up
kernel (csrc/ccx_reset_obs.hip) and the RSO instantiations of ccx::step_kernel, which are held to the budgets of the
step kernel's other single-step instantiations (tests/test_mixed_control_resources.py)."""

import re

from test_kernel_resources import _kernels


def test_fix_up_kernel_has_no_scratch_and_no_sgpr_spills(tmp_path):
    ks = {k: v for k, v in _kernels(tmp_path).items() if "reset_obs_kernel" in k}
    assert len(ks) == 2, sorted(ks)                      # PAIR: 16-byte units for even agent counts, 8-byte for odd
    assert all(v[1] == 0 and v[2] == 0 for v in ks.values()), ks
    assert max(v[0] for v in ks.values()) <= 64, ks


def test_step_kernel_reset_obs_instantiations_stay_within_the_budget(tmp_path):
    ks = {k: v for k, v in _kernels(tmp_path).items() if "step_kernel" in k}
    # mangled template arguments: ILi<GLOG>ELb<PAIR>ELb<K1>ELb<ORD>ELb<POL>ELb<MSK>ELb<RSO>E
    rso = {k: v for k, v in ks.items() if re.search(r"ILi\dELb[01]ELb1ELb0ELb0ELb[01]ELb1E", k)}
    assert len(rso) == 28, sorted(rso)                   # 7 lane-group sizes x PAIR x MSK
    assert not {k: v for k, v in rso.items() if v[0] > 128 or v[1] != 0 or v[2] != 0}, rso
    # ... and only where the issue asks for them: one env-step, slot order, no scripted policy
    assert not [k for k in ks if re.search(r"ILi\dELb[01]ELb[01]ELb[01]ELb[01]ELb[01]ELb1E", k) and k not in rso]
    # the hot single step and its MSK sibling are still there, without the flag, and no fatter than their RSO siblings
    hot = {k: v for k, v in ks.items() if re.search(r"ILi3ELb1ELb1ELb0ELb0ELb[01]ELb0E", k)}
    sib = {k: v for k, v in rso.items() if "ILi3ELb1E" in k}
    assert len(hot) == 2 and len(sib) == 2 and max(v[0] for v in hot.values()) <= min(v[0] for v in sib.values()), (hot, sib)
