"""Register budget of the step kernel's mixed-control instantiations (csrc/ccx_step.hip, POL = true), read from the code
objects inside libccx.so the way test_kernel_resources.py reads them (no GPU needed)."""

import re

from test_kernel_resources import _kernels

# mangled template arguments of ccx::step_kernel: ILi<GLOG>ELb<PAIR>ELb<K1>ELb<ORD>ELb<POL>E
POL = re.compile(r"step_kernelILi(\d)ELb([01])ELb([01])ELb([01])ELb1E")
PLAIN = re.compile(r"step_kernelILi(\d)ELb([01])ELb([01])ELb([01])ELb0E")


def test_mixed_step_kernels_have_no_scratch_and_no_vgpr_spills(tmp_path):
    ks = _kernels(tmp_path)
    pol = {POL.search(k).groups(): v for k, v in ks.items() if POL.search(k)}
    plain = {PLAIN.search(k).groups(): v for k, v in ks.items() if PLAIN.search(k)}
    # 7 lane-group sizes x PAIR x K1 x ORD, once without and once with the policy: policy id and epsilon are run-time values
    assert len(plain) == 56 and len(pol) == 56, (len(plain), len(pol))
    for key, (vgpr, scratch, sgpr_spill) in pol.items():
        assert scratch == 0, (key, vgpr, scratch, sgpr_spill)          # (no scratch = no VGPR spill)
        assert vgpr <= 128, (key, vgpr)
    # SGPR spills, as the build produces them.  The single-step instantiations (K1: ccx_step / step_mixed, the
    # policy-in-the-loop path) spill NOTHING.  The multi-step ones keep 31-44 scalars in VGPR lanes (v_writelane in the
    # prologue): output bases, strides and reward constants that the longer live ranges of the unrolled 16-step action /
    # order bursts push out; the policy's own scalars (mask, policy id, seed words, epsilon) are among them and are read
    # back once per step.
    k1 = {k: v[2] for k, v in pol.items() if k[2] == "1"}
    multi = {k: v[2] for k, v in pol.items() if k[2] == "0"}
    assert len(k1) == 28 and set(k1.values()) == {0}, k1
    assert len(multi) == 28 and max(multi.values()) <= 44, multi
    expect = {"0": (44, 44), "6": (37, 38)}
    for key, spills in multi.items():
        lo, hi = expect.get(key[0], (31, 32))
        assert lo <= spills <= hi, (key, spills)
