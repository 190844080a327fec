"""Register use of the CCX_EVALUATE kernels (csrc/ccx_evaluate.hip), read from the code objects inside libccx.so (no GPU
needed): the exact number of instantiations, no scratch and no SGPR spills.  The VGPR count is printed, not pinned (DESIGN.md
3.13 records it)."""

from test_kernel_resources import _kernels


def test_evaluate_kernels_count_scratch_and_sgpr_spills(tmp_path):
    ks = {k: v for k, v in _kernels(tmp_path).items() if "evaluate_fwd_kernel" in k or "evaluate_bwd_kernel" in k}
    fwd = [k for k in ks if "evaluate_fwd_kernel" in k]
    bwd = [k for k in ks if "evaluate_bwd_kernel" in k]
    assert len(fwd) == 4, sorted(fwd)                    # masks or none x entropy or none
    assert len(bwd) == 6, sorted(bwd)                    # masks or none x (both gradients, grad_logp alone, grad_entropy alone)
    assert not [k for k in ks if "sample_kernel" in k]   # tests/test_sample_resources.py counts the kernels with that name
    print({k: v[0] for k, v in ks.items()})
    assert all(v[1] == 0 and v[2] == 0 for v in ks.values()), ks
