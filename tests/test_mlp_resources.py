"""Register use of the CCX_MLP kernels (csrc/ccx_mlp.hip), read from the code objects inside libccx.so (no GPU needed): the
exact number of instantiations, no scratch and no SGPR spills.  The VGPR counts are printed, not pinned (DESIGN.md records
them): a workgroup has up to 16 waves, and __launch_bounds__(1024) keeps every instantiation within the 128 registers at
which the largest workgroup still fits a CU."""

from test_kernel_resources import _kernels


def test_mlp_kernels_count_scratch_and_sgpr_spills(tmp_path):
    ks = {k: v for k, v in _kernels(tmp_path).items() if "mlp_" in k}
    fwd = [k for k in ks if "mlp_forward_kernel" in k]
    draw = [k for k in ks if "mlp_draw_kernel" in k]
    assert len(fwd) == 1 and len(draw) == 4 and len(ks) == 5, sorted(ks)   # the forward; fused: deterministic / sampled x with / without logp or entropy
    print({k: v[0] for k, v in ks.items()})
    assert all(v[1] == 0 and v[2] == 0 for v in ks.values()), ks
    for name in ("sample_kernel", "evaluate_fwd_kernel", "evaluate_bwd_kernel", "gae_kernel", "step_kernel", "rollout_kernel"):
        assert not [k for k in ks if name in k], name                      # the neighbours' resource tests count by these substrings
