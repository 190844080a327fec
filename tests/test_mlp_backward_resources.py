"""Register use of the kernels of CCX_MLP's backward pass (csrc/ccx_mlp_backward.hip), read from the code objects inside
libccx.so (no GPU needed): the exact number of kernels, no scratch and no SGPR spills.  The VGPR counts are printed, not
pinned (DESIGN.md records them)."""

from test_kernel_resources import _kernels


def test_head_grad_kernels_count_scratch_and_sgpr_spills(tmp_path):
    ks = {k: v for k, v in _kernels(tmp_path).items() if "head_grad_" in k}
    blocks = [k for k in ks if "head_grad_blocks_kernel" in k]
    final = [k for k in ks if "head_grad_final_kernel" in k]
    assert len(blocks) == 1 and len(final) == 1 and len(ks) == 2, sorted(ks)   # block partials; the final step
    print({k: v[0] for k, v in ks.items()})
    assert all(v[1] == 0 and v[2] == 0 for v in ks.values()), ks
    for name in ("mlp_", "sample_kernel", "step_kernel", "gae_kernel", "evaluate_fwd_kernel", "evaluate_bwd_kernel", "rollout_kernel",
                 "reset_obs_kernel"):
        assert not [k for k in ks if name in k], name                    # the neighbours' resource tests count by these substrings
