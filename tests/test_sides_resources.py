"""Register use of the kernels of CCX_SIDES (csrc/ccx_sides.hip and the sides kernel of csrc/ccx_mlp_backward.hip), read from
the code objects inside libccx.so (no GPU needed): the exact number of instantiations, no scratch and no SGPR spills, and no
symbol that a neighbour's resource test would count as its own.  The VGPR counts are printed, not pinned (DESIGN.md records
them)."""

from test_kernel_resources import _kernels

# the substrings by which the other resource tests count their kernels (mangled symbols: namespaces of argument and template
# types included)
TAKEN = ("mlp_", "head_grad_", "sample_kernel", "evaluate_fwd_kernel", "evaluate_bwd_kernel", "gae_kernel", "step_kernel",
         "rollout_kernel", "render_kernel", "reset_obs_kernel", "step_begin_kernel", "step_finish_kernel", "ppo_partial_kernel",
         "ppo_final_kernel", "ppo_bwd_kernel", "moments_partial_kernel", "moments_final_kernel")


def test_sides_kernels_count_scratch_and_sgpr_spills(tmp_path):
    ks = {k: v for k, v in _kernels(tmp_path).items() if "sides_" in k}
    fwd = [k for k in ks if "sides_forward_kernel" in k]
    draw = [k for k in ks if "sides_draw_kernel" in k]
    grad = [k for k in ks if "sides_grad_blocks_kernel" in k]
    # the forward; fused: deterministic / sampled x with / without logp or entropy; the block partials of one group (the final
    # step is CCX_MLP's kernel as it is)
    assert len(fwd) == 1 and len(draw) == 4 and len(grad) == 1 and len(ks) == 6, sorted(ks)
    print({k: v[0] for k, v in ks.items()})
    assert all(v[1] == 0 and v[2] == 0 for v in ks.values()), ks
    assert all(v[0] <= 128 for k, v in ks.items() if k in fwd + draw), ks    # (a workgroup of sixteen waves still fits a CU)
    for name in TAKEN:
        assert not [k for k in ks if name in k], name
