"""Register use of the CCX_MLP_WIDE kernels (csrc/ccx_mlp_wide.hip), read from the code objects inside libccx.so (no GPU
needed): the exact number of kernels, no scratch and no SGPR spills, and names that none of the neighbours' resource tests
count.  The VGPR counts are printed, not pinned (DESIGN.md records them): the forward's workgroup has up to 16 waves, and
__launch_bounds__(1024) keeps it within the 128 registers at which that workgroup still fits a CU."""

from test_kernel_resources import _kernels

NEIGHBOURS = ("mlp_", "head_grad_", "sides_", "c51_", "obs_q_", "sample_kernel", "evaluate_", "gae_kernel", "step_kernel", "rollout_kernel",
              "reset_obs_kernel", "minibatch_", "replay_", "prio_", "nstep_", "tdn_")


def test_wide_kernels_count_scratch_and_sgpr_spills(tmp_path):
    ks = {k: v for k, v in _kernels(tmp_path).items() if "wide_" in k}
    fwd = [k for k in ks if "wide_forward_kernel" in k]
    blocks = [k for k in ks if "wide_grad_blocks_kernel" in k]
    assert len(fwd) == 1 and len(blocks) == 1 and len(ks) == 2, sorted(ks)   # the forward; the backward's block partials
    print({k: v[0] for k, v in ks.items()})
    assert all(v[1] == 0 and v[2] == 0 for v in ks.values()), ks
    assert ks[fwd[0]][0] <= 128, ks                                       # sixteen waves of the largest workgroup on one CU
    for name in NEIGHBOURS:
        assert not [k for k in ks if name in k], name                    # the neighbours' resource tests count by these substrings
