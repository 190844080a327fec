"""Register use of the CCX_MLP_DEEP kernels (csrc/ccx_mlp_deep.hip), read from the code objects inside libccx.so (no GPU
needed): the exact number of kernels, no scratch and no SGPR spills, at most 128 VGPRs for the forward kernels -- their
workgroup has up to 16 waves, and that many still fit a CU at 128 registers -- and names that none of the neighbours'
resource tests count."""

from test_kernel_resources import _kernels

NEIGHBOURS = ("mlp_", "wide_", "head_grad_", "sides_", "c51_", "obs_q_", "sample_kernel", "evaluate_", "gae_kernel", "step_kernel",
              "rollout_kernel", "reset_obs_kernel", "minibatch_", "replay_", "prio_", "nstep_", "tdn_")


def test_deep_kernels_count_scratch_and_sgpr_spills(tmp_path):
    ks = {k: v for k, v in _kernels(tmp_path).items() if "deep_" in k}
    fwd = [k for k in ks if "deep_forward_kernel" in k]
    draw = [k for k in ks if "deep_draw_kernel" in k]
    q = [k for k in ks if "deep_q_kernel" in k]
    blocks = [k for k in ks if "deep_grad_blocks_kernel" in k]
    # the forward; its fusion with the draw (DET x STATS) and with the Q choice (EPS x DUEL); the backward's block partials
    assert (len(fwd), len(draw), len(q), len(blocks), len(ks)) == (1, 4, 4, 1, 10), sorted(ks)
    print({k: v[0] for k, v in ks.items()})
    assert all(v[1] == 0 and v[2] == 0 for v in ks.values()), ks
    for k in fwd + draw + q:
        assert ks[k][0] <= 128, (k, ks[k])                                # sixteen waves of the largest workgroup on one CU
    for name in NEIGHBOURS:
        assert not [k for k in ks if name in k], name                    # the neighbours' resource tests count by these substrings
