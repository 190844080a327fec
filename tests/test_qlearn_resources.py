"""Register use of the kernels of CCX_QLEARN (csrc/ccx_qlearn.hip), read from the code objects inside libccx.so (no GPU
needed): the exact number of instantiations of each of the four kernels, no scratch and no SGPR spills.  The VGPR counts are
printed, not pinned (DESIGN.md records them)."""

from test_kernel_resources import _kernels

NEIGHBOURS = ("sample_kernel", "evaluate_fwd_kernel", "evaluate_bwd_kernel", "gae_kernel", "step_kernel", "rollout_kernel",
              "render_kernel", "reset_obs_kernel", "step_begin_kernel", "step_finish_kernel", "ppo_", "moments_", "mlp_", "sides_",
              "head_grad_", "stats_")


def test_qlearn_kernels_count_scratch_and_sgpr_spills(tmp_path):
    all_kernels = _kernels(tmp_path)
    names = {"q_act_kernel": 4,        # MASK x epsilon present / absent
             "td_partial_kernel": 2,   # double-Q on / off
             "td_final_kernel": 1,
             "td_bwd_kernel": 2}       # double-Q on / off
    ks = {k: v for k, v in all_kernels.items() if any(n in k for n in names)}
    for name, count in names.items():
        assert len([k for k in ks if name in k]) == count, (name, sorted(ks))
    assert len(ks) == sum(names.values()), sorted(ks)
    print({k: v[0] for k, v in ks.items()})
    assert all(v[1] == 0 and v[2] == 0 for v in ks.values()), ks
    for name in NEIGHBOURS:
        assert not [k for k in ks if name in k], name                    # the neighbours' resource tests count by these substrings
