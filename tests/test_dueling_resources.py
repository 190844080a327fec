"""Register use of the kernels of CCX_DUELING (csrc/ccx_dueling.hip and the fused kernel of csrc/ccx_sides.hip), read from the
code objects inside libccx.so (no GPU needed): the exact number of instantiations, no scratch and no SGPR spills, the fused
kernels within the 128 registers at which a workgroup of sixteen waves still fits a CU, and no symbol that a neighbour's
resource test would count as its own.  The VGPR counts are printed, not pinned (DESIGN.md records them)."""

from test_kernel_resources import _kernels

NEIGHBOURS = ("mlp_", "sides_", "head_grad_", "sample_kernel", "evaluate_fwd_kernel", "evaluate_bwd_kernel", "gae_kernel", "step_kernel",
              "rollout_kernel", "render_kernel", "reset_obs_kernel", "ppo_", "moments_", "stats_", "q_act_kernel", "td_partial_kernel",
              "td_final_kernel", "td_bwd_kernel", "tdn_", "nstep_", "replay_", "prio_", "adam_")


def test_dueling_kernels_count_scratch_and_sgpr_spills(tmp_path):
    all_kernels = _kernels(tmp_path)
    names = {"dueling_fwd_kernel": 1, "dueling_bwd_kernel": 1,
             "obs_q_kernel": 4,          # epsilon present / absent x plain / dueling
             "obs_q_groups_kernel": 4}
    ks = {k: v for k, v in all_kernels.items() if any(n in k for n in names)}
    for name, count in names.items():
        assert len([k for k in ks if name in k]) == count, (name, sorted(ks))
    assert len(ks) == sum(names.values()), sorted(ks)
    print({k: v[0] for k, v in ks.items()})
    assert all(v[1] == 0 and v[2] == 0 for v in ks.values()), ks
    assert all(v[0] <= 128 for k, v in ks.items() if "obs_q_" in k), ks
    for name in NEIGHBOURS:
        assert not [k for k in ks if name in k], name
