"""Register use of the CCX_PPO_LOSS kernels (csrc/ccx_ppo_loss.hip), read from the code objects inside libccx.so (no GPU
needed): the exact number of kernels and their instantiations, no scratch and no SGPR spills.  The VGPR count is printed, not
pinned (DESIGN.md records it)."""

from test_kernel_resources import _kernels

OTHERS = ("sample_kernel", "evaluate_fwd_kernel", "evaluate_bwd_kernel", "gae_kernel", "step_kernel", "rollout_kernel",
          "render_kernel", "reset_obs_kernel", "step_begin_kernel", "step_finish_kernel")


def test_ppo_loss_kernels_count_scratch_and_sgpr_spills(tmp_path):
    names = ("ppo_partial_kernel", "ppo_final_kernel", "ppo_bwd_kernel", "moments_partial_kernel", "moments_final_kernel")
    ks = {k: v for k, v in _kernels(tmp_path).items() if any(n in k for n in names)}
    count = {n: len([k for k in ks if n in k]) for n in names}
    assert count == {"ppo_partial_kernel": 2,        # masks or none
                     "ppo_final_kernel": 1,
                     "ppo_bwd_kernel": 5,            # masks or none x (both gradients, grad_logits alone), + grad_values alone
                     "moments_partial_kernel": 1, "moments_final_kernel": 1}, sorted(ks)
    assert not [k for k in ks if any(o in k for o in OTHERS)]            # the other resource tests select by these substrings
    print({k: v[0] for k, v in ks.items()})
    assert all(v[1] == 0 and v[2] == 0 for v in ks.values()), ks
