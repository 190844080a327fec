"""Register use of the kernels of CCX_C51 (csrc/ccx_c51.hip), read from the code objects inside libccx.so (no GPU needed): the
exact number of instantiations of each of the four kernels, no scratch and no SGPR spills, and names that none of the
neighbours' resource tests counts.  The VGPR counts are printed, not pinned (DESIGN.md records them)."""

from pathlib import Path

from test_kernel_resources import _kernels

import collectivecrossing_amd

NEIGHBOURS = ("sample_kernel", "evaluate_fwd_kernel", "evaluate_bwd_kernel", "gae_kernel", "step_kernel", "rollout_kernel",
              "render_kernel", "reset_obs_kernel", "step_begin_kernel", "step_finish_kernel", "observe_kernel", "q_act_kernel",
              "ppo_", "moments_", "mlp_", "sides_", "head_grad_", "stats_", "td_", "tdn_", "adam_", "replay_", "prio_", "nstep_",
              "dueling_", "minibatch_")


def test_c51_kernels_count_scratch_and_sgpr_spills(tmp_path):
    assert (Path(collectivecrossing_amd.__file__).parent / "csrc" / "ccx_c51.hip").exists()
    all_kernels = _kernels(tmp_path)
    names = {"c51_q_kernel": 1,
             "c51_partial_kernel": 2,          # double-Q or not
             "c51_final_kernel": 1,
             "c51_bwd_kernel": 1}
    ks = {k: v for k, v in all_kernels.items() if any(n in k for n in names)}
    for name, count in names.items():
        assert len([k for k in ks if name in k]) == count, (name, sorted(ks))
    assert len(ks) == sum(names.values()), sorted(ks)
    print({k: v for k, v in ks.items()})
    assert all(v[1] == 0 and v[2] == 0 for v in ks.values()), ks
    for name in NEIGHBOURS:
        assert not [k for k in ks if name in k], name                    # the neighbours' resource tests count by these substrings
    assert len([k for k in all_kernels if "c51_" in k]) == len(ks)       # nothing else carries the prefix
