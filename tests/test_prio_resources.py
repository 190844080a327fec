"""Register use of the kernels of CCX_PRIO (csrc/ccx_prio.hip), read from the code objects inside libccx.so (no GPU needed):
the exact number of instantiations of each kernel, no scratch and no SGPR spills, and names that none of the neighbours'
resource tests counts (``replay_`` among them).  The VGPR counts are printed, not pinned."""

from pathlib import Path

from test_kernel_resources import _kernels

import collectivecrossing_amd

NEIGHBOURS = ("replay_", "sample_kernel", "evaluate_", "gae_kernel", "step_kernel", "rollout_kernel", "render_kernel", "observe_kernel",
              "ppo_", "moments_", "mlp_", "sides_", "head_grad_", "stats_", "q_act_kernel", "td_", "adam_")


def test_prio_kernels_count_scratch_and_sgpr_spills(tmp_path):
    assert (Path(collectivecrossing_amd.__file__).parent / "csrc" / "ccx_prio.hip").exists()
    all_kernels = _kernels(tmp_path)
    names = {"prio_set_kernel": 1, "prio_mark_kernel": 1, "prio_max_kernel": 1,
             "prio_tree_kernel": 2,        # over the leaves (i32) / over a level of nodes (i64)
             "prio_draw_kernel": 1, "prio_count_kernel": 1}
    ks = {k: v for k, v in all_kernels.items() if "prio_" in k}
    for name, count in names.items():
        assert len([k for k in ks if name in k]) == count, (name, sorted(ks))
    assert len(ks) == sum(names.values()), sorted(ks)                    # nothing else carries the prefix
    print({k: v[0] for k, v in ks.items()})
    assert all(v[1] == 0 and v[2] == 0 for v in ks.values()), ks
    for name in NEIGHBOURS:
        assert not [k for k in ks if name in k], name                    # the neighbours' resource tests count by these substrings
