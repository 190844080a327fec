"""The split-step kernels' register budget (csrc/ccx_split_step.hip), read from the code objects inside libccx.so the
way test_kernel_resources.py reads them (no GPU needed): no scratch, no SGPR / VGPR spills."""

from test_kernel_resources import _kernels


def test_split_step_kernels_have_no_scratch_and_no_spills(tmp_path):
    kernels = {name: v for name, v in _kernels(tmp_path).items()
               if "step_begin_kernel" in name or "step_finish_kernel" in name}
    # begin, and finish for 16-byte / 8-byte observation row units (even / odd agent counts)
    assert len(kernels) == 3, sorted(kernels)
    assert sum("step_begin_kernel" in n for n in kernels) == 1
    for name, (vgpr, scratch, sgpr_spill) in kernels.items():
        assert scratch == 0 and sgpr_spill == 0, (name, vgpr, scratch, sgpr_spill)
        assert vgpr <= 128, (name, vgpr)      # (no VGPR spill without scratch; a budget that keeps 4 waves per SIMD)
