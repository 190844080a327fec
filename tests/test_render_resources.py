"""The render kernels' register budget, read from the code objects inside libccx.so the way test_kernel_resources.py
reads them (no GPU needed): no scratch, no spills."""

from test_kernel_resources import _kernels


def test_render_kernels_have_no_scratch_and_no_spills(tmp_path):
    kernels = {name: v for name, v in _kernels(tmp_path).items() if "render_kernel" in name}
    assert len(kernels) == 2, sorted(kernels)          # the state and the compact-row instantiation
    for name, (vgpr, scratch, sgpr_spill) in kernels.items():
        assert scratch == 0 and sgpr_spill == 0, (name, vgpr, scratch, sgpr_spill)
        assert vgpr <= 128, (name, vgpr)
