"""Register use of the CCX_GAE kernels (csrc/ccx_gae.hip), read from the code objects inside libccx.so (no GPU needed): no
scratch and no SGPR spills.  The VGPR count is printed, not pinned (DESIGN.md records it): two register chunks of four
input streams are the design, and at one wave per SIMD occupancy is not what limits the kernel."""

from test_kernel_resources import _kernels


def test_gae_kernels_have_no_scratch_and_no_sgpr_spills(tmp_path):
    ks = {k: v for k, v in _kernels(tmp_path).items() if "gae_kernel" in k}
    assert len(ks) == 4, sorted(ks)                      # with / without final_values x with / without valid
    print({k: v[0] for k, v in ks.items()})
    assert all(v[1] == 0 and v[2] == 0 for v in ks.values()), ks
