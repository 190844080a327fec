"""Register use of the CCX_SAMPLE kernels (csrc/ccx_sample.hip), read from the code objects inside libccx.so (no GPU needed):
the exact number of instantiations, no scratch and no SGPR spills.  The VGPR count is printed, not pinned (DESIGN.md records
it): at 19-26 registers it is nowhere near limiting occupancy."""

from test_kernel_resources import _kernels


def test_sample_kernels_count_scratch_and_sgpr_spills(tmp_path):
    ks = {k: v for k, v in _kernels(tmp_path).items() if "sample_kernel" in k}
    assert len(ks) == 8, sorted(ks)                      # mask / no mask x deterministic / sampled x with / without logp or entropy
    print({k: v[0] for k, v in ks.items()})
    assert all(v[1] == 0 and v[2] == 0 for v in ks.values()), ks
