"""Register use of the kernels of CCX_NSTEP (csrc/ccx_nstep.hip, and the discounted TD loss in csrc/ccx_qlearn.hip), read from
the code objects inside libccx.so (no GPU needed): the exact number of instantiations of each kernel, no scratch and no SGPR
spills, and names that none of the neighbours' resource tests counts.  The VGPR counts are printed, not pinned (DESIGN.md
records them)."""

from pathlib import Path

from test_kernel_resources import _kernels

import collectivecrossing_amd

NEIGHBOURS = ("sample_kernel", "evaluate_fwd_kernel", "evaluate_bwd_kernel", "gae_kernel", "step_kernel", "rollout_kernel",
              "render_kernel", "reset_obs_kernel", "step_begin_kernel", "step_finish_kernel", "ppo_", "moments_", "mlp_", "sides_",
              "head_grad_", "stats_", "q_act_kernel", "td_partial_kernel", "td_final_kernel", "td_bwd_kernel", "td_", "adam_",
              "observe_kernel", "replay_", "prio_")


def test_nstep_kernels_count_scratch_and_sgpr_spills(tmp_path):
    assert (Path(collectivecrossing_amd.__file__).parent / "csrc" / "ccx_nstep.hip").exists()
    all_kernels = _kernels(tmp_path)
    names = {"nstep_push_kernel": 1,
             "nstep_cut_kernel": 1,
             "nstep_fetch_kernel": 4,      # draws / reads the caller's indices x 16-byte / 8-byte row stores
             "nstep_draws_kernel": 1,
             "tdn_partial_kernel": 2,      # double-Q or not
             "tdn_bwd_kernel": 2}
    ks = {k: v for k, v in all_kernels.items() if any(n in k for n in names)}
    for name, count in names.items():
        assert len([k for k in ks if name in k]) == count, (name, sorted(ks))
    assert len(ks) == sum(names.values()), sorted(ks)
    print({k: v[0] for k, v in ks.items()})
    assert all(v[1] == 0 and v[2] == 0 for v in ks.values()), ks
    for name in NEIGHBOURS:
        assert not [k for k in ks if name in k], name                    # the neighbours' resource tests count by these substrings
    assert len([k for k in all_kernels if "nstep_" in k or "tdn_" in k]) == len(ks)      # nothing else carries the prefixes


def test_fetch_issues_the_windows_loads_without_a_wait_between_them(tmp_path):
    """What include/ccx.h and DESIGN.md 3.25 say of the fetch, read from the code objects: each of the 16 basic blocks that load
    a step of the window (three byte loads -- cut, done, valid -- and the f64 reward) holds NO ``s_waitcnt vmcnt``: nothing
    loaded is used before the last load of the window has been issued."""
    import re
    import subprocess

    from test_kernel_resources import LLVM

    _kernels(tmp_path)                                                   # (unbundles the code objects into tmp_path)
    seen = 0
    for co in sorted(tmp_path.glob("*.co")):
        if b"nstep_fetch_kernel" not in co.read_bytes():
            continue
        text = subprocess.run([str(LLVM / "llvm-objdump"), "-d", "--symbolize-operands", "--no-show-raw-insn", "--no-leading-addr", str(co)],
                              capture_output=True, text=True).stdout
        for func in re.split(r"\n(?=<_Z[^>]*>:)", text):
            name = re.match(r"<([^>]+)>:", func)
            if not name or "nstep_fetch_kernel" not in name.group(1):
                continue
            blocks = re.split(r"\n<L\d+>:|\n\s*s_cbranch_\w+ [^\n]*|\n\s*s_branch [^\n]*", func)
            steps = [b for b in blocks if b.count("global_load_ubyte") >= 3 and "global_load_dwordx2" in b]
            assert len(steps) == 16, (name.group(1), len(steps))
            waits = [re.findall(r"s_waitcnt vmcnt\(\d+\)", b) for b in steps]
            assert not any(waits), (name.group(1), waits)
            seen += 1
    assert seen == 4
