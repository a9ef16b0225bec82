"""Register budget of the built kernels (CPU: reads what the compiler reported while `__graft_entry__.build()` / `python -m odise_amd.build`
compiled csrc/, odise_amd/lib/obj/*.usage).  A main-loop kernel that starts spilling does not fail any numerics test - it silently costs the
step 10 % (round 6: an epilogue variant pushed every dense 256x256 kernel from 241 VGPRs to 256 + 100-230 spilled registers; the step went
79.2 -> 88.1 ms on the same box before anything else showed it).  The budget below is what the tree ships with; raise an entry only with a
same-box bench beside it."""
import re

import pytest

from odise_amd import build as B

# spilled VGPRs allowed per kernel family (regex on the mangled name -> limit); everything not listed must not spill at all
ALLOWED = [
    (r"gemm_pp2_kernelILi256ELi256ELi2ELi2ELb1", 32),   # implicit-GEMM conv form: 24 spilled since round 4
    (r"gemm_pp2_kernelILi512ELi128ELi1ELi2ELb1", 64),
    (r"gemm_pp_kernelILi512ELi128ELi1ELi2ELb1", 32),
    (r"conv3_halo_kernelILi256ELi2", 8),
    (r"conv3_halo4_kernelILi128", 28),
]


def test_no_kernel_spills_beyond_the_budget():
    usage = B.resource_usage()
    if not usage:
        pytest.skip("no .usage files next to the objects: the library was not built by this tree's build.py")
    assert len(usage) > 100, len(usage)
    bad = []
    for name, u in sorted(usage.items()):
        limit = next((lim for pat, lim in ALLOWED if re.search(pat, name)), 0)
        if u.get("vgpr_spill", 0) > limit:
            bad.append((name, u.get("vgprs"), u.get("vgpr_spill"), u.get("scratch"), limit))
    assert not bad, "kernels spilling beyond their budget (name, VGPRs, spilled, scratch bytes, allowed): " + repr(bad)


def test_the_hot_kernels_keep_their_occupancy():
    usage = B.resource_usage()
    if not usage:
        pytest.skip("no .usage files")
    occ = {n: u.get("occupancy") for n, u in usage.items()}
    # two 4-wave halo blocks per CU need <= 256 VGPRs; the tiled attention kernel at d_head 40 runs three waves per SIMD
    assert occ[next(n for n in occ if "conv3_halo4_kernelILi128" in n)] >= 2
    assert occ[next(n for n in occ if re.search(r"attn_kernelILi48E", n))] >= 3
    assert occ[next(n for n in occ if re.search(r"attn_sa_kernelILi80E", n))] >= 2
