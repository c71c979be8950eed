"""Resource budget of bpr_fused_last_kernel (score.hip: the BPR step's last layer inside the BPR launch), from the compiler's own
resource remarks for gfx950 with the Makefile's flags (no GPU needed).

The kernel runs 1 024-thread workgroups — 16 waves, four per SIMD — and is launched as ONE dispatch round of up to two workgroups
per CU (512 workgroups at T = 2 048).  Two workgroups on a CU are eight waves per SIMD sharing its 512-entry-per-lane register
file: at most 64 VGPRs per lane (the kernel asks for that occupancy in its __launch_bounds__, so a version that needs more would
spill instead — hence the scratch check), and two workgroups' segment sums must fit the CU's 160 KB of LDS: static LDS <= 64 KB."""
import os
import re
import subprocess
import sys

from conftest import REPO

sys.path.insert(0, os.path.join(REPO, "tools"))

VGPR_BOUND = 64            # 512 registers per lane and SIMD / 8 waves (two 16-wave workgroups per CU)
LDS_BOUND = 64 * 1024


def demangled(names):
    out = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True).stdout.splitlines()
    return [re.sub(r"\(anonymous namespace\)::", "", re.sub(r"^void ", "", n)).split("(")[0] for n in out]


def test_fused_last_kernel_fits_two_workgroups_per_cu():
    from kernel_resources import resources
    table = resources(os.path.join(REPO, "spex_amd", "csrc", "score.hip"))
    assert table, "no resource remarks for score.hip: did it compile?"
    by_name = dict(zip(demangled([k["name"] for k in table]), table))
    for name in ("bpr_fused_last_kernel<true>", "bpr_fused_last_kernel<false>"):
        assert name in by_name, f"no instantiation {name} (have: {sorted(by_name)})"
        k = by_name[name]
        used = k["VGPRs"] + k.get("AGPRs", 0)
        print(f"{name}: VGPR {k['VGPRs']} AGPR {k.get('AGPRs', 0)} scratch {k['ScratchSize [bytes/lane]']} LDS {k.get('LDS Size [bytes/block]', 0)}")
        assert k["ScratchSize [bytes/lane]"] == 0, f"{name} spills {k['ScratchSize [bytes/lane]']} bytes per lane"
        assert used <= VGPR_BOUND, f"{name}: {used} registers per lane, {VGPR_BOUND} allowed"
        assert 0 < k.get("LDS Size [bytes/block]", 0) <= LDS_BOUND
