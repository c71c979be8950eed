"""Register / scratch / LDS budget of the exact BPR step's batch kernel (lightgcn_bpr_batch_kernel<PUSH>, three rows per workgroup),
from the compiler's own resource remarks (no GPU needed): both instantiations exist, neither spills to scratch, and each stays inside
the budget of its 1 024-thread launch bounds — 16 waves on a CU's four SIMDs share each SIMD's 512-entry-per-lane register file four
ways: at most 128 VGPRs + AGPRs per lane.  The kernel keeps a segment's 64 gathers, two prefetched push runs and three gradient rows
live at once: a change that holds more would spill, silently, into a slow kernel."""
import os
import re
import subprocess
import sys

from conftest import REPO

sys.path.insert(0, os.path.join(REPO, "tools"))

KERNELS = ("lightgcn_bpr_batch_kernel<false>", "lightgcn_bpr_batch_kernel<true>")


def demangled(names):
    out = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True).stdout.splitlines()
    return [re.sub(r"\(anonymous namespace\)::", "", re.sub(r"^void ", "", n)).split("(")[0] for n in out]


def test_bpr_batch_kernel_instantiations_exist_without_scratch_and_inside_their_budgets():
    from kernel_resources import resources
    table = resources(os.path.join(REPO, "spex_amd", "csrc", "batch.hip"))
    assert table, "no resource remarks for batch.hip: did it compile?"
    by_name = dict(zip(demangled([k["name"] for k in table]), table))
    for name in KERNELS:
        assert name in by_name, f"batch.hip: no instantiation {name} (have: {sorted(n for n in by_name if 'batch' in n)})"
        k = by_name[name]
        used = k["VGPRs"] + k.get("AGPRs", 0)
        print(f"{name}: VGPR {k['VGPRs']} AGPR {k.get('AGPRs', 0)} scratch {k['ScratchSize [bytes/lane]']} LDS {k.get('LDS Size [bytes/block]', 0)}")
        assert k["ScratchSize [bytes/lane]"] == 0, f"{name} spills {k['ScratchSize [bytes/lane]']} bytes per lane"
        assert used <= 128, f"{name}: {used} registers per lane, 128 allowed at 1 024 threads"
        assert k.get("LDS Size [bytes/block]", 0) <= 160 * 1024
