"""Register / scratch budget of the wide (d = 128 / 256) instantiations of the batch-sized kernels, from the compiler's own resource
remarks (no GPU needed): every instantiation exists, none spills to scratch, and each stays inside the VGPR budget its launch bounds
imply — a 1 024-thread workgroup is 16 waves on a CU's four SIMDs, i.e. 4 waves sharing a SIMD's 512-entry-per-lane register file:
at most 128 VGPRs + AGPRs per lane; a 256-thread workgroup is one wave per SIMD: the whole file.  The V = 4 batch kernel holds a
segment's gathers 16 rows of 4 registers at a time: a change that keeps more in flight would spill, silently, into a slow kernel."""
import os
import re
import subprocess
import sys

import pytest

from conftest import REPO

sys.path.insert(0, os.path.join(REPO, "tools"))

# kernel (demangled, without arguments) -> threads of its __launch_bounds__
WIDE_KERNELS = {
    "batch.hip": {
        "lightgcn_batch_wide_kernel<false, 2>": 1024, "lightgcn_batch_wide_kernel<false, 4>": 1024,
        "lightgcn_batch_wide_kernel<true, 2>": 1024, "lightgcn_batch_wide_kernel<true, 4>": 1024,
    },
    "rows.hip": {
        "spmm_push_batch_wide_kernel<2>": 256, "spmm_push_batch_wide_kernel<4>": 256,
        "reduce_slots_wide_kernel<2>": 256, "reduce_slots_wide_kernel<4>": 256,
    },
    "spmm.hip": {"spmm_rowlist_wide_kernel<2>": 1024, "spmm_rowlist_wide_kernel<4>": 1024},
}


def vgpr_budget(threads):
    waves_per_simd = -(-(threads // 64) // 4)
    return 512 // waves_per_simd


def demangled(names):
    out = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True).stdout.splitlines()
    return [re.sub(r"\(anonymous namespace\)::", "", re.sub(r"^void ", "", n)).split("(")[0] for n in out]


@pytest.mark.parametrize("src", sorted(WIDE_KERNELS))
def test_wide_instantiations_exist_without_scratch_and_inside_their_vgpr_budget(src):
    from kernel_resources import resources
    table = resources(os.path.join(REPO, "spex_amd", "csrc", src))
    assert table, f"no resource remarks for {src}: did it compile?"
    by_name = dict(zip(demangled([k["name"] for k in table]), table))
    for name, threads in WIDE_KERNELS[src].items():
        assert name in by_name, f"{src}: no instantiation {name} (have: {sorted(n for n in by_name if 'wide' in n)})"
        k = by_name[name]
        used = k["VGPRs"] + k.get("AGPRs", 0)
        print(f"{name}: VGPR {k['VGPRs']} AGPR {k.get('AGPRs', 0)} scratch {k['ScratchSize [bytes/lane]']} LDS {k.get('LDS Size [bytes/block]', 0)}")
        assert k["ScratchSize [bytes/lane]"] == 0, f"{name} spills {k['ScratchSize [bytes/lane]']} bytes per lane"
        assert used <= vgpr_budget(threads), f"{name}: {used} registers per lane, {vgpr_budget(threads)} allowed at {threads} threads"
        assert k.get("LDS Size [bytes/block]", 0) <= 160 * 1024
