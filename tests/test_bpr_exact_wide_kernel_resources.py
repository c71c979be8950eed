"""Register / scratch / LDS budget of the exact BPR step's wide batch kernel (lightgcn_bpr_batch_wide_kernel<PUSH, V>, V = 2 / 4: three
rows per workgroup at d = 128 / 256) and of the Adam pass's L2 form, from the compiler's own resource remarks (no GPU needed): the
four instantiations exist, none spills to scratch, and each stays inside the budget of its 1 024-thread launch bounds — 16 waves on a
CU's four SIMDs share each SIMD's 512-entry-per-lane register file four ways: at most 128 VGPRs + AGPRs per lane — and inside the
64 KB of LDS a workgroup may declare statically.  The wide kernel holds 64 result registers of gathers, the running-sum and E0 rows of
V registers each, two prefetched push runs and three gradient rows of V registers: a change that holds more would spill, silently,
into a slow kernel.
The V = 1 kernel (lightgcn_bpr_batch_kernel<PUSH>) is the same source as before the wide kernel and must compile to the same
figures: 94 / 103 VGPRs and 13 068 bytes of LDS (s_part 12 KB + s_light 768 B + s_norm 12 B).  (DESIGN.md 4.12 quotes 94 / 99 from the
compiler of its day; the figures asserted here are what that unchanged source gives with the compiler that builds the library now —
the commit before the wide kernel compiles to 94 / 103 as well.)  Remarks only: no assembly is inspected."""
import os
import re
import subprocess
import sys

from conftest import REPO

sys.path.insert(0, os.path.join(REPO, "tools"))

WIDE = {"lightgcn_bpr_batch_wide_kernel<false, 2>": 2, "lightgcn_bpr_batch_wide_kernel<true, 2>": 2,
        "lightgcn_bpr_batch_wide_kernel<false, 4>": 4, "lightgcn_bpr_batch_wide_kernel<true, 4>": 4}
NARROW = {"lightgcn_bpr_batch_kernel<false>": 94, "lightgcn_bpr_batch_kernel<true>": 103}


def demangled(names):
    out = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True).stdout.splitlines()
    return [re.sub(r"\(anonymous namespace\)::", "", re.sub(r"^void ", "", n)).split("(")[0] for n in out]


def table_of(src):
    from kernel_resources import resources
    table = resources(os.path.join(REPO, "spex_amd", "csrc", src))
    assert table, f"no resource remarks for {src}: did it compile?"
    return dict(zip(demangled([k["name"] for k in table]), table))


def lds_bytes(V):
    return 4 * (3 * 16 * 64 * V + 3 * 64 * V + 3)           # s_part[3][16][64 V], s_light[3][64 V], s_norm[3]


def test_wide_bpr_batch_kernel_instantiations_exist_without_scratch_and_inside_their_budgets():
    by_name = table_of("batch.hip")
    for name, V in WIDE.items():
        assert name in by_name, f"batch.hip: no instantiation {name} (have: {sorted(n for n in by_name if 'bpr' in n)})"
        k = by_name[name]
        used = k["VGPRs"] + k.get("AGPRs", 0)
        lds = k.get("LDS Size [bytes/block]", 0)
        print(f"{name}: VGPR {k['VGPRs']} AGPR {k.get('AGPRs', 0)} scratch {k['ScratchSize [bytes/lane]']} LDS {lds}")
        assert k["ScratchSize [bytes/lane]"] == 0, f"{name} spills {k['ScratchSize [bytes/lane]']} bytes per lane"
        assert used <= 128, f"{name}: {used} registers per lane, 128 allowed at 1 024 threads"
        assert lds == lds_bytes(V) and lds <= 64 * 1024, f"{name}: {lds} bytes of LDS, expected {lds_bytes(V)}"


def test_narrow_bpr_batch_kernel_compiles_to_the_figures_it_had():
    by_name = table_of("batch.hip")
    for name, vgprs in NARROW.items():
        k = by_name[name]
        print(f"{name}: VGPR {k['VGPRs']} AGPR {k.get('AGPRs', 0)} scratch {k['ScratchSize [bytes/lane]']} LDS {k.get('LDS Size [bytes/block]', 0)}")
        assert k["VGPRs"] == vgprs and k.get("AGPRs", 0) == 0 and k["ScratchSize [bytes/lane]"] == 0
        assert k.get("LDS Size [bytes/block]", 0) == lds_bytes(1)


def test_adam_pass_with_the_l2_form_has_no_scratch():
    by_name = table_of("optim.hip")
    for name in ("adam_kernel<false>", "adam_kernel<true>"):
        assert name in by_name, f"optim.hip: no instantiation {name} (have: {sorted(by_name)})"
        k = by_name[name]
        print(f"{name}: VGPR {k['VGPRs']} scratch {k['ScratchSize [bytes/lane]']}")
        assert k["ScratchSize [bytes/lane]"] == 0 and k["VGPRs"] + k.get("AGPRs", 0) <= 512
