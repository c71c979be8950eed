"""Register / scratch / LDS budgets of the kernels behind SPEX_STEP_BF16_GATHER, from the compiler's own resource remarks (no GPU
needed): the four bf16-source batch kernels of batch_bf16.hip exist, none spills to scratch, and none uses more registers or more
LDS than its fp32 sibling of batch.hip FROM THE SAME BUILD (a segment's 64 gathers sit in 32 packed registers there, so a bf16 kernel
that needs more than the fp32 one has lost the packing); the Adam pass with the bf16 shadow output has no scratch either."""
import os
import re
import subprocess
import sys

import pytest

from conftest import REPO

sys.path.insert(0, os.path.join(REPO, "tools"))

SIBLINGS = {"lightgcn_batch_bf16_kernel<false>": "lightgcn_batch_kernel<false>",
            "lightgcn_batch_bf16_kernel<true>": "lightgcn_batch_kernel<true>",
            "lightgcn_bpr_batch_bf16_kernel<false>": "lightgcn_bpr_batch_kernel<false>",
            "lightgcn_bpr_batch_bf16_kernel<true>": "lightgcn_bpr_batch_kernel<true>"}


def by_name(src):
    from kernel_resources import resources
    table = resources(os.path.join(REPO, "spex_amd", "csrc", src))
    assert table, f"no resource remarks for {src}: did it compile?"
    names = subprocess.run(["c++filt"], input="\n".join(k["name"] for k in table), capture_output=True, text=True, check=True).stdout.splitlines()
    names = [re.sub(r"\(anonymous namespace\)::", "", re.sub(r"^void ", "", n)).split("(")[0] for n in names]
    return dict(zip(names, table))


@pytest.fixture(scope="module")
def tables():
    return by_name("batch_bf16.hip"), by_name("batch.hip")


@pytest.mark.parametrize("name", sorted(SIBLINGS))
def test_bf16_batch_kernel_stays_inside_its_fp32_siblings_budget(tables, name):
    bf16, fp32 = tables
    assert name in bf16, f"batch_bf16.hip: no instantiation {name} (have: {sorted(bf16)})"
    assert SIBLINGS[name] in fp32, f"batch.hip: no instantiation {SIBLINGS[name]}"
    k, s = bf16[name], fp32[SIBLINGS[name]]
    regs = lambda x: x["VGPRs"] + x.get("AGPRs", 0)
    lds = lambda x: x.get("LDS Size [bytes/block]", 0)
    print(f"{name}: VGPR+AGPR {regs(k)} (fp32 sibling {regs(s)}) scratch {k['ScratchSize [bytes/lane]']} LDS {lds(k)} (fp32 sibling {lds(s)})")
    assert k["ScratchSize [bytes/lane]"] == 0, f"{name} spills {k['ScratchSize [bytes/lane]']} bytes per lane"
    assert regs(k) <= regs(s), f"{name}: {regs(k)} registers per lane, its fp32 sibling has {regs(s)}"
    assert lds(k) <= lds(s), f"{name}: {lds(k)} bytes of LDS, its fp32 sibling has {lds(s)}"


def test_adam_pass_with_the_shadow_output_has_no_scratch():
    table = by_name("optim.hip")
    for name in ("adam_shadow_kernel<false>", "adam_shadow_kernel<true>"):
        assert name in table, f"optim.hip: no instantiation {name} (have: {sorted(table)})"
        k = table[name]
        print(f"{name}: VGPR {k['VGPRs']} scratch {k['ScratchSize [bytes/lane]']}")
        assert k["ScratchSize [bytes/lane]"] == 0, f"{name} spills {k['ScratchSize [bytes/lane]']} bytes per lane"
