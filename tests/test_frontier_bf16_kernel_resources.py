"""The kernel behind SPEX_STEP_FRONTIER | SPEX_STEP_BF16_GATHER, from the compiler's own resource remarks (no GPU needed):
spmm_rowlist_dev_bf16_kernel (spmm_bf16.hip; the body of spmm_rowlist_dev_kernel instantiated for a bf16 table) compiles for gfx950,
does not spill, and keeps the LDS of the 64 task slots, so that two 16-wave workgroups fit a compute unit.  Also: the new symbol stands
in the header and in the binding (tests/test_abi.py then checks its signature by itself), and the descriptor did not grow."""
import os
import re

from conftest import REPO
from test_frontier_kernel_resources import by_name

SYMBOL = "spex_spmm_rowlist_dev_bf16_f32"


def test_bf16_rowlist_kernel_compiles_without_scratch():
    table = by_name("spmm_bf16.hip")
    name = "spmm_rowlist_dev_bf16_kernel"
    assert name in table, f"spmm_bf16.hip: no kernel {name} (have: {sorted(table)})"
    k = table[name]
    lds = k.get("LDS Size [bytes/block]", 0)
    print(f"{name}: VGPR {k['VGPRs']} AGPR {k.get('AGPRs', 0)} SGPR {k.get('TotalSGPRs', -1)} scratch {k['ScratchSize [bytes/lane]']} "
          f"LDS {lds} occupancy {k.get('Occupancy [waves/SIMD]', -1)}")
    assert k["ScratchSize [bytes/lane]"] == 0, f"{name} spills {k['ScratchSize [bytes/lane]']} bytes per lane"
    assert lds <= 64 * 64 * 4 + 64, f"{name}: {lds} bytes of LDS, expected at most {64 * 64 * 4 + 64}"
    assert k["VGPRs"] + k.get("AGPRs", 0) <= 128, f"{name}: a 16-wave workgroup needs <= 128 registers per lane"


def test_symbol_stands_in_header_and_binding_and_the_descriptor_did_not_grow():
    from spex_amd import _lib
    header = open(os.path.join(REPO, "include", "spex_hip.h")).read()
    assert re.search(r"\bint\s+%s\s*\(" % SYMBOL, header), f"{SYMBOL} is not declared in the header"
    assert SYMBOL in _lib.SIGNATURES, f"{SYMBOL} is not bound"
    fields = [n for n, _ in _lib.LightGCNStepDesc._fields_]
    assert fields[-4:] == ["frontier_list", "frontier_stamp", "frontier_counts", "frontier_epoch"], "the combined mode needs no new field"
    assert re.search(r"frontier_epoch;[^}]*}\s*spex_lightgcn_step_t;", header, re.S)
