"""The two kernels behind SPEX_STEP_FRONTIER, from the compiler's own resource remarks (no GPU needed): frontier_rows_kernel
(rows.hip) and spmm_rowlist_dev_kernel (spmm.hip) compile for gfx950, neither spills to scratch, and the list-driven SpMM keeps the
LDS of its 64 task slots (16 KiB + the 16 task counts) so that two 16-wave workgroups fit a compute unit.  Also: the flag's value and
the new symbols stand in the header and in the binding (tests/test_abi.py then checks their signatures by itself)."""
import os
import re
import subprocess
import sys

import pytest

from conftest import REPO

sys.path.insert(0, os.path.join(REPO, "tools"))

SYMBOLS = ("spex_frontier_rows_i32", "spex_spmm_rowlist_dev_f32", "spex_spmm_push_rows_scaled_f32")


def by_name(src):
    from kernel_resources import resources
    table = resources(os.path.join(REPO, "spex_amd", "csrc", src))
    assert table, f"no resource remarks for {src}: did it compile?"
    names = subprocess.run(["c++filt"], input="\n".join(k["name"] for k in table), capture_output=True, text=True, check=True).stdout.splitlines()
    names = [re.sub(r"\(anonymous namespace\)::", "", re.sub(r"^void ", "", n)).split("(")[0] for n in names]
    return dict(zip(names, table))


@pytest.mark.parametrize("src,name,max_lds", [("rows.hip", "frontier_rows_kernel", 0), ("spmm.hip", "spmm_rowlist_dev_kernel", 64 * 64 * 4 + 64)])
def test_frontier_kernel_compiles_without_scratch(src, name, max_lds):
    table = by_name(src)
    assert name in table, f"{src}: no kernel {name} (have: {sorted(table)})"
    k = table[name]
    lds = k.get("LDS Size [bytes/block]", 0)
    print(f"{name}: VGPR {k['VGPRs']} AGPR {k.get('AGPRs', 0)} SGPR {k.get('TotalSGPRs', -1)} scratch {k['ScratchSize [bytes/lane]']} "
          f"LDS {lds} occupancy {k.get('Occupancy [waves/SIMD]', -1)}")
    assert k["ScratchSize [bytes/lane]"] == 0, f"{name} spills {k['ScratchSize [bytes/lane]']} bytes per lane"
    assert lds <= max_lds, f"{name}: {lds} bytes of LDS, expected at most {max_lds}"
    assert k["VGPRs"] + k.get("AGPRs", 0) <= 128, f"{name}: a 16-wave workgroup needs <= 128 registers per lane"


def test_flag_and_symbols_stand_in_header_and_binding():
    from spex_amd import _lib
    header = open(os.path.join(REPO, "include", "spex_hip.h")).read()
    assert re.search(r"SPEX_STEP_FRONTIER\s*=\s*128\b", header)
    assert _lib.STEP_FRONTIER == 128
    for sym in SYMBOLS:
        assert re.search(r"\bint\s+%s\s*\(" % sym, header), f"{sym} is not declared in the header"
        assert sym in _lib.SIGNATURES, f"{sym} is not bound"
    fields = [n for n, _ in _lib.LightGCNStepDesc._fields_]
    assert fields[-4:] == ["frontier_list", "frontier_stamp", "frontier_counts", "frontier_epoch"], "new descriptor fields go at the end"
    assert re.search(r"frontier_epoch;[^}]*}\s*spex_lightgcn_step_t;", header, re.S)
