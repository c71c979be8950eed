"""The kernels behind SPEX_STEP_FRONTIER_DEEP, from the compiler's own resource remarks (no GPU needed): spmm_push_list_kernel and
spmm_push_list_masked_kernel (rows.hip) and the row-sparse Adam pass with a range of its own for the add term, adam_rows_range_kernel
(optim.hip), compile for gfx950 without scratch, in at most 128 registers per lane and in the LDS their source declares (the push: the
16 task counts of a pass; Adam: none).  They are new kernel NAMES: the kernels the frontier forms had before keep the parent commit's
VGPR / AGPR / SGPR / scratch / LDS figures, recorded in profiles/frontier_deep/kernel_resources.txt ([parent] and [change] tables of
tools/kernel_resources.py).  Also: the new symbol stands in the header and in the binding (tests/test_abi.py then checks its signature
by itself), the flag's value, and the step descriptor's field list is what it was."""
import os
import re
import sys

import pytest

from conftest import REPO
from test_frontier_kernel_resources import by_name

sys.path.insert(0, os.path.join(REPO, "tools"))

NEW = [("rows.hip", "spmm_push_list_kernel", 16 * 4), ("rows.hip", "spmm_push_list_masked_kernel", 16 * 4),
       ("optim.hip", "adam_rows_range_kernel<true>", 0), ("optim.hip", "adam_rows_range_kernel<false>", 0)]
KEPT = [("rows.hip", "spmm_push_rows_kernel"), ("rows.hip", "spmm_push_rows_masked_kernel"), ("rows.hip", "frontier_rows_kernel"),
        ("rows.hip", "frontier_rows_masked_kernel"), ("rows.hip", "frontier_init_kernel"), ("spmm.hip", "spmm_rowlist_dev_kernel"),
        ("spmm.hip", "spmm_rowlist_dev_masked_kernel"), ("spmm_bf16.hip", "spmm_rowlist_dev_bf16_kernel"),
        ("optim.hip", "adam_rows_kernel<true>"), ("optim.hip", "adam_rows_kernel<false>")]
_tables = {}


def table_of(src):
    if src not in _tables:
        _tables[src] = by_name(src)
    return _tables[src]


def recorded(section):
    """name -> (VGPR, AGPR, SGPR, scratch, LDS) of one section of the committed table."""
    text = open(os.path.join(REPO, "profiles", "frontier_deep", "kernel_resources.txt")).read()
    body = re.search(r"\[%s\]\n(.*?)(?=\n\[|\Z)" % section, text, re.S).group(1)
    out = {}
    for ln in body.splitlines():
        m = re.match(r"(\S+)\s+VGPR\s+(\d+) AGPR\s+(\d+) SGPR\s+(\d+) scratch\s+(\d+) LDS\s+(\d+)", ln)
        if m:
            out[m.group(1)] = tuple(int(x) for x in m.groups()[1:])
    return out


def figures(k):
    return (k["VGPRs"], k.get("AGPRs", 0), k.get("TotalSGPRs", -1), k["ScratchSize [bytes/lane]"], k.get("LDS Size [bytes/block]", 0))


@pytest.mark.parametrize("src,name,max_lds", NEW)
def test_new_kernel_compiles_without_scratch(src, name, max_lds):
    table = table_of(src)
    assert name in table, f"{src}: no kernel {name} (have: {sorted(table)})"
    vgpr, agpr, sgpr, scratch, lds = figures(table[name])
    print(f"{name}: VGPR {vgpr} AGPR {agpr} SGPR {sgpr} scratch {scratch} LDS {lds}")
    assert scratch == 0, f"{name} spills {scratch} bytes per lane"
    assert lds <= max_lds, f"{name}: {lds} bytes of LDS, the source declares {max_lds}"
    assert vgpr + agpr <= 128, f"{name}: a 16-wave workgroup needs <= 128 registers per lane"
    assert recorded("change")[name] == (vgpr, agpr, sgpr, scratch, lds), "profiles/frontier_deep/kernel_resources.txt is stale"


@pytest.mark.parametrize("src,name", KEPT)
def test_existing_kernel_keeps_the_parents_resources(src, name):
    parent = recorded("parent")
    assert name in parent, f"{name} is not in the [parent] table"
    got = figures(table_of(src)[name])
    assert got == parent[name], f"{name}: (VGPR, AGPR, SGPR, scratch, LDS) {got}, the parent commit's {parent[name]}"
    assert recorded("change")[name] == got


def test_symbol_and_flag_stand_in_header_and_binding_and_the_descriptor_is_unchanged():
    from spex_amd import _lib
    header = open(os.path.join(REPO, "include", "spex_hip.h")).read()
    sym = "spex_spmm_push_list_f32"
    assert re.search(r"\bint\s+%s\s*\(" % sym, header), f"{sym} is not declared in the header"
    assert sym in _lib.SIGNATURES and len(_lib.SIGNATURES[sym][1]) == 9
    assert re.search(r"SPEX_STEP_FRONTIER_DEEP\s*=\s*1024\b", header) and _lib.STEP_FRONTIER_DEEP == 1024
    fields = [n for n, _ in _lib.LightGCNStepDesc._fields_]
    assert fields[-4:] == ["frontier_list", "frontier_stamp", "frontier_counts", "frontier_epoch"]
    assert re.search(r"frontier_epoch;[^}]*}\s*spex_lightgcn_step_t;", header, re.S)
