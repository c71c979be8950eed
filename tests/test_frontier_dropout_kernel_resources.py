"""The three kernels behind the frontier steps under edge dropout, from the compiler's own resource remarks (no GPU needed):
frontier_rows_masked_kernel and spmm_push_rows_masked_kernel (rows.hip) and spmm_rowlist_dev_masked_kernel (spmm.hip) compile for
gfx950 without scratch; the masked list SpMM stays in 128 registers per lane and in the LDS of its 64 task slots (16 KiB + the 16 task
counts).  They are new kernel NAMES around the existing bodies: the unmasked kernels' VGPR / SGPR / LDS figures equal the parent
commit's, recorded in profiles/frontier_dropout/kernel_resources.txt ([parent] and [change] tables of tools/kernel_resources.py).
Also: the new symbol stands in the header and in the binding (tests/test_abi.py then checks its signature by itself), and the step
descriptor's field list is what it was."""
import os
import re
import sys

import pytest

from conftest import REPO
from test_frontier_kernel_resources import by_name

sys.path.insert(0, os.path.join(REPO, "tools"))

MASKED = [("rows.hip", "frontier_rows_masked_kernel", 0), ("rows.hip", "spmm_push_rows_masked_kernel", 0),
          ("spmm.hip", "spmm_rowlist_dev_masked_kernel", 64 * 64 * 4 + 64)]
UNMASKED = [("rows.hip", "frontier_rows_kernel"), ("rows.hip", "spmm_push_rows_kernel"), ("rows.hip", "frontier_init_kernel"),
            ("spmm.hip", "spmm_rowlist_dev_kernel"), ("spmm_bf16.hip", "spmm_rowlist_dev_bf16_kernel")]
_tables = {}


def table_of(src):
    if src not in _tables:
        _tables[src] = by_name(src)
    return _tables[src]


def recorded(section):
    """name -> (VGPR, AGPR, SGPR, scratch, LDS) of one section of the committed table."""
    text = open(os.path.join(REPO, "profiles", "frontier_dropout", "kernel_resources.txt")).read()
    body = re.search(r"\[%s\]\n(.*?)(?=\n\[|\Z)" % section, text, re.S).group(1)
    out = {}
    for ln in body.splitlines():
        m = re.match(r"(\S+)\s+VGPR\s+(\d+) AGPR\s+(\d+) SGPR\s+(\d+) scratch\s+(\d+) LDS\s+(\d+)", ln)
        if m:
            out[m.group(1)] = tuple(int(x) for x in m.groups()[1:])
    return out


def figures(k):
    return (k["VGPRs"], k.get("AGPRs", 0), k.get("TotalSGPRs", -1), k["ScratchSize [bytes/lane]"], k.get("LDS Size [bytes/block]", 0))


@pytest.mark.parametrize("src,name,max_lds", MASKED)
def test_masked_kernel_compiles_without_scratch(src, name, max_lds):
    table = table_of(src)
    assert name in table, f"{src}: no kernel {name} (have: {sorted(table)})"
    vgpr, agpr, sgpr, scratch, lds = figures(table[name])
    print(f"{name}: VGPR {vgpr} AGPR {agpr} SGPR {sgpr} scratch {scratch} LDS {lds}")
    assert scratch == 0, f"{name} spills {scratch} bytes per lane"
    assert lds <= max_lds, f"{name}: {lds} bytes of LDS, expected at most {max_lds}"
    assert vgpr + agpr <= 128, f"{name}: a 16-wave workgroup needs <= 128 registers per lane"
    assert recorded("change")[name] == (vgpr, agpr, sgpr, scratch, lds), "profiles/frontier_dropout/kernel_resources.txt is stale"


@pytest.mark.parametrize("src,name", UNMASKED)
def test_unmasked_kernel_keeps_the_parents_resources(src, name):
    parent = recorded("parent")
    assert name in parent, f"{name} is not in the [parent] table"
    got = figures(table_of(src)[name])
    assert got == parent[name], f"{name}: (VGPR, AGPR, SGPR, scratch, LDS) {got}, the parent commit's {parent[name]}"


def test_symbol_stands_in_header_and_binding_and_the_descriptor_is_unchanged():
    from spex_amd import _lib
    header = open(os.path.join(REPO, "include", "spex_hip.h")).read()
    sym = "spex_frontier_rows_masked_i32"
    assert re.search(r"\bint\s+%s\s*\(" % sym, header), f"{sym} is not declared in the header"
    assert sym in _lib.SIGNATURES and _lib.SIGNATURES[sym] == _lib.SIGNATURES["spex_frontier_rows_i32"]
    fields = [n for n, _ in _lib.LightGCNStepDesc._fields_]
    assert fields[-4:] == ["frontier_list", "frontier_stamp", "frontier_counts", "frontier_epoch"]
    assert re.search(r"frontier_epoch;[^}]*}\s*spex_lightgcn_step_t;", header, re.S)
