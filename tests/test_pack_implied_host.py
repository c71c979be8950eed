"""Host side of the chunk table at implied positions (graph.hip) and the register budgets of the two kernels that read it, without a
GPU.

Layout: on a bin-packed table (source table <= 16 MiB) task k's chunks start at chunk k * stride, stride = the pack capacity in
chunks — 4 on Epinion2, above 4 on the Weibo-shaped graph, whose packs were raised to fit 512 workgroups; a table that
streams from HBM, and any table under SPEX_PACK_IMPLIED=0, keeps the dense layout (stride 0).  The stride is read from the packer's
own SPEX_DEBUG_PACK line, through spex_graph_pack_digest (host only: nothing goes to a device).

Registers (the compiler's resource remarks, as tests/test_bpr_sampler_kernel_resources.py reads them): every d = 64 instantiation of
spmm_chunk_kernel within 64 VGPRs, bpr_fused_last_kernel within 48, none with scratch."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from conftest import REPO

sys.path.insert(0, os.path.join(REPO, "tools"))


def pack_line(capfd, csr, n_cols=None):
    """(stride, chunks, tasks, chunk-table bytes, digest) of the packer's layout for a CSR matrix."""
    from spex_amd import _lib
    lib = _lib.load()
    rowptr, col, val = (np.ascontiguousarray(a, dt) for a, dt in zip(csr, (np.int32, np.int32, np.float32)))
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    d = (ctypes.c_uint64 * 8)()
    capfd.readouterr()
    n_rows = len(rowptr) - 1
    rc = lib.spex_graph_pack_digest(p(rowptr), p(col), p(val), n_rows, n_rows if n_cols is None else n_cols, len(col), d)
    assert rc == 0, lib.spex_last_error()
    err = capfd.readouterr().err
    m = re.search(r"(\d+) tasks = \d+ workgroups, (\d+) chunks .* chunk stride (\d+), chunk table (\d+) bytes", err)
    assert m, err
    print(err.strip())
    return int(m.group(3)), int(m.group(2)), int(m.group(1)), int(m.group(4)), tuple(d)


@pytest.fixture()
def debug_pack(monkeypatch):
    monkeypatch.setenv("SPEX_DEBUG_PACK", "1")
    monkeypatch.delenv("SPEX_PACK_IMPLIED", raising=False)
    return monkeypatch


def epinion2_csr(epinion2):
    from spex_amd.graph import lightgcn_norm_adj
    tr = epinion2["train"]
    return lightgcn_norm_adj(tr[:, 0], tr[:, 1], 3185, 12407)


def weibo_csr():
    from spex_amd.datasets import synthetic_interactions
    from spex_amd.graph import lightgcn_norm_adj
    u, i = synthetic_interactions(6812, 20000, 400000, seed=7, sigma=1.4)
    return lightgcn_norm_adj(u, i, 6811, 20000)


def test_stride_epinion2_is_4_and_switch_restores_dense(epinion2, debug_pack, capfd):
    csr = epinion2_csr(epinion2)
    stride, chunks, tasks, nbytes, dig = pack_line(capfd, csr)
    assert stride == 4 and chunks == 4 * tasks
    debug_pack.setenv("SPEX_PACK_IMPLIED", "0")
    stride0, chunks0, tasks0, nbytes0, dig0 = pack_line(capfd, csr)
    assert stride0 == 0 and tasks0 == tasks and chunks0 <= chunks
    assert dig0[0] != dig[0] and dig0[6] == dig[6]            # task.x moved; the segment tables did not
    print("Epinion2 chunk table bytes: dense", nbytes0, "implied", nbytes)
    debug_pack.setenv("SPEX_PACK_IMPLIED", "1")
    assert pack_line(capfd, csr)[4] == dig


def test_stride_weibo_shape_is_above_4(debug_pack, capfd):
    csr = weibo_csr()
    stride, chunks, tasks, nbytes, _ = pack_line(capfd, csr)
    assert stride in (5, 6) and chunks == stride * tasks and tasks // 16 <= 512
    debug_pack.setenv("SPEX_PACK_IMPLIED", "0")
    stride0, chunks0, tasks0, nbytes0, _ = pack_line(capfd, csr)
    assert stride0 == 0 and tasks0 == tasks
    print("Weibo-shaped chunk table bytes: dense", nbytes0, "implied", nbytes)


def test_hbm_streaming_table_keeps_the_dense_layout(debug_pack, capfd):
    """70 000 columns x 256 B is above 16 MiB: no row ids, adjacent-row packs, stride 0."""
    rng = np.random.default_rng(3)
    n = 70000
    deg = rng.integers(0, 5, n)
    rowptr = np.concatenate([[0], np.cumsum(deg)]).astype(np.int32)
    col = np.concatenate([np.sort(rng.choice(n, k, replace=False)) for k in deg]).astype(np.int32)
    stride, _, _, _, _ = pack_line(capfd, (rowptr, col, np.ones(len(col), np.float32)))
    assert stride == 0


def demangled(names):
    out = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True).stdout.splitlines()
    return [re.sub(r"\(anonymous namespace\)::", "", re.sub(r"^void ", "", n)).split("(")[0] for n in out]


@pytest.mark.parametrize("src,kernel,limit,at_least", [("spmm.hip", "spmm_chunk_kernel<", 64, 18), ("score.hip", "bpr_fused_last_kernel<", 48, 2)])
def test_register_budgets(src, kernel, limit, at_least):
    from kernel_resources import resources
    table = resources(os.path.join(REPO, "spex_amd", "csrc", src))
    assert table, f"no resource remarks for {src}: did it compile?"
    mine = [(n, k) for n, k in zip(demangled([k["name"] for k in table]), table) if n.startswith(kernel)]
    assert len(mine) >= at_least, [n for n, _ in mine]
    for n, k in mine:
        regs = k["VGPRs"] + k.get("AGPRs", 0)
        print(f"{n}: VGPR {k['VGPRs']} AGPR {k.get('AGPRs', 0)} SGPR {k.get('TotalSGPRs', -1)} scratch {k['ScratchSize [bytes/lane]']}")
        assert k["ScratchSize [bytes/lane]"] == 0, f"{n} spills {k['ScratchSize [bytes/lane]']} bytes per lane"
        assert regs <= limit, f"{n}: {regs} registers per lane (limit {limit})"
