"""Host side of the row heads (graph.hip: head_col / head_val) and the register budget of the kernel that reads them, without a GPU.

Layout, through spex_graph_pack_row_heads (host only: the table spex_graph_create would upload): for every row of the hand-made graph
of tests/test_gpu_row_heads.py and of the golden Epinion2 adjacency, slots r * H .. r * H + min(deg, H) - 1 hold the row's first
entries in CSR order and the rest of the row's H slots hold column 0 / value 0; a table that streams from HBM (source table above
16 MiB), a graph with a row beyond 1 024 entries and any handle under SPEX_ROW_HEADS=0 build none.  The packer's SPEX_DEBUG_PACK line
reports the table's bytes.

Registers, under the flags csrc/Makefile compiles score.hip with: both bpr_fused_last_kernel instantiations within 48 VGPRs, no
scratch, the 14 preloaded dwords kept."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import REPO

CSRC = os.path.join(REPO, "spex_amd", "csrc")

# the hand-made graph (shared with tests/test_gpu_row_heads.py)
DEGS = [0, 1, 3, 15, 16, 17, 63, 64, 65, 128, 130, 200]
N_SPECIAL = len(DEGS)
N_USERS, N_ITEMS = 230, 260


def make_csr(seed=5, link00=False):
    """(rowptr, col, val) of the symmetric bipartite adjacency, users first; special rows' lengths asserted.  link00: user 0 and item 0,
    otherwise without entries, are joined — each the other's only neighbour."""
    from spex_amd.graph import lightgcn_norm_adj
    rng = np.random.default_rng(seed)
    B = np.zeros((N_USERS, N_ITEMS), bool)
    B[N_SPECIAL:, N_SPECIAL:] = rng.random((N_USERS - N_SPECIAL, N_ITEMS - N_SPECIAL)) < 0.03
    for k, d in enumerate(DEGS):
        B[k, N_SPECIAL + rng.choice(N_ITEMS - N_SPECIAL, d, replace=False)] = True     # special user k: d ordinary items
        B[N_SPECIAL + rng.choice(N_USERS - N_SPECIAL, d, replace=False), k] = True     # special item k: d ordinary users
    B[0, 0] = link00
    uu, ii = np.nonzero(B)
    rowptr, col, _ = lightgcn_norm_adj(uu, ii, N_USERS - 1, N_ITEMS)
    deg = np.diff(rowptr)
    assert len(deg) == N_USERS + N_ITEMS and deg.max() <= 1024
    want = [int(link00)] + DEGS[1:]
    assert list(deg[:N_SPECIAL]) == want and list(deg[N_USERS:N_USERS + N_SPECIAL]) == want
    val = rng.uniform(0.05, 1.0, len(col)).astype(np.float32) * rng.choice([-1.0, 1.0], len(col)).astype(np.float32)
    return rowptr, col, val


def row_heads(csr, n_cols=None):
    """(H, head_col[n_rows, H], head_val[n_rows, H]) or (H, None, None) where the packer builds none."""
    from spex_amd import _lib
    lib = _lib.load()
    rowptr, col, val = (np.ascontiguousarray(a, dt) for a, dt in zip(csr, (np.int32, np.int32, np.float32)))
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    n_rows = len(rowptr) - 1
    args = (p(rowptr), p(col), p(val), n_rows, n_rows if n_cols is None else n_cols, len(col))
    n, H = ctypes.c_int64(-1), ctypes.c_int32(0)
    assert lib.spex_graph_pack_row_heads(*args, None, None, 0, ctypes.byref(n), ctypes.byref(H)) == 0, lib.spex_last_error()
    assert H.value in (16, 64)
    if n.value == 0:
        return H.value, None, None
    assert n.value == n_rows * H.value
    hc, hv = np.full(n.value, -7, np.int32), np.full(n.value, np.nan, np.float32)
    assert lib.spex_graph_pack_row_heads(*args, p(hc), p(hv), n.value, ctypes.byref(n), ctypes.byref(H)) == 0, lib.spex_last_error()
    return H.value, hc.reshape(n_rows, H.value), hv.reshape(n_rows, H.value)


def check_layout(csr):
    rowptr, col, val = csr
    H, hc, hv = row_heads(csr)
    assert hc is not None
    deg = np.diff(rowptr)
    for r in range(len(deg)):
        k = min(int(deg[r]), H)
        b = int(rowptr[r])
        assert np.array_equal(hc[r, :k], col[b:b + k]) and np.array_equal(hv[r, :k], np.asarray(val[b:b + k], np.float32)), r
        assert not hc[r, k:].any() and not hv[r, k:].any() and not np.signbit(hv[r, k:]).any(), r
    return H, deg


@pytest.fixture()
def heads_on(monkeypatch):
    monkeypatch.delenv("SPEX_ROW_HEADS", raising=False)
    return monkeypatch


def test_heads_hold_the_csr_prefix_small_graph(heads_on):
    H, deg = check_layout(make_csr())
    assert list(deg[:N_SPECIAL]) == DEGS and list(deg[N_USERS:N_USERS + N_SPECIAL]) == DEGS     # rows on both sides of H and of a chunk
    assert deg.min() == 0 and deg.max() > H


def test_heads_hold_the_csr_prefix_epinion2(epinion2, heads_on, capfd):
    from spex_amd.graph import lightgcn_norm_adj
    tr = epinion2["train"]
    csr = lightgcn_norm_adj(tr[:, 0], tr[:, 1], 3185, 12407)
    heads_on.setenv("SPEX_DEBUG_PACK", "1")
    capfd.readouterr()
    H, deg = check_layout(csr)
    m = re.search(r"row heads (\d+) bytes", capfd.readouterr().err)
    assert m and int(m.group(1)) == len(deg) * H * 8
    print("Epinion2:", len(deg), "rows, H", H, "row heads", m.group(1), "bytes; rows beyond H:", int((deg > H).sum()))


def test_switch_builds_none(heads_on, capfd):
    csr = make_csr()
    heads_on.setenv("SPEX_ROW_HEADS", "0")
    heads_on.setenv("SPEX_DEBUG_PACK", "1")
    capfd.readouterr()
    assert row_heads(csr)[1] is None
    assert "row heads 0 bytes" in capfd.readouterr().err
    heads_on.setenv("SPEX_ROW_HEADS", "1")
    assert row_heads(csr)[1] is not None


def test_hbm_streaming_table_builds_none(heads_on):
    """70 000 columns x 256 B is above 16 MiB (test_pack_implied_host.py's table)."""
    rng = np.random.default_rng(3)
    n = 70000
    deg = rng.integers(0, 5, n)
    rowptr = np.concatenate([[0], np.cumsum(deg)]).astype(np.int32)
    col = np.concatenate([np.sort(rng.choice(n, k, replace=False)) for k in deg]).astype(np.int32)
    assert row_heads((rowptr, col, np.ones(len(col), np.float32)))[1] is None


def test_hub_row_builds_none(heads_on):
    """A row beyond 1 024 entries keeps the step on the whole-graph schedule: no heads."""
    n = 1500
    deg = np.ones(n, np.int64)
    deg[7] = 1100
    rowptr = np.concatenate([[0], np.cumsum(deg)]).astype(np.int32)
    col = np.concatenate([np.arange(k) if k > 1 else [r] for r, k in enumerate(deg)]).astype(np.int32)
    assert row_heads((rowptr, col, np.ones(len(col), np.float32)))[1] is None


def test_fused_kernel_register_budget_with_heads(tmp_path):
    from test_kernarg_preload_host import makefile_flags
    from test_pack_implied_host import demangled
    asm = tmp_path / "score.s"
    r = subprocess.run(["/opt/rocm/bin/hipcc"] + makefile_flags("score.hip") + ["-S", "--cuda-device-only", os.path.join(CSRC, "score.hip"), "-o", str(asm)],
                       capture_output=True, text=True, cwd=CSRC)
    assert r.returncode == 0, r.stderr[-2000:]
    desc, cur = {}, None
    for ln in asm.read_text().splitlines():
        m = re.match(r"\s*\.amdhsa_kernel (\S+)", ln)
        if m:
            cur = desc.setdefault(m.group(1), {})
            continue
        m = re.match(r"\s*\.amdhsa_(user_sgpr_kernarg_preload_length|next_free_vgpr|private_segment_fixed_size|group_segment_fixed_size) (\d+)", ln)
        if m and cur is not None:
            cur[m.group(1)] = int(m.group(2))
    names = list(desc)
    mine = [(n, desc[k]) for n, k in zip(demangled(names), names) if n.startswith("bpr_fused_last_kernel<")]
    assert sorted(n for n, _ in mine) == ["bpr_fused_last_kernel<false>", "bpr_fused_last_kernel<true>"]
    for n, k in mine:
        print(n, k)
        assert k["next_free_vgpr"] <= 48, f"{n}: {k['next_free_vgpr']} registers per lane (limit 48)"
        assert k["private_segment_fixed_size"] == 0, f"{n} spills"
        assert k["user_sgpr_kernarg_preload_length"] == 14, n
        assert k["group_segment_fixed_size"] <= 48 * 1024 + 64, n      # s_seg within 48 KB (+ the loss partials)
