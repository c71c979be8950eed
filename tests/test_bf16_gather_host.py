"""bf16 gather tables (spmm_bf16.hip), the part that needs no GPU: the four entry points are declared, bound and exported; their
argument validation returns the documented codes before anything touches the device; and the compiled kernels' resources, from the
compiler's own remarks (tools/kernel_resources.py): no scratch in any bf16 instantiation, and no more VGPRs than the fp32 chunk
kernel of the same form (epilogue, edge dropout, row ids) — two gathered bf16 entries share a register, so the bf16 form has no
business needing more."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from conftest import REPO
from spex_amd import _lib

sys.path.insert(0, os.path.join(REPO, "tools"))

HEADER = os.path.join(REPO, "include", "spex_hip.h")
ENTRIES = {"spex_cast_bf16_f32": 4, "spex_spmm_bf16_f32": 11, "spex_propagate_bf16_f32": 7, "spex_propagate_bwd_bf16_f32": 8}
INVALID, UNSUPPORTED = -1, -4


def test_entries_are_declared_bound_and_exported():
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name, n_args in ENTRIES.items():
        m = re.search(r"\bint\s+%s\s*\((.*?)\)\s*;" % name, src, flags=re.S)
        assert m, f"{name} is not declared in include/spex_hip.h"
        assert m.group(1).count(",") + 1 == n_args
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == n_args
        assert hasattr(lib, name), f"libspexhip.so does not export {name}"
    assert _lib.load().spex_version() == 5          # symbols were added, the ABI version stays


@pytest.fixture()
def buf():
    """A 16-byte aligned host buffer to stand for a table: validation must return before anything dereferences it."""
    raw = np.zeros(1024 + 16, np.uint8)
    off = (-raw.ctypes.data) % 16
    keep = raw[off:off + 1024]
    p = lambda k: ctypes.c_void_p(keep.ctypes.data + 256 * k)
    p.keep = raw
    return p


def _err(lib):
    return lib.spex_last_error().decode()


def test_spmm_bf16_validates_before_touching_the_device(buf):
    lib = _lib.load()
    f = lib.spex_spmm_bf16_f32
    # (graph, X16, Y, Y16, add_in, add_div, acc_in, acc_out, acc_div, d, stream) — no handle exists without a device: the checks that
    # need none come first, and each names its cause
    assert f(None, None, buf(1), None, None, 1.0, None, None, 1.0, 64, None) == INVALID and "NULL X16" in _err(lib)
    assert f(None, buf(0), None, None, None, 1.0, None, None, 1.0, 64, None) == INVALID and "no output" in _err(lib)
    assert f(None, buf(0), buf(1), None, None, 1.0, None, None, 1.0, 32, None) == UNSUPPORTED and "d == 64" in _err(lib)
    assert f(None, buf(0), buf(1), None, None, 1.0, None, None, 1.0, 128, None) == UNSUPPORTED
    assert f(None, buf(0), None, buf(0), None, 1.0, None, None, 1.0, 64, None) == INVALID and "alias" in _err(lib)
    assert f(None, buf(0), buf(1), buf(1), None, 1.0, None, None, 1.0, 64, None) == INVALID and "alias" in _err(lib)
    assert f(None, buf(0), None, None, None, 1.0, None, buf(1), 1.0, 64, None) == INVALID and "acc_in" in _err(lib)
    assert f(None, buf(0), None, None, None, 1.0, buf(2), buf(1), 0.0, 64, None) == INVALID and "acc_div" in _err(lib)
    assert f(None, buf(0), buf(1), None, buf(2), 0.0, None, None, 1.0, 64, None) == INVALID and "add_div" in _err(lib)
    unaligned = ctypes.c_void_p(buf(0).value + 2)
    assert f(None, unaligned, buf(1), None, None, 1.0, None, None, 1.0, 64, None) == INVALID and "aligned" in _err(lib)
    assert f(None, buf(0), buf(1), None, buf(2), 1.0, buf(3), buf(3), 1.0, 64, None) == UNSUPPORTED and "one epilogue" in _err(lib)
    assert f(None, buf(0), buf(1), None, None, 1.0, None, None, 1.0, 64, None) == INVALID and "NULL graph" in _err(lib)
    with pytest.raises(_lib.SpexError):
        _lib.call("spex_spmm_bf16_f32", None, None, None, None, None, 1.0, None, None, 1.0, 64, None)


def test_cast_and_propagate_validate_before_touching_the_device(buf):
    lib = _lib.load()
    assert lib.spex_cast_bf16_f32(None, buf(0), 8, None) == INVALID and "NULL" in _err(lib)
    assert lib.spex_cast_bf16_f32(buf(0), None, 8, None) == INVALID
    assert lib.spex_cast_bf16_f32(buf(0), buf(1), -1, None) == INVALID
    assert lib.spex_cast_bf16_f32(buf(0), buf(0), 8, None) == INVALID and "alias" in _err(lib)
    assert lib.spex_cast_bf16_f32(None, None, 0, None) == 0                       # nothing to do, nothing launched
    fwd, bwd = lib.spex_propagate_bf16_f32, lib.spex_propagate_bwd_bf16_f32
    # (graph, E0, mean_out, ws16, L, d, stream)
    assert fwd(None, buf(0), buf(1), buf(2), 3, 32, None) == UNSUPPORTED and "d == 64" in _err(lib)
    assert fwd(None, None, buf(1), buf(2), 3, 64, None) == INVALID and "NULL" in _err(lib)
    assert fwd(None, buf(0), None, buf(2), 3, 64, None) == INVALID
    assert fwd(None, buf(0), buf(1), None, 3, 64, None) == INVALID and "ws16" in _err(lib)
    assert fwd(None, buf(0), buf(0), buf(2), 3, 64, None) == INVALID and "alias" in _err(lib)
    assert fwd(None, buf(0), buf(1), buf(1), 3, 64, None) == INVALID and "alias" in _err(lib)
    assert fwd(None, buf(0), buf(1), buf(2), -1, 64, None) == INVALID
    assert fwd(None, buf(0), buf(1), buf(2), 3, 64, None) == INVALID and "NULL graph" in _err(lib)
    # (graph^T, g_out, grad_E0, ws, ws16, L, d, stream)
    assert bwd(None, buf(0), buf(1), buf(2), buf(3), 3, 256, None) == UNSUPPORTED
    assert bwd(None, None, buf(1), buf(2), buf(3), 3, 64, None) == INVALID and "NULL" in _err(lib)
    assert bwd(None, buf(0), buf(1), None, buf(3), 3, 64, None) == INVALID
    assert bwd(None, buf(0), buf(1), buf(2), None, 3, 64, None) == INVALID
    assert bwd(None, buf(0), buf(0), buf(2), buf(3), 3, 64, None) == INVALID and "alias" in _err(lib)
    assert bwd(None, buf(0), buf(1), buf(1), buf(3), 3, 64, None) == INVALID and "alias" in _err(lib)
    assert bwd(None, buf(0), buf(1), buf(2), buf(2), 3, 64, None) == INVALID and "alias" in _err(lib)
    assert bwd(None, buf(0), buf(1), buf(2), buf(3), 3, 64, None) == INVALID and "NULL graph" in _err(lib)


def test_python_surface_refuses_other_gather_dtypes():
    import torch
    from spex_amd.graph import _gather_bf16
    assert _gather_bf16(None) is False and _gather_bf16(torch.float32) is False and _gather_bf16(torch.bfloat16) is True
    for bad in (torch.float16, torch.float64, "bf16"):
        with pytest.raises(ValueError, match="gather_dtype"):
            _gather_bf16(bad)


def demangled(names):
    out = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True).stdout.splitlines()
    return [re.sub(r"\(anonymous namespace\)::", "", re.sub(r"^void ", "", n)).split("(")[0] for n in out]


def test_bf16_kernels_spill_nothing_and_need_no_more_vgprs_than_the_fp32_form():
    from kernel_resources import resources
    csrc = os.path.join(REPO, "spex_amd", "csrc")
    t16, t32 = resources(os.path.join(csrc, "spmm_bf16.hip")), resources(os.path.join(csrc, "spmm.hip"))
    assert t16 and t32, "no resource remarks: did the files compile?"
    k16, k32 = dict(zip(demangled([k["name"] for k in t16]), t16)), dict(zip(demangled([k["name"] for k in t32]), t32))
    for name, k in k16.items():
        print(f"{name}: VGPR {k['VGPRs']} AGPR {k.get('AGPRs', 0)} scratch {k['ScratchSize [bytes/lane]']}")
        assert k["ScratchSize [bytes/lane]"] == 0, f"{name} spills {k['ScratchSize [bytes/lane]']} bytes per lane"
    for helper in ("cast_bf16_kernel<true>", "cast_bf16_kernel<false>", "spmm_hub_fixup_bf16_kernel"):
        assert helper in k16, sorted(k16)
    b = {False: "false", True: "true"}
    for epi in (0, 1, 2):
        for masked in (False, True):
            for rowids in (False, True):
                mine = k16.get(f"spmm_chunk_bf16_kernel<{epi}, {b[masked]}, {b[rowids]}>")
                assert mine is not None, f"no bf16 instantiation <{epi}, {masked}, {rowids}>"
                # the fp32 form: both hub-fold variants where both are compiled (an unmasked launch always carries the fold) — the
                # bf16 kernel stays at or below the SMALLER of them
                theirs = [k32[n] for n in (f"spmm_chunk_kernel<{epi}, {b[masked]}, {b[rowids]}, {f}>" for f in ("true", "false")) if n in k32]
                assert theirs, f"no fp32 instantiation <{epi}, {masked}, {rowids}, *>"
                budget = min(k["VGPRs"] + k.get("AGPRs", 0) for k in theirs)
                used = mine["VGPRs"] + mine.get("AGPRs", 0)
                assert used <= budget, f"bf16 <{epi}, {masked}, {rowids}>: {used} registers per lane, the fp32 form has {budget}"
                assert mine.get("LDS Size [bytes/block]", 0) == 16 * 64 * 4          # the segment sums, as in the fp32 kernel
