"""The kernel behind SPEX_STEP_SPARSE_ADAM, from the compiler's own resource remarks (no GPU needed): adam_rows_kernel (optim.hip)
compiles for gfx950 in both its forms without spilling to scratch and without LDS.  Also: both flag values and the two new symbols
stand in the header and in the binding (tests/test_abi.py then checks their signatures by itself), and the mode added no field to the
step descriptor — its state lives in frontier_counts and in one flag bit."""
import os
import re
import subprocess
import sys

from conftest import REPO

sys.path.insert(0, os.path.join(REPO, "tools"))

SYMBOLS = ("spex_adam_rows_f32", "spex_zero_rows_f32")


def by_name(src):
    from kernel_resources import resources
    table = resources(os.path.join(REPO, "spex_amd", "csrc", src))
    assert table, f"no resource remarks for {src}: did it compile?"
    names = subprocess.run(["c++filt"], input="\n".join(k["name"] for k in table), capture_output=True, text=True, check=True).stdout.splitlines()
    names = [re.sub(r"\(anonymous namespace\)::", "", re.sub(r"^void ", "", n)).split("(")[0] for n in names]
    return list(zip(names, table))


def test_adam_rows_kernel_compiles_without_scratch():
    found = [(n, k) for n, k in by_name("optim.hip") if n.startswith("adam_rows_kernel")]
    assert len(found) == 2, f"optim.hip: expected adam_rows_kernel<true> and <false> (have: {sorted(n for n, _ in by_name('optim.hip'))})"
    for name, k in found:
        lds = k.get("LDS Size [bytes/block]", 0)
        print(f"{name}: VGPR {k['VGPRs']} AGPR {k.get('AGPRs', 0)} SGPR {k.get('TotalSGPRs', -1)} scratch {k['ScratchSize [bytes/lane]']} "
              f"LDS {lds} occupancy {k.get('Occupancy [waves/SIMD]', -1)}")
        assert k["ScratchSize [bytes/lane]"] == 0, f"{name} spills {k['ScratchSize [bytes/lane]']} bytes per lane"
        assert lds == 0, f"{name}: {lds} bytes of LDS, expected none"
        assert k["VGPRs"] + k.get("AGPRs", 0) <= 128, f"{name}: more than 128 registers per lane leaves fewer than four waves per SIMD"


def test_flags_and_symbols_stand_in_header_and_binding():
    from spex_amd import _lib
    header = open(os.path.join(REPO, "include", "spex_hip.h")).read()
    assert re.search(r"SPEX_STEP_SPARSE_ADAM\s*=\s*256\b", header)
    assert re.search(r"SPEX_STEP_GRAD_ROWS_LISTED\s*=\s*512\b", header)
    assert _lib.STEP_SPARSE_ADAM == 256 and _lib.STEP_GRAD_ROWS_LISTED == 512
    for sym in SYMBOLS:
        assert re.search(r"\bint\s+%s\s*\(" % sym, header), f"{sym} is not declared in the header"
        assert sym in _lib.SIGNATURES, f"{sym} is not bound"
    fields = [n for n, _ in _lib.LightGCNStepDesc._fields_]
    assert fields[-1] == "frontier_epoch", "the mode adds no field to the step descriptor"
    assert re.search(r"frontier_epoch;[^}]*}\s*spex_lightgcn_step_t;", header, re.S)
