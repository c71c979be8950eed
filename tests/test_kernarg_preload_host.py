"""Preloaded kernel arguments (csrc/Makefile: spmm.hip and score.hip are compiled with -mllvm -amdgpu-kernarg-preload-count), without
a GPU: under the flags the Makefile gives them, every d = 64 spmm_chunk_kernel instantiation and bpr_fused_last_kernel carries a
non-zero preload length in its kernel descriptor (.amdhsa_user_sgpr_kernarg_preload_length: the leading arguments a wave finds in user
SGPRs), long enough for what its prologue reads — the five chunk-table pointers and four integers of the SpMM, the three index
pointers, rowptr and the three 64-bit bounds of the fused BPR launch: 14 dwords each, all the user SGPRs there are beside the kernarg
pointer — and keeps its register budget (64 / 48 VGPRs, no scratch).  The other translation units keep their flags."""
import os
import re
import subprocess

import pytest

from conftest import REPO

CSRC = os.path.join(REPO, "spex_amd", "csrc")


def makefile_flags(src):
    """The hipcc flags csrc/Makefile compiles `src` with (make -n: nothing is built)."""
    obj = src.replace(".hip", ".o")
    out = subprocess.run(["make", "-C", CSRC, "-n", "-B", obj], capture_output=True, text=True, check=True).stdout
    line = next(ln for ln in out.splitlines() if ln.rstrip().endswith("-o " + obj))
    words = line.split()
    return words[1:words.index("-c")]


def test_only_the_two_files_are_compiled_with_preloading():
    for src in ("graph.hip", "batch.hip", "spmm_bf16.hip"):
        assert not any("kernarg-preload" in f for f in makefile_flags(src)), src
    for src in ("spmm.hip", "score.hip"):
        assert "-amdgpu-kernarg-preload-count=14" in makefile_flags(src), src


@pytest.mark.parametrize("src,kernel,limit,at_least", [("spmm.hip", "spmm_chunk_kernel<", 64, 18), ("score.hip", "bpr_fused_last_kernel<", 48, 2)])
def test_preload_length_and_register_budgets(src, kernel, limit, at_least, tmp_path):
    from test_pack_implied_host import demangled
    asm = tmp_path / (src + ".s")
    r = subprocess.run(["/opt/rocm/bin/hipcc"] + makefile_flags(src) + ["-S", "--cuda-device-only", os.path.join(CSRC, src), "-o", str(asm)],
                       capture_output=True, text=True, cwd=CSRC)
    assert r.returncode == 0, r.stderr[-2000:]
    desc, cur = {}, None
    for ln in asm.read_text().splitlines():
        m = re.match(r"\s*\.amdhsa_kernel (\S+)", ln)
        if m:
            cur = desc.setdefault(m.group(1), {})
            continue
        m = re.match(r"\s*\.amdhsa_(user_sgpr_kernarg_preload_length|next_free_vgpr|private_segment_fixed_size) (\d+)", ln)
        if m and cur is not None:
            cur[m.group(1)] = int(m.group(2))
    names = list(desc)
    mine = [(n, desc[k]) for n, k in zip(demangled(names), names) if n.startswith(kernel)]
    assert len(mine) >= at_least, [n for n, _ in mine]
    for n, k in mine:
        print(n, k)
        assert k["user_sgpr_kernarg_preload_length"] == 14, n        # non-zero, and the whole prologue group (see the module docstring)
        assert k["private_segment_fixed_size"] == 0, f"{n} spills"
        assert k["next_free_vgpr"] <= limit, f"{n}: {k['next_free_vgpr']} registers per lane (limit {limit})"     # (VGPRs + AGPRs)
