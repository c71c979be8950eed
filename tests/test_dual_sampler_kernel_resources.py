"""The device dual-task path sampler's kernel (sample_dual_paths_kernel<CAP>, one 256-thread workgroup per batch, an instance per
batch capacity CAP = 256 / 1 024 / 4 096) from the compiler's own resource remarks (no GPU needed): every instance compiles for
gfx950 without scratch — the six round keys, the Feistel walk and the binary search stay in registers — and holds in LDS what its
layout needs and no more: the batch's users (int32 [CAP]), the open-addressing table (int32 [2 CAP]), the counts / offsets
(uint32 [CAP]), 256 scan cells and the total."""
import os
import sys

from conftest import REPO
from test_bce_sampler_kernel_resources import demangled

sys.path.insert(0, os.path.join(REPO, "tools"))


def layout_bytes(cap):
    return 4 * cap + 4 * 2 * cap + 4 * cap + 4 * 256 + 4


def test_dual_sampler_kernel_compiles_without_scratch_and_within_its_lds_layout():
    from kernel_resources import resources
    table = resources(os.path.join(REPO, "spex_amd", "csrc", "sampler.hip"))
    assert table, "no resource remarks for sampler.hip: did it compile?"
    by_name = dict(zip(demangled([k["name"] for k in table]), table))
    assert "sample_bce_epoch_kernel" in by_name and "sample_bpr_triples_kernel" in by_name and "sample_negatives_kernel" in by_name
    assert layout_bytes(4096) == 66564
    for cap in (256, 1024, 4096):
        name = f"sample_dual_paths_kernel<{cap}>"
        assert name in by_name, f"sampler.hip: no kernel {name} (have: {sorted(by_name)})"
        k = by_name[name]
        print(f"{name}: VGPR {k['VGPRs']} AGPR {k.get('AGPRs', 0)} SGPR {k.get('TotalSGPRs', -1)} scratch {k['ScratchSize [bytes/lane]']} "
              f"LDS {k.get('LDS Size [bytes/block]', 0)} occupancy {k.get('Occupancy [waves/SIMD]', -1)}")
        assert k["ScratchSize [bytes/lane]"] == 0, f"{name} spills {k['ScratchSize [bytes/lane]']} bytes per lane"
        assert 0 < k.get("LDS Size [bytes/block]", 0) <= layout_bytes(cap), f"{name}: {k.get('LDS Size [bytes/block]', 0)} bytes of LDS"
        # the largest instance must fit a CDNA4 compute unit's 160 KB twice over (two workgroups in flight per CU)
        assert 2 * k["LDS Size [bytes/block]"] <= 160 * 1024
