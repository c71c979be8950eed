"""The device NGCF epoch sampler's kernel (sample_ngcf_epoch_kernel, one thread per output slot, 256-thread blocks) from the compiler's
own resource remarks (no GPU needed): it compiles for gfx950, keeps both Feistel walks, the user's six round keys and the two binary
searches in registers — no scratch — uses no LDS (the shuffle's round keys arrive as kernel arguments), and leaves the three existing
samplers' kernels beside it."""
import os
import sys

from conftest import REPO
from test_bce_sampler_kernel_resources import demangled

sys.path.insert(0, os.path.join(REPO, "tools"))


def test_ngcf_sampler_kernel_compiles_without_scratch_or_lds():
    from kernel_resources import resources
    table = resources(os.path.join(REPO, "spex_amd", "csrc", "sampler.hip"))
    assert table, "no resource remarks for sampler.hip: did it compile?"
    by_name = dict(zip(demangled([k["name"] for k in table]), table))
    assert "sample_negatives_kernel" in by_name and "sample_bpr_triples_kernel" in by_name and "sample_bce_epoch_kernel" in by_name
    assert any(n.startswith("sample_dual_paths_kernel") for n in by_name)
    name = "sample_ngcf_epoch_kernel"
    assert name in by_name, f"sampler.hip: no kernel {name} (have: {sorted(by_name)})"
    k = by_name[name]
    print(f"{name}: VGPR {k['VGPRs']} AGPR {k.get('AGPRs', 0)} SGPR {k.get('TotalSGPRs', -1)} scratch {k['ScratchSize [bytes/lane]']} "
          f"LDS {k.get('LDS Size [bytes/block]', 0)} occupancy {k.get('Occupancy [waves/SIMD]', -1)}")
    assert k["ScratchSize [bytes/lane]"] == 0, f"{name} spills {k['ScratchSize [bytes/lane]']} bytes per lane"
    assert k.get("LDS Size [bytes/block]", 0) == 0
    # a latency-bound kernel of table look-ups wants many waves per SIMD: at most 64 registers keeps all eight (its siblings' bound)
    assert k["VGPRs"] + k.get("AGPRs", 0) <= 64, f"{name}: {k['VGPRs'] + k.get('AGPRs', 0)} registers per lane"
