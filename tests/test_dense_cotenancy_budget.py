"""CPU (-m "not gpu"): the resource budget of the fp32 dense instantiation -- gemm_kernel<1, 3, 4, 1, 0, 2, 2, 1, false>, the
6032 x 6032 layer of the three-step joint model -- whose K loop (dense_ring_loop) takes its weights through an LDS ring.

What the numbers guard: the loop counts LDS-DMA requests and inline-asm loads with constant s_waitcnt vmcnt values, and the
registers those loads land in are known to hipcc as written from the moment the load is issued -- a spill or scratch access inside
the loop would break both, so none is allowed. The VGPR and static-LDS bounds are the ones under which a dense workgroup COULD
share a CU with a fused inception module workgroup (one dense wave and two module waves in a SIMD's 512-entry
register file, registers granted in blocks of 8; 49 KB of the 160 KB of LDS beside a module's 111). That placement is available
but NOT enabled: launched that way the pipelined step was measured slower than the parent's (profiles/EXPERIMENTS.md), so
launch_gemm adds DR_SOLO_PAD_BYTES of unused dynamic LDS and keeps one dense workgroup per CU. The second test holds the launch
to that: static + dynamic LDS leave no room for a module or a second dense workgroup, and do leave room for BiLSTM cell workgroups.
Counts only; the text is not searched for any instruction."""
import functools
import os
import shutil
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIMD_VGPRS = 512      # gfx950: unified VGPR / AGPR file per SIMD lane
GRANULE = 8           # allocation granularity
DENSE = "gemm_kernel<1, 3, 4, 1, 0, 2, 2, 1, false>"


def granted(vgprs):
    return (vgprs + GRANULE - 1) // GRANULE * GRANULE


@functools.lru_cache(maxsize=None)      # one hipcc -S run for both tests
def _resources():
    if not shutil.which("/opt/rocm/bin/hipcc"):
        pytest.skip("hipcc not available")
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources
    old = os.environ.get("DS_KERNEL_SOURCES")
    os.environ["DS_KERNEL_SOURCES"] = "ds_kernels.hip"      # both kernels live in this file
    try:
        res = kernel_resources.kernel_resources()
    finally:
        if old is None:
            del os.environ["DS_KERNEL_SOURCES"]
        else:
            os.environ["DS_KERNEL_SOURCES"] = old
    module = [r for n, r in res.items() if "inception_fused_kernel<3>" in n]
    dense = [r for n, r in res.items() if DENSE in n]
    assert len(module) == 1 and len(dense) == 1, sorted(res)
    return module[0], dense[0]


def test_a_dense_wave_fits_beside_two_module_waves():
    module, dense = _resources()
    print("module %d VGPRs, dense %d VGPRs, %d B of static LDS" % (module["vgprs"], dense["vgprs"], dense["static_lds_bytes"]))
    assert dense["vgprs"] <= 152, dense
    assert dense["static_lds_bytes"] <= 49152, dense
    assert dense["scratch_bytes"] == 0 and dense["vgpr_spills"] == 0 and dense["sgpr_spills"] == 0, dense
    assert 2 * granted(module["vgprs"]) + granted(dense["vgprs"]) <= SIMD_VGPRS, (module, dense)


def test_the_launch_keeps_one_dense_workgroup_per_cu():
    """static LDS + the launch's pad (DR_SOLO_PAD_BYTES in ds_kernels.hip): no second dense workgroup and no fused module
    (111 KB at the headline's tiles, 105 KB at the least) beside it, four cell workgroups of 12 KB do fit."""
    import re
    _, dense = _resources()
    src = open(os.path.join(ROOT, "deepsignal_amd", "csrc", "ds_kernels.hip")).read()
    m = re.search(r"constexpr int DR_SOLO_PAD_BYTES = (\d+) \* 1024;", src)
    assert m, "DR_SOLO_PAD_BYTES not found"
    pad = int(m.group(1)) * 1024
    assert "dim3(256), DR_SOLO_PAD_BYTES, s, d_launch)" in src      # the dense launch passes it
    total, cu = dense["static_lds_bytes"] + pad, 160 * 1024
    print("dense launch: %d B of LDS per workgroup" % total)
    assert 2 * total > cu                       # one per CU
    assert total + 105 * 1024 > cu              # never beside a fused-module workgroup
    assert total + 4 * 12 * 1024 <= cu          # four BiLSTM cell workgroups beside it
