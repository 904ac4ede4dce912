"""CPU (-m "not gpu"): TWO BiLSTM cell waves fit beside TWO fused-module waves in a SIMD's 512-entry register file
("Sharing a CU"). Registers are granted in blocks of 8, so the sum is taken over the rounded-up counts:
2 x 184 + 2 x 72 = 512. The cell kernel's ring is a dynamic LDS allocation (a static one would make hipcc derive the register
budget from the LDS-limited occupancy), and its K loop counts LDS-DMA requests with constant s_waitcnt vmcnt values, which a
spill inside the loop would break: no static LDS, no spills, no scratch."""
import os
import shutil
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIMD_VGPRS = 512      # gfx950: unified VGPR / AGPR file per SIMD lane
GRANULE = 8           # allocation granularity


def granted(vgprs):
    return (vgprs + GRANULE - 1) // GRANULE * GRANULE


def test_two_cell_waves_fit_beside_two_module_waves():
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
    cell = [r for n, r in res.items() if "lstm_cell_lds_kernel<1>" in n]
    assert len(module) == 1 and len(cell) == 1, sorted(res)
    module, cell = module[0], cell[0]
    print("module %d VGPRs, cell %d VGPRs" % (module["vgprs"], cell["vgprs"]))
    assert 2 * granted(module["vgprs"]) + 2 * granted(cell["vgprs"]) <= SIMD_VGPRS, (module, cell)
    assert cell["static_lds_bytes"] == 0, cell
    assert cell["scratch_bytes"] == 0 and cell["vgpr_spills"] == 0 and cell["sgpr_spills"] == 0, cell
