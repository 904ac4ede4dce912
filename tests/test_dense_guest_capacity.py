"""CPU (-m "not gpu"): how many BiLSTM cell workgroups the dense launch of the three-step joint model leaves room for on its CU.

The fp32 dense instantiation (gemm_kernel<1, 3, 4, 1, 0, 2, 2, 1, false>) is launched with DR_SOLO_PAD_BYTES of unused dynamic
LDS, which keeps a second dense workgroup and a fused module off its CU (tests/test_dense_cotenancy_budget.py) and decides how
many 12 KB cell workgroups (lstm_cell_lds_kernel<1>: a ring of 3 stages x 4 KB) may be guests there. GUESTS of them must fit in
both budgets of the CU: 160 KB of LDS, and per SIMD -- one dense wave and one wave of every cell workgroup -- 512 registers,
granted in blocks of 8. From the hipcc -S metadata and the source constant; the text is not searched for any instruction.

GUESTS is FOUR. A pad of 52 KB seats a fifth (46 + 52 + 5 x 12 = 158 KB, 136 + 5 x 72 = 496 registers) and was measured
(profiles/cell_guest_ab.json): alone 447.4 k sites/s against the parent's 447.8 k, and together with the cell waves' issue
priority no better than the priority alone in any pairing (452.3 k against 453.0 k at DS_CELL_PRIO 1 held through the gates) -- dense
keeps the matrix pipe about 89 % busy and a fifth guest only divides what the four already get. The pad stays at 56 KB; the
registers would allow five, the LDS does not."""
import os
import re
import shutil
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIMD_VGPRS = 512      # gfx950: unified VGPR / AGPR file per SIMD lane
GRANULE = 8           # allocation granularity
CU_LDS = 160 * 1024
CELL_LDS = 3 * 1 * 4 * 1024      # the cell launch's dynamic LDS at NT = 1 (launch_lstm_cells: 3 stages x KGS x FR KiB)
GUESTS = 4
DENSE = "gemm_kernel<1, 3, 4, 1, 0, 2, 2, 1, false>"


def granted(vgprs):
    return (vgprs + GRANULE - 1) // GRANULE * GRANULE


def test_four_cell_workgroups_fit_beside_the_dense_workgroup():
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
    dense = [r for n, r in res.items() if DENSE in n]
    cell = [r for n, r in res.items() if "lstm_cell_lds_kernel<1>" in n]
    assert len(dense) == 1 and len(cell) == 1, sorted(res)
    dense, cell = dense[0], cell[0]
    src = open(os.path.join(ROOT, "deepsignal_amd", "csrc", "ds_kernels.hip")).read()
    m = re.search(r"constexpr int DR_SOLO_PAD_BYTES = (\d+) \* 1024;", src)
    assert m, "DR_SOLO_PAD_BYTES not found"
    pad = int(m.group(1)) * 1024
    assert "lstm_cell_lds_kernel<1>, grid, dim3(256), 3 * 1 * 4 * 1024, s, L)" in src      # CELL_LDS is what the launch asks for
    assert cell["static_lds_bytes"] == 0, cell
    lds = dense["static_lds_bytes"] + pad + GUESTS * CELL_LDS
    regs = granted(dense["vgprs"]) + GUESTS * granted(cell["vgprs"])
    print("dense %d B static + %d B pad + %d x %d B = %d B of %d; dense %d VGPRs + %d x cell %d VGPRs -> %d granted of %d"
          % (dense["static_lds_bytes"], pad, GUESTS, CELL_LDS, lds, CU_LDS, dense["vgprs"], GUESTS, cell["vgprs"], regs, SIMD_VGPRS))
    assert lds <= CU_LDS
    assert regs <= SIMD_VGPRS
    # the count above is the launch's real capacity: one guest more does not fit the LDS
    assert lds + CELL_LDS > CU_LDS
    # (the register file would seat the fifth: the pad, not the registers, is what a later change of mind has to move)
    assert regs + granted(cell["vgprs"]) <= SIMD_VGPRS
