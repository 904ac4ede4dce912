"""CPU (-m "not gpu"): the DS_PRECISION_FP16X2 instantiations of the split-operand kernels (ds_split_kernels.inc compiled for
TermsHf2) keep what their three-term twins are held to in tests/test_kernel_resources.py: no scratch, no spill of any kind (the ring
kernels overwrite m0 between one save and one restore and count their LDS-DMA requests with a constant vmcnt: both rest on hipcc
spilling nothing), registers within the waves per SIMD their __launch_bounds__ declare, and no static LDS beside the dynamic ring."""
import os
import shutil
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# kernel -> VGPR cap of its launch bounds: 512 threads x 2 workgroups or 256 threads x 2 = up to 4 / 2 waves per SIMD ... the caps of the
# three-term twins (one workgroup per CU is what the LDS they ask for allows; the unified file holds 512 registers per SIMD lane)
KERNELS = {
    "inception_fused_fp16x2_kernel<1>": 256, "inception_fused_fp16x2_kernel<2>": 256, "inception_fused_fp16x2_kernel<3>": 256,
    "stem23_fp16x2_kernel": 256, "lstm_xproj_fp16x2_kernel": 256, "pack_joint_fp16x2_kernel": 256,
    "lstm_cell_fp16x2_kernel<1, 1, 2, 2>": 128, "lstm_cell_fp16x2_kernel<1, 2, 2, 2>": 256, "lstm_cell_fp16x2_kernel<2, 2, 2, 2>": 256,
    "lstm_cell_fp16x2_kernel<1, 2, 4, 2>": 256, "dense_fp16x2_kernel<1, 3, 4, 1>": 256, "dense_fp16x2_kernel<4, 3, 2, 2>": 512,
}


def test_the_fp16x2_instantiations_do_not_spill_and_fit_their_launch_bounds():
    if not shutil.which("/opt/rocm/bin/hipcc"):
        pytest.skip("hipcc not available")
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources
    res = kernel_resources.kernel_resources()
    for name, cap in KERNELS.items():
        hit = [r for n, r in res.items() if name in n]
        assert len(hit) == 1, (name, sorted(res))
        r = hit[0]
        assert r["scratch_bytes"] == 0 and r["vgpr_spills"] == 0 and r["sgpr_spills"] == 0, (name, r)
        assert r["vgprs"] <= cap, (name, r)
        assert r["static_lds_bytes"] == 0, (name, r)      # all LDS is the dynamic allocation the launcher sizes (<= 160 KiB, checked there)
