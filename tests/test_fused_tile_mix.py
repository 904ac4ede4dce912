"""CPU (-m "not gpu"): the tile mix and the budgets of the native fp32 fused inception kernel ("Inside a
fused-module workgroup").

Its 48-channel branches b3b / b4b run channels 0..31 on 32x32x2 tiles and channels 32..47 on 16x16x4 tiles, so that no matrix
cycle goes to padded columns. That is only worth having inside the co-tenancy budget (<= 184 VGPRs, no scratch: two module
waves and two BiLSTM cell waves of <= 72 share a SIMD), and it must not move the other chain kernels, whose source it does not
touch."""
import os
import shutil
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# resource lines of the chain kernels this kernel shares a file (and helper functions) with: (VGPRs, scratch, static LDS)
OTHER_CHAIN_KERNELS = {
    "inception_fused_bf16_kernel<1>": (112, 0, 0), "inception_fused_bf16_kernel<2>": (114, 0, 0), "inception_fused_bf16_kernel<3>": (128, 0, 0),
    "inception_fused_split_kernel<1>": (184, 0, 0), "inception_fused_split_kernel<2>": (200, 0, 0), "inception_fused_split_kernel<3>": (231, 0, 0),
}


@pytest.fixture(scope="module")
def resources():
    if not shutil.which("/opt/rocm/bin/hipcc"):
        pytest.skip("hipcc not available")
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources
    return kernel_resources.kernel_resources()


def _one(res, name):
    hit = [r for n, r in res.items() if name + "(" in n]
    assert len(hit) == 1, (name, sorted(res))
    return hit[0]


def test_fused_fp32_kernel_is_within_the_cotenancy_budget(resources):
    fused = _one(resources, "inception_fused_kernel<3>")
    assert fused["vgprs"] <= 184, fused
    assert fused["scratch_bytes"] == 0 and fused["vgpr_spills"] == 0 and fused["sgpr_spills"] == 0, fused
    cell = _one(resources, "lstm_cell_lds_kernel<1>")
    assert cell["vgprs"] <= 72 and cell["scratch_bytes"] == 0, cell


@pytest.mark.parametrize("tm", [1, 2, 3])
def test_fused_fp32_kernel_runs_its_remainders_on_16_wide_tiles(resources, tm):
    r = _one(resources, "inception_fused_kernel<%d>" % tm)
    assert r["mfma_f32_16x16x4"] > 0 and r["mfma_f32_32x32x2"] > 0, r
    assert r["scratch_bytes"] == 0, r


def test_other_chain_kernels_are_unchanged(resources):
    for name, (vgprs, scratch, lds) in OTHER_CHAIN_KERNELS.items():
        r = _one(resources, name)
        assert (r["vgprs"], r["scratch_bytes"], r["static_lds_bytes"]) == (vgprs, scratch, lds), (name, r)
        assert r["mfma_f32_16x16x4"] == 0 and r["mfma_f32_32x32x2"] == 0, (name, r)      # bf16 MFMAs only
