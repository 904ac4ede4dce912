"""CPU (-m "not gpu"): register budget of the step's six short non-matrix kernels ("Guests ask for priority").
They run as guests beside two fused-module waves (<= 184 VGPRs each) and a BiLSTM cell wave (<= 96) per SIMD, or beside the
dense behind the join. A SIMD has 512 registers, granted in blocks of 8:
  * the kernels inside the branches (stem1_kernel<false>, avgpool7_kernel, gather_inputs_kernel) and the output copy must fit the
    512 - 2 x 184 - 96 = 48 registers that company leaves, or their waves wait for a module wave to retire;
  * the two head kernels keep eight waves per SIMD (<= 64).
None may use scratch or spill a vector register (head_folded_kernel parks four scalars in a vector register's lanes, as it
always has: that is not scratch). A change that costs a co-tenant its registers fails here and not in a benchmark."""
import os
import shutil
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

BUDGETS = (("stem1_kernel<false>", 48), ("avgpool7_kernel", 48), ("gather_inputs_kernel", 48), ("scatter_outputs_kernel", 48),
           ("ds::head_kernel", 64), ("head_folded_kernel", 64))


def test_small_kernel_register_budgets(monkeypatch):
    if not shutil.which("/opt/rocm/bin/hipcc"):
        pytest.skip("hipcc not available")
    monkeypatch.setenv("DS_KERNEL_SOURCES", "ds_kernels.hip")
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources
    res = kernel_resources.kernel_resources()
    for name, cap in BUDGETS:
        hit = [r for n, r in res.items() if name in n and "bf16" not in n]
        assert len(hit) == 1, (name, sorted(res))
        r = hit[0]
        assert r["vgprs"] <= cap, (name, r)
        assert r["scratch_bytes"] == 0 and r["vgpr_spills"] == 0, (name, r)
        assert r["sgpr_spills"] <= (4 if name == "head_folded_kernel" else 0), (name, r)
    # head_kernel and head_folded_kernel alone keep static LDS (their 4 x 16 partial sums); stem1's window is dynamic
    assert [r["static_lds_bytes"] for n, r in res.items() if "stem1_kernel<false>" in n] == [0]
