"""CPU (-m "not gpu"): the vector-ALU budget of the fp32 forward's matrix kernels ("Vector instructions are
matrix time").

On gfx950 a vector-ALU instruction does not run in the shadow of an fp32 MFMA: it costs its ~4.5 cycles of the datapath the
MFMAs of the same SIMD want. So the fused inception chain addresses global memory as (wave-uniform base in SGPRs,
scalar adds) + (32-bit lane offset) + (immediate), and this test pins, from the gfx950 assembly of
ds_kernels.hip (compiled as tests/test_kernel_resources.py compiles it):

  * structure: no 64-bit vector address arithmetic in any basic block of inception_fused_kernel<1|2|3> that holds 8 or more
    MFMAs -- the P1 chunk blocks, the pooling waves' P1, every P2 unit;
  * the static count of vector-ALU instructions (v_* other than v_mfma_*) of each kernel the pass touched. These kernels have
    no vector work inside a rolled loop, so the static count tracks the issued one. The literals are what the build reaches
    (measured, not chosen); the count of the commit before the pass stands beside each.
A change that brings per-lane pointers or per-chunk index arithmetic back fails here without failing any numerical test."""
import os
import re
import shutil
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"

ADDRESS_OPS_64 = ("v_lshl_add_u64", "v_add_co_u32", "v_addc_co_u32", "v_mad_u64_u32")
MFMA_BLOCK = 8

#                                               now   before the pass
STATIC_VALU = {
    "_ZN2ds22inception_fused_kernelILi1EEEvNS_10FusedChainE": (596, 806),
    "_ZN2ds22inception_fused_kernelILi2EEEvNS_10FusedChainE": (809, 1029),
    "_ZN2ds22inception_fused_kernelILi3EEEvNS_10FusedChainE": (977, 1230),
}


@pytest.fixture(scope="module")
def kernels():
    """mangled name -> list of basic blocks, each a list of instruction lines"""
    if not shutil.which(HIPCC):
        pytest.skip("hipcc not available")
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "k.s")
        subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-Wno-unused-value", "--cuda-device-only", "-S",
                        "-x", "hip", "-o", out, os.path.join(ROOT, "deepsignal_amd", "csrc", "ds_kernels.hip")],
                       check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
        text = open(out).read()
    res = {}
    for m in re.finditer(r"^(_Z\w+):.*?\n(.*?)s_endpgm", text, re.S | re.M):
        blocks = [[]]
        for line in m.group(2).split("\n"):
            line = line.strip()
            if re.match(r"\.LBB\d+_\d+:", line):
                blocks.append([])
            elif line and not line.startswith((";", ".")):
                blocks[-1].append(line)
        res[m.group(1)] = blocks
    return res


def _is_valu(line):
    return line.startswith("v_") and not line.startswith("v_mfma")


@pytest.mark.parametrize("tm", [1, 2, 3])
def test_no_64_bit_vector_address_arithmetic_beside_mfmas(kernels, tm):
    blocks = kernels["_ZN2ds22inception_fused_kernelILi%dEEEvNS_10FusedChainE" % tm]
    hot = [b for b in blocks if sum(l.startswith("v_mfma") for l in b) >= MFMA_BLOCK]
    assert len(hot) >= 20, len(hot)          # 16 P1 chunks + the pooling waves' P1 + the P2 units
    bad = [l for b in hot for l in b if l.split()[0].startswith(ADDRESS_OPS_64)]
    assert not bad, bad


@pytest.mark.parametrize("name", sorted(STATIC_VALU))
def test_static_vector_alu_count(kernels, name):
    now, before = STATIC_VALU[name]
    count = sum(_is_valu(l) for b in kernels[name] for l in b)
    print("%s: %d static vector-ALU instructions (budget %d, %d before the pass)" % (name, count, now, before))
    assert count <= now, (name, count, now)
