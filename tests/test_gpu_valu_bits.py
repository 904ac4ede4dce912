"""GPU: the fp32 forward computes the BITS it computed before the vector-ALU pass over the fp32 kernels (scalar-base
addressing, hoisted index arithmetic: no MFMA's order, no tile shape and no fma chain was changed, so nothing may move).

tests/golden/valu_parent_bits.npz was recorded once on an MI355X from a build of the commit before that pass
(tests/golden/make_valu_parent_bits.py, whose case list the file carries): `act` and `pred` raw and, for the debug engines
(three-step joint model), the SHA-256 of every debug tap (module1..11, lstm_{fw,bw}_l{0,1,2}, signal_feat, fc1, logits).
The cases reach every instantiation of the fused chain kernel, ragged chain tiles, a cell workgroup with a ragged m-tile and
the masked dense (see the generator's docstring). Equality is exact: no tolerance."""
import json
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
sys.path.insert(0, GOLDEN)
import make_valu_parent_bits as gen  # noqa: E402

_REC = np.load(os.path.join(GOLDEN, "valu_parent_bits.npz"))
_CASES = json.loads(str(_REC["cases"]))


def test_the_record_holds_the_generators_cases():
    assert _CASES == gen.CASES


@pytest.mark.parametrize("index", range(len(_CASES)),
                         ids=["%s-n%d-s%d-%s" % (c["weights"], c["n"], c["signal_len"], c["engine"]) for c in _CASES])
def test_forward_bits_equal_the_parents(index):
    case = _CASES[index]
    got = gen.run_case(case, index)
    want = {k.split("/", 1)[1]: _REC[k] for k in _REC.files if k.startswith(gen.case_key(index) + "/")}
    assert sorted(got) == sorted(want)
    assert len(want) == (2 + 11 + 6 + 3 if case["engine"] == "threestep" else 2)
    moved = [k for k in sorted(want) if got[k].dtype != want[k].dtype or got[k].shape != want[k].shape
             or got[k].tobytes() != want[k].tobytes()]
    if "act" in moved:
        print("act: max |d| = %g" % float(np.abs(got["act"] - want["act"]).max()))
    assert not moved, "%s: these outputs are no longer the parent's bytes: %s" % (case, moved)
