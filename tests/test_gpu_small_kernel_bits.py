"""GPU: the step's short non-matrix kernels (stem1_kernel, avgpool7_kernel, head_kernel, head_folded_kernel,
gather_inputs_kernel, scatter_outputs_kernel) compute the BITS they computed before they were given an issue priority and lean
bodies ("Guests ask for priority"): the site in a scalar base, 32-bit lane offsets, the stem's shared conv position
carried in a register, 16-byte copies. No sum, fma chain or maximum was reordered, so nothing may move.

tests/golden/small_kernel_parent_bits.npz was recorded once on an MI355X from a build of the commit before that pass
(tests/golden/make_small_kernel_parent_bits.py, whose case list the file carries and whose docstring names what each case is
for): `act` and `pred` raw, and the SHA-256 of the taps stem_pool, signal_feat and logits. Equality is exact: no tolerance.

Beside the record, avgpool7_kernel is held to a statement that needs no GPU build: the engine's own module11 tap, summed in
NumPy float32 from zero over the taps in bounds in ascending order, then one float32 division by their count. And 16 forwards in
flight over four slots are held to a one-slot engine synchronised after each: an issue priority may change who runs first, never
a bit."""
import json
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
sys.path.insert(0, GOLDEN)
import make_small_kernel_parent_bits as gen  # noqa: E402

_REC = np.load(os.path.join(GOLDEN, "small_kernel_parent_bits.npz"))
_CASES = json.loads(str(_REC["cases"]))
_POOL_CASES = [i for i, c in enumerate(_CASES) if "signal_feat" in c["taps"] and not c.get("hostile")]


def test_the_record_holds_the_generators_cases():
    assert _CASES == gen.CASES
    names = [c["name"] for c in _CASES]
    assert names == ["default", "s100", "s90", "s40", "s16", "class3", "no_rnn", "no_cnn", "bf16x3", "folded", "hostile"]


@pytest.mark.parametrize("index", range(len(_CASES)), ids=[c["name"] for c in _CASES])
def test_forward_bits_equal_the_parents(index):
    case = _CASES[index]
    got = gen.run_case(case, index)
    want = {k: _REC[k] for k in _REC.files if k.startswith("c%02d_" % index)}
    assert sorted(got) == sorted(want)
    assert len(want) == len(gen.SIZES) * (2 + len(case["taps"]))
    moved = [k for k in sorted(want) if got[k].dtype != want[k].dtype or got[k].shape != want[k].shape
             or got[k].tobytes() != want[k].tobytes()]
    for k in moved:
        if k.endswith("/act"):
            print("%s: max |d| = %g" % (k, float(np.nanmax(np.abs(got[k] - want[k])))))
    assert not moved, "%s: these outputs are no longer the parent's bytes: %s" % (case["name"], moved)


def test_hostile_rows_keep_their_nan():
    """What the hostile case is for: the all-NaN window leaves stem1_kernel as NaN (a maximum that dropped NaN gave relu(-inf + b)
    = 0 and a finite site), and the +-1e30 row stays finite or infinite by the arithmetic, not by a clamp. The record holds the bytes;
    this holds that the record is of the behaviour meant."""
    index = next(i for i, c in enumerate(_CASES) if c.get("hostile"))
    act = _REC[gen.case_key(index, 33) + "/act"]
    assert np.isnan(act[0]).all()
    assert np.isfinite(act[2:]).all()


def _avgpool7_statement(x):
    """[n, w, ch] float32 -> [n, w * ch]: per output the in-bounds taps wo - 3 .. wo + 3 added one by one from 0.f, ascending, then
    one float32 division by their count"""
    n, w, ch = x.shape
    out = np.empty((n, w, ch), np.float32)
    for wo in range(w):
        acc = np.zeros((n, ch), np.float32)
        cnt = 0
        for wi in range(max(wo - 3, 0), min(wo + 3, w - 1) + 1):
            acc = (acc + x[:, wi, :]).astype(np.float32)
            cnt += 1
        out[:, wo, :] = acc / np.float32(cnt)
    return out.reshape(n, w * ch)


@pytest.mark.parametrize("index", _POOL_CASES, ids=[_CASES[i]["name"] for i in _POOL_CASES])
def test_avgpool7_equals_its_float32_statement(index):
    case = _CASES[index]
    eng = gen.make_engine(case)
    try:
        for n in gen.SIZES:
            feats = gen.features_of(case, index, n)
            eng.run(*(feats[k] for k in gen.KEYS))
            x = eng.intermediate("module11", gen.tap_shape(case, "module11", n))
            got = eng.intermediate("signal_feat", gen.tap_shape(case, "signal_feat", n))
            assert x.dtype == np.float32 and np.isfinite(x).all() and float(np.abs(x).max()) > 0
            want = _avgpool7_statement(x)
            assert got.tobytes() == want.tobytes(), "%s, n = %d: %d of %d outputs differ from the statement, max |d| = %g" % (
                case["name"], n, int((got != want).sum()), got.size, float(np.abs(got - want).max()))
    finally:
        eng.close()


@pytest.mark.parametrize("n", [33, 70])
def test_sixteen_forwards_in_flight_equal_the_synchronised_one_slot_engine(n):
    import torch
    from deepsignal_amd import synth
    forwards = 16
    case = _CASES[0]
    w = gen.weights_of(case)
    feats = synth.synthetic_features(forwards * n, seed=7900 + n, signal_len=case["signal_len"])
    dev = torch.device("cuda", 0)
    d = {k: torch.from_numpy(np.ascontiguousarray(feats[k], np.int32 if k == "kmer" else np.float32)).to(dev) for k in gen.KEYS}

    def run(eng, sync_every):
        act = [torch.full((n, 2), -7.0, dtype=torch.float32, device=dev) for _ in range(forwards)]
        pred = [torch.full((n,), -7, dtype=torch.int32, device=dev) for _ in range(forwards)]
        torch.cuda.synchronize()                  # the engine's streams do not wait for torch's
        for f in range(forwards):
            eng.run_device(n, *(d[k][f * n:(f + 1) * n].data_ptr() for k in gen.KEYS), act[f].data_ptr(), pred[f].data_ptr())
            if sync_every:
                eng.sync()
        eng.sync()
        return [(a.cpu().numpy(), p.cpu().numpy()) for a, p in zip(act, pred)]

    one, four = gen.make_engine(case, slots=1, w=w), gen.make_engine(case, slots=4, w=w)
    try:
        assert four.slots == 4
        want = run(one, True)
        assert all(np.isfinite(a).all() for a, _ in want) and len({a.tobytes() for a, _ in want}) == forwards
        for rep in range(2):
            got = run(four, False)
            moved = [f for f in range(forwards) if got[f][0].tobytes() != want[f][0].tobytes() or got[f][1].tobytes() != want[f][1].tobytes()]
            assert not moved, "n = %d, pass %d: forwards %s differ from the synchronised one-slot engine's bytes" % (n, rep, moved)
    finally:
        one.close()
        four.close()
