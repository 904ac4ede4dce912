"""GPU: which forwards share a CU, and in what order their waves win issue, never changes a result.

The BiLSTM cell workgroups are guests: they run on CUs that a fused-module or a dense workgroup of ANOTHER forward holds
("Sharing a CU"; two fit beside a module, four beside the dense launch's workgroup: tests/test_dense_guest_capacity.py),
their waves ask for the SIMD's issue priority (DS_CELL_PRIO), and how a SIMD arbitrates between a guest wave and its host
differs from run to run. Every forward's bytes must not: each of 24 forwards
with its own data, pipelined through `submit` / `wait` over 8 and over 2 slots, returns `act` and `pred` byte for byte as the same
data through a one-slot engine of the same library, where no two forwards ever meet.

Engines: fp32, three-step joint model. Sizes: n = 64 (one m-block of the cell kernel), n = 70 (a ragged m-tile), n = 128 (the
smallest batch on the ring dense instantiation and its padded launch). signal_len 128, the shortest of
tests/golden/make_valu_parent_bits.py. Models: the default one, and is_cnn=False -- cells and dense with no inception module
on the GPU. Equality is exact: no tolerance."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

KEYS = ("kmer", "means", "stds", "sanums", "signals")
SIGNAL_LEN = 128
FORWARDS = 24
SIZES = (64, 70, 128)
VARIANTS = {"default": {}, "no_cnn": {"is_cnn": False}}


@pytest.fixture(scope="module", params=sorted(VARIANTS))
def engines(request):
    from deepsignal_amd import weights
    from deepsignal_amd.engine import Engine
    variant = VARIANTS[request.param]
    w = weights.random_weights(seed=7, lstm_bias_std=0.1, signal_len=SIGNAL_LEN, **variant)
    made = {}
    for slots in (1, 2, 8):
        made[slots] = Engine(max_batch=max(SIZES), signal_len=SIGNAL_LEN, slots=slots, precision="fp32", fold_fc=False,
                             fuse_min_tiles=1, **variant)
        made[slots].load_weights(w)
        assert made[slots].slots == slots
    yield request.param, made
    for e in made.values():
        e.close()


def _pipelined(eng, batches):
    """every batch through submit / wait, as many in flight as the engine has slots; results in submission order"""
    out, pending = [], []
    for b in batches:
        if len(pending) == eng.slots:
            out.append(eng.wait(pending.pop(0)))
        pending.append(eng.submit(*b))
    for t in pending:
        out.append(eng.wait(t))
    return out


@pytest.mark.parametrize("n", SIZES)
def test_pipelined_forwards_equal_the_one_slot_engine(engines, n):
    from deepsignal_amd import synth
    name, eng = engines
    feats = synth.synthetic_features(FORWARDS * n, seed=5200 + n, signal_len=SIGNAL_LEN)
    batches = [tuple(feats[k][f * n:(f + 1) * n] for k in KEYS) for f in range(FORWARDS)]
    want = _pipelined(eng[1], batches)
    assert all(np.isfinite(a).all() for a, _ in want)
    # different data per forward really gives different results (a stale or swapped buffer would show)
    assert len({a.tobytes() for a, _ in want}) == FORWARDS
    for slots in (8, 2):
        got = _pipelined(eng[slots], batches)
        moved = [f for f in range(FORWARDS)
                 if got[f][0].tobytes() != want[f][0].tobytes() or got[f][1].tobytes() != want[f][1].tobytes()]
        for f in moved[:3]:
            print("%s n=%d slots=%d forward %d: max |d act| = %g" % (name, n, slots, f, float(np.abs(got[f][0] - want[f][0]).max())))
        assert not moved, "%s, n = %d, %d slots: forwards %s differ from the one-slot engine's bytes" % (name, n, slots, moved)
