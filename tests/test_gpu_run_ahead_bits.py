"""GPU: a forward's BiLSTM branch runs on the slot's event stream with no launch of its own forward in front of it, so it
starts while EARLIER forwards' joint models still run ("Streams"). What keeps a slot's buffers safe is then one
explicit edge, the event stream's wait for the slot's previous forward (ds_engine.cpp, fork_event_stream). These tests hold the
results to the bytes of an engine in which no two forwards ever meet: one slot, synchronised after every forward.

Geometry and models as tests/test_gpu_cell_guest_bits.py: max_batch 128, n = 64 / 70 / 128, signal_len 128, the default model and
is_cnn=False; is_rnn=False beside them (no event branch: nothing may be forked or joined). Equality is exact: no tolerance."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

KEYS = ("kmer", "means", "stds", "sanums", "signals")
SIGNAL_LEN = 128
FORWARDS = 32
SIZES = (64, 70, 128)
MAX_BATCH = max(SIZES)
VARIANTS = {"default": {}, "no_cnn": {"is_cnn": False}, "no_rnn": {"is_rnn": False}}
# (model, precision, folded joint model): fp32 three-step and folded on every model; one case each of the two 16-bit modes
CASES = [(v, "fp32", fold) for v in sorted(VARIANTS) for fold in (False, True)] + [("default", "bf16_all", False), ("default", "bf16x3", False)]


def _weights(variant):
    from deepsignal_amd import weights
    return weights.random_weights(seed=7, lstm_bias_std=0.1, signal_len=SIGNAL_LEN, **VARIANTS[variant])


def _engine(w, variant, precision, fold, slots, signal_len=SIGNAL_LEN):
    from deepsignal_amd.engine import Engine
    eng = Engine(max_batch=MAX_BATCH, signal_len=signal_len, slots=slots, precision=precision, fold_fc=fold, fuse_min_tiles=1,
                 **VARIANTS[variant])
    eng.load_weights(w)
    assert eng.slots == slots
    return eng


def _to_device(torch, feats):
    dev = torch.device("cuda", 0)
    return {k: torch.from_numpy(np.ascontiguousarray(feats[k], np.int32 if k == "kmer" else np.float32)).to(dev) for k in KEYS}


class _DeviceBatches:
    """`count` input batches of n sites in device memory, and one output pair per forward, so that forwards in flight never
    share a byte of caller memory."""

    def __init__(self, feats, n, count, forwards=None):
        import torch
        self.n, self.count = n, count
        self.d = _to_device(torch, {k: feats[k][:count * n] for k in KEYS})
        self.forwards = forwards if forwards is not None else list(range(count))      # forward f takes batch forwards[f]
        self.torch = torch

    def run(self, eng, sync_every):
        torch, n = self.torch, self.n
        dev = torch.device("cuda", 0)
        act = [torch.full((n, 2), -7.0, dtype=torch.float32, device=dev) for _ in self.forwards]
        pred = [torch.full((n,), -7, dtype=torch.int32, device=dev) for _ in self.forwards]
        torch.cuda.synchronize()                  # the engine's streams do not wait for torch's
        for f, b in enumerate(self.forwards):
            eng.run_device(n, *(self.d[k][b * n:(b + 1) * n].data_ptr() for k in KEYS), act[f].data_ptr(), pred[f].data_ptr())
            if sync_every:
                eng.sync()
        eng.sync()
        return [(a.cpu().numpy(), p.cpu().numpy()) for a, p in zip(act, pred)]


def _moved(got, want):
    return [f for f in range(len(want)) if got[f][0].tobytes() != want[f][0].tobytes() or got[f][1].tobytes() != want[f][1].tobytes()]


@pytest.fixture(scope="module", params=CASES, ids=lambda c: "%s-%s-%s" % (c[0], c[1], "folded" if c[2] else "three_step"))
def engines(request):
    variant, precision, fold = request.param
    w = _weights(variant)
    made = {slots: _engine(w, variant, precision, fold, slots) for slots in (1, 2, 4, 8)}
    yield request.param, made
    for e in made.values():
        e.close()


@pytest.mark.parametrize("n", SIZES)
def test_forwards_in_flight_equal_the_synchronised_one_slot_engine(engines, n):
    from deepsignal_amd import synth
    case, eng = engines
    feats = synth.synthetic_features(FORWARDS * n, seed=6100 + n, signal_len=SIGNAL_LEN)
    batches = _DeviceBatches(feats, n, FORWARDS)
    want = batches.run(eng[1], sync_every=True)
    assert all(np.isfinite(a).all() for a, _ in want)
    # different data per forward really gives different results (a stale or swapped buffer would show)
    assert len({a.tobytes() for a, _ in want}) == FORWARDS
    for slots in (8, 4, 2, 1):
        got = batches.run(eng[slots], sync_every=False)
        moved = _moved(got, want)
        for f in moved[:3]:
            print("%s n=%d slots=%d forward %d: max |d act| = %g" % (case, n, slots, f, float(np.abs(got[f][0] - want[f][0]).max())))
        assert not moved, "%s, n = %d, %d slots: forwards %s differ from the synchronised one-slot engine's bytes" % (case, n, slots, moved)


@pytest.mark.parametrize("precision", ["fp32", "bf16_all"])
def test_back_to_back_reuse_of_one_slot_keeps_every_label(stress_weights, precision):
    """One slot, two alternating batches, nothing synchronised in between: every forward's event branch overwrites what the
    previous forward's dense launch reads (hlast; in the bf16 modes the joint row). Stress weights (|h| up to 0.99, logits
    spanning +-10) and two batches with different k-mers: a dense that read the NEXT forward's h would change labels."""
    from deepsignal_amd import synth
    from deepsignal_amd.engine import Engine
    n = MAX_BATCH
    a = synth.synthetic_features(n, seed=6201)
    b = synth.synthetic_features(n, seed=6202)
    b["kmer"] = ((a["kmer"] + 1 + np.arange(a["kmer"].shape[1], dtype=np.int32)[None, :] % 3) % 4).astype(np.int32)   # no code in common with a
    feats = {k: np.concatenate([a[k], b[k]]) for k in KEYS}
    batches = _DeviceBatches(feats, n, 2, forwards=[f % 2 for f in range(FORWARDS)])
    eng = Engine(max_batch=n, slots=1, precision=precision, fold_fc=False)
    eng.load_weights(stress_weights)
    try:
        want = batches.run(eng, sync_every=True)
        # the two batches are told apart by their LABELS, not by low bits
        differ = int((want[0][1] != want[1][1]).sum())
        print("%s: %d of %d sites change label between the two batches" % (precision, differ, n))
        assert differ >= n // 8
        assert not _moved(want[2:], want[:2] * (FORWARDS // 2 - 1))
        for rep in range(2):
            got = batches.run(eng, sync_every=False)
            moved = _moved(got, want)
            for f in moved[:3]:
                print("%s forward %d: %d labels differ" % (precision, f, int((got[f][1] != want[f][1]).sum())))
            assert not moved, "%s: forwards %s of the unsynchronised run differ" % (precision, moved)
    finally:
        eng.close()


@pytest.mark.parametrize("variant", sorted(VARIANTS))
def test_tickets_over_eight_slots_equal_the_blocking_forward(variant):
    """The host routes share the forward's issue: 16 submit / wait tickets of 70 sites over 8 slots against run() of the same arrays."""
    from deepsignal_amd import synth
    n, tickets = 70, 16
    eng = _engine(_weights(variant), variant, "fp32", False, 8)
    try:
        feats = synth.synthetic_features(tickets * n, seed=6300, signal_len=SIGNAL_LEN)
        parts = [tuple(feats[k][t * n:(t + 1) * n] for k in KEYS) for t in range(tickets)]
        want = [eng.run(*p) for p in parts]
        assert len({a.tobytes() for a, _ in want}) == tickets
        got, pending = [], []
        for p in parts:
            if len(pending) == eng.slots:
                got.append(eng.wait(pending.pop(0)))
            pending.append(eng.submit(*p))
        got += [eng.wait(t) for t in pending]
        assert not _moved(got, want)
    finally:
        eng.close()


@pytest.mark.parametrize("variant", sorted(VARIANTS))
def test_ragged_sizes_in_sequence_equal_fresh_engines(variant):
    """n = 128, 1, 70, 128 on one two-slot engine, three times over and never synchronised inside a pass: the full batch replays
    the graphs captured at load, 1 and 70 are issued eagerly at their first use and captured when they come back on the same slot."""
    from deepsignal_amd import synth
    sizes = (128, 1, 70, 128)
    w = _weights(variant)
    feats = synth.synthetic_features(MAX_BATCH, seed=6400, signal_len=SIGNAL_LEN)
    want = {}
    for n in sorted(set(sizes)):
        fresh = _engine(w, variant, "fp32", False, 1)
        want[n] = _DeviceBatches(feats, n, 1).run(fresh, sync_every=True)[0]
        fresh.close()
    eng = _engine(w, variant, "fp32", False, 2)
    try:
        import torch
        dev = torch.device("cuda", 0)
        d = _to_device(torch, feats)
        for rep in range(3):
            outs = [(torch.full((n, 2), -7.0, dtype=torch.float32, device=dev), torch.full((n,), -7, dtype=torch.int32, device=dev)) for n in sizes]
            torch.cuda.synchronize()
            for n, (a, p) in zip(sizes, outs):
                eng.run_device(n, *(d[k].data_ptr() for k in KEYS), a.data_ptr(), p.data_ptr())
            eng.sync()
            for i, (n, (a, p)) in enumerate(zip(sizes, outs)):
                assert a.cpu().numpy().tobytes() == want[n][0].tobytes() and p.cpu().numpy().tobytes() == want[n][1].tobytes(), \
                    "%s: pass %d, forward %d (n = %d) differs from a fresh engine" % (variant, rep, i, n)
    finally:
        eng.close()


@pytest.mark.parametrize("variant", sorted(VARIANTS))
def test_graphs_captured_under_profiling_mode_3_replay_on_both_streams(variant):
    """The full-batch graphs are captured when the weights are loaded and kept. Profiling mode 3 (every launch on one stream) may
    be on at that moment and off afterwards: the captured split must not have followed it, or the event ops would sit in the
    signal graph on stream 0 while ds_forward_device copies their inputs on stream 1 with nothing ordering the two. 8 forwards
    with their own data, unsynchronised, on such an engine against a fresh engine synchronised after every forward."""
    from deepsignal_amd import synth
    from deepsignal_amd.engine import Engine
    n, forwards = MAX_BATCH, 8
    w = _weights(variant)
    feats = synth.synthetic_features(forwards * n, seed=6500, signal_len=SIGNAL_LEN)
    batches = _DeviceBatches(feats, n, forwards)
    fresh = _engine(w, variant, "fp32", False, 1)
    want = batches.run(fresh, sync_every=True)
    fresh.close()
    assert len({a.tobytes() for a, _ in want}) == forwards
    eng = Engine(max_batch=MAX_BATCH, signal_len=SIGNAL_LEN, slots=2, precision="fp32", fold_fc=False, fuse_min_tiles=1, **VARIANTS[variant])
    try:
        eng.set_profiling(3)
        eng.load_weights(w)
        profiled = batches.run(eng, sync_every=False)          # mode 3 itself: eager, one stream
        assert not _moved(profiled, want), "%s: profiling mode 3 moved results" % variant
        eng.set_profiling(0)
        for rep in range(2):
            got = batches.run(eng, sync_every=False)
            moved = _moved(got, want)
            assert not moved, "%s: forwards %s differ after profiling mode 3 was switched off (pass %d)" % (variant, moved, rep)
    finally:
        eng.close()
