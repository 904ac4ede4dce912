"""GPU: the inference BiLSTM at the ends of kmer_len. ds_create accepts every odd kmer_len in [1, 255]; the rest of the suite runs
5, 9, 13, 17 and 21, all above the three LSTM layers and below the 32nd anti-diagonal. Held here: T = 1, 3, 101 and 255 against the
fp32 C oracle (tests/test_oracle.py pins it to both torch statements at T = 1 and 3; it is general in T), signal_len 40,
max_batch 128, one slot, n = 1 / 33 / 70 = one partial 32-site m-tile, two, three.

The branch of plan_event_model (ds_engine.cpp) or of the cell kernels each case exists for:

  T = 1     a diagonal holds one cell per direction and no cell has a recurrent operand (ah == nullptr everywhere), so
            cls_tiles[0] stays 0 on every diagonal and lstm_logical_tile deals from the second class alone; hlast of BOTH
            directions is taken at sidx == T - 1 == 0, i.e. from t = 0; with lstm_xproj the loop starts at diagonal 1 and
            `nsteps = lstm_xproj_all ? T : 1` makes the "first step" and "all steps" forms one
  T = 3     = NLAYER: exactly one full diagonal (d = 2) between two ramps; T = 5 already has three
  T = 101   a captured chain of T + 2 dependent launches; with DS_TUNE_DEBUG_STAMPS the diagonals past the 32nd get L.dbg == nullptr
            (d < 32); explicit assertions on lstm_fw_l0[:, 100] and lstm_bw_l0[:, 0], both written on diagonal 100
  T = 255   the largest accepted: H / Cst / xproj strides multiplied by t up to 254 (n = 33 only, to stay within seconds)
  stress    weights.stress_weights at T = 1 and 3 only, bars of tests/test_gpu_stress.py against the float64 oracle: at long T the
            fp32 ORACLE is already 7e-5 (T = 101) and 5e-4 (T = 255) from float64 on the LSTM taps, past any bar
  directions at T = 1       fw and bw read the same single step with their own weights: swapped weights or a bw stack that reads
            t = T - 1 - sidx wrongly cannot show at T > 1 in the same way; joint = [lstm_fw_l2[:, 0] | lstm_bw_l2[:, 0]] byte for byte
  lstm_xproj forms          (True, "all", False) give the same bytes at T = 1 and 3, and lstm_xproj_kernel runs iff the form is not False
  tilings                   every engine.LSTM_TILINGS value gives the bytes of "auto" when a diagonal has 2 (T = 1) or 2 .. 6 (T = 3) cells
  fp16x2, bf16_all, bf16    T = 1 and 3 at n = 70, against the CPU statements of the same arithmetic with the bars of
            tests/test_gpu_fp16x2.py and test_other_kmer_and_signal_lengths; not at long T: the project has no bar for the bf16
            recurrence beyond T = 21 and none can be derived without a GPU
  in flight at T = 1        the event branch is three launches and ends long before the signal branch: the join and the slot-reuse
            edge (fork_event_stream) are exercised the other way round from tests/test_gpu_run_ahead_bits.py
"""
import numpy as np
import pytest

from test_gpu_parity import INTERMEDIATE_RTOL, _check_outputs
from test_gpu_stress import FLOOR_REL, NOISE_FACTOR, _check_outputs_f64
from test_oracle import end_features

pytestmark = pytest.mark.gpu

KEYS = ("kmer", "means", "stds", "sanums", "signals")
S, MAX_BATCH = 40, 128
SIZES = {1: (1, 33, 70), 3: (1, 33, 70), 101: (1, 33, 70), 255: (33,)}
LSTM_TAPS = tuple("lstm_%s_l%d" % (d, l) for d in ("fw", "bw") for l in range(3))
# fp32-class engines: the folded joint model has no joint tensor, the others give it
ENGINES = {"fp32-folded": dict(precision="fp32"),
           "fp32-three_step": dict(precision="fp32", fold_fc=False),
           "bf16x3-xproj_first": dict(precision="bf16x3", fold_fc=False, lstm_xproj=True),
           "bf16x3-xproj_all": dict(precision="bf16x3", fold_fc=False, lstm_xproj="all"),
           "bf16x3-xproj_none": dict(precision="bf16x3", fold_fc=False, lstm_xproj=False)}

_CASES = {}


def _geom(T):
    return dict(kmer_len=T, signal_len=S)


def _case(T, kind="random"):
    """Weights, the largest batch of this T and the oracle's results on it, computed once (a site's oracle bits do not depend on
    the batch it travels in: tests/test_oracle.py::test_site_independence_and_batch_order)."""
    if (T, kind) not in _CASES:
        from deepsignal_amd import weights as W
        from oracle import oracle
        n = max(SIZES[T])
        feats = end_features(n, 8, T, S)
        c = {"feats": feats}
        if kind == "random":
            w = W.random_weights(seed=33, lstm_bias_std=0.1, **_geom(T))
        else:
            # the head is centred on a probe batch from the float64 oracle's fc1, as tests/test_gpu_stress.py does for its other
            # geometries: both labels occur
            w = W.stress_weights(**_geom(T))
            probe = end_features(96, 778, T, S)
            _, _, taps = oracle.forward(w, probe, "f64", taps=True, **_geom(T))
            W.install_head(w, W.centred_head(taps["fc1"], w["dense_1/kernel"][:, 0], 3.5, 779))
            c["f64"] = oracle.forward(w, feats, "f64", taps=True, **_geom(T))
            # the fp32 oracle's own distance to float64 on a fixed 96-site batch (test_gpu_stress._fp32_noise, at this geometry)
            noise_feats = end_features(96, 901, T, S)
            _, _, t32 = oracle.forward(w, noise_feats, "f32", taps=True, **_geom(T))
            _, _, t64 = oracle.forward(w, noise_feats, "f64", taps=True, **_geom(T))
            c["noise"] = {k: float(np.abs(t32[k] - t64[k]).max()) for k in t64}
        c["w"] = w
        c["f32"] = oracle.forward(w, feats, "f32", taps=True, **_geom(T))
        _CASES[(T, kind)] = c
    return _CASES[(T, kind)]


def _engine(w, T, **kw):
    from deepsignal_amd.engine import Engine
    kw.setdefault("slots", 1)
    eng = Engine(max_batch=MAX_BATCH, **_geom(T), **kw)
    eng.load_weights(w)
    return eng


def _args(feats, n):
    return [feats[k][:n] for k in KEYS]


def _tap_names(cfg):
    return LSTM_TAPS + (("joint",) if cfg.get("fold_fc", True) is False else ()) + ("logits",)


def _taps(eng, names, ref, n):
    return {k: eng.intermediate(k, (n,) + ref[k].shape[1:]) for k in names}


@pytest.mark.parametrize("tag", sorted(ENGINES))
@pytest.mark.parametrize("T", sorted(SIZES))
def test_fp32_class_parity_with_the_oracle(T, tag):
    c = _case(T)
    o_act, o_pred, o_taps = c["f32"]
    eng = _engine(c["w"], T, debug=True, **ENGINES[tag])
    try:
        for n in SIZES[T]:
            act, pred = eng.run(*_args(c["feats"], n))
            got = _taps(eng, _tap_names(ENGINES[tag]), o_taps, n)
            bad = {}
            for name, g in got.items():
                ref = o_taps[name][:n]
                err, tol = float(np.abs(g - ref).max()), INTERMEDIATE_RTOL * max(1.0, float(np.abs(ref).max()))
                print("T=%d %s n=%d %-10s err %.3g tol %.3g" % (T, tag, n, name, err, tol))
                if not (np.isfinite(g).all() and err <= tol):
                    bad[name] = (err, tol)
            assert not bad, (n, bad)
            _check_outputs(act, pred, o_act[:n], o_pred[:n])
            if T == 101:
                # the steps far beyond the 32nd diagonal, named so that the intent survives refactoring: fw layer 0 step 100 is
                # diagonal 100; bw layer 0 at t = 0 is its last step, diagonal 100 too
                for name, t in (("lstm_fw_l0", 100), ("lstm_bw_l0", 0)):
                    ref = o_taps[name][:n, t]
                    assert float(np.abs(ref).max()) > 1e-3
                    assert np.abs(got[name][:, t] - ref).max() <= INTERMEDIATE_RTOL * max(1.0, float(np.abs(o_taps[name][:n]).max())), name
    finally:
        eng.close()


def test_stamp_buffers_end_at_the_32nd_diagonal():
    """DS_TUNE_DEBUG_STAMPS gives the fp32 cell launches of diagonals 0 .. 31 a stamp buffer and the later ones L.dbg == nullptr: at
    T = 101 seventy-one diagonals run without one. Stamping is no arithmetic: the taps are the bytes of the engine without stamps."""
    T, n = 101, 70
    c = _case(T)
    outs = []
    for stamps in (False, True):
        eng = _engine(c["w"], T, debug=True, debug_stamps=stamps, precision="fp32", fold_fc=False)
        try:
            res = list(eng.run(*_args(c["feats"], n)))
            res.extend(eng.intermediate(k, (n, T, 256)) for k in LSTM_TAPS)
            if stamps:
                assert eng.intermediate("lstm_stamps31", (12,))[0] > 0      # workgroups that stamped on the last stamped diagonal
                with pytest.raises(RuntimeError):
                    eng.intermediate("lstm_stamps32", (12,))
        finally:
            eng.close()
        outs.append(res)
    for i, (a, b) in enumerate(zip(*outs)):
        assert a.tobytes() == b.tobytes(), i


@pytest.mark.parametrize("tag", sorted(ENGINES))
@pytest.mark.parametrize("T", [1, 3])
def test_fp32_class_parity_in_the_trained_regime(T, tag):
    """Bars of tests/test_gpu_stress.py, unchanged: every tap within NOISE_FACTOR x the fp32 oracle's own distance to float64 (the
    larger of this batch and a fixed 96-site batch) + FLOOR_REL of the tensor's scale; outputs within 1e-4 of float64; labels equal
    beyond the margin, and both labels present in the 70-site batch."""
    c = _case(T, "stress")
    a64, p64, t64 = c["f64"]
    _, _, t32 = c["f32"]
    # (one step from c = 0 bounds |h| by tanh(1) = 0.76, whatever the weights: the stress set reaches about half of that at T = 1)
    assert float(np.abs(t64["lstm_fw_l2"]).max()) > 0.3, "the stress set no longer drives the gates"
    eng = _engine(c["w"], T, debug=True, **ENGINES[tag])
    try:
        for n in SIZES[T]:
            act, pred = eng.run(*_args(c["feats"], n))
            bad = {}
            for name, g in _taps(eng, _tap_names(ENGINES[tag]), t64, n).items():
                ref = t64[name][:n]
                e_hip, e_o32 = float(np.abs(g - ref).max()), float(np.abs(t32[name][:n] - ref).max())
                tol = NOISE_FACTOR * max(e_o32, c["noise"][name]) + FLOOR_REL * max(1.0, float(np.abs(ref).max()))
                print("T=%d %s n=%d %-10s HIP-f64 %.3g o32-f64 %.3g tol %.3g" % (T, tag, n, name, e_hip, e_o32, tol))
                if not (np.isfinite(g).all() and e_hip <= tol):
                    bad[name] = (e_hip, tol)
            assert not bad, (n, bad)
            _check_outputs_f64(act, pred, a64[:n], p64[:n], need_balance=n == 70)
    finally:
        eng.close()


def test_directions_at_one_step():
    c = _case(1)
    _, _, o_taps = c["f32"]
    n = 70
    eng = _engine(c["w"], 1, debug=True, precision="fp32", fold_fc=False)
    try:
        eng.run(*_args(c["feats"], n))
        got = _taps(eng, LSTM_TAPS + ("joint",), o_taps, n)
    finally:
        eng.close()
    for l in range(3):
        fw, bw = got["lstm_fw_l%d" % l], got["lstm_bw_l%d" % l]
        assert fw.shape == bw.shape == (n, 1, 256)
        # each direction has its own weights: the oracle's two taps differ by far more than the bar, and each engine tap is ITS oracle tap
        o_fw, o_bw = o_taps["lstm_fw_l%d" % l][:n], o_taps["lstm_bw_l%d" % l][:n]
        assert float(np.abs(o_fw - o_bw).max()) > 100 * INTERMEDIATE_RTOL
        assert float(np.abs(fw - bw).max()) > 100 * INTERMEDIATE_RTOL
        assert np.abs(fw - o_fw).max() <= INTERMEDIATE_RTOL and np.abs(bw - o_bw).max() <= INTERMEDIATE_RTOL
    assert got["joint"][:, :256].tobytes() == got["lstm_fw_l2"][:, 0].tobytes()
    assert got["joint"][:, 256:512].tobytes() == got["lstm_bw_l2"][:, 0].tobytes()


@pytest.mark.parametrize("T", [1, 3])
def test_lstm_xproj_forms_give_the_same_bits(T):
    """tests/test_gpu_split.py::test_lstm_xproj_gives_the_bits_of_the_cells_own_initial_values holds this at T = 17."""
    c = _case(T)
    outs = []
    for xp in (True, "all", False):
        eng = _engine(c["w"], T, debug=True, precision="bf16x3", lstm_xproj=xp)
        try:
            eng.set_profiling(1)
            res = []
            for n in SIZES[T]:
                res.extend(eng.run(*_args(c["feats"], n)))
                res.extend(eng.intermediate(k, (n, T, 256)) for k in LSTM_TAPS)
            ran = {k["name"]: k["launches"] for k in eng.kernel_stats() if k["launches"]}
        finally:
            eng.close()
        assert ("lstm_xproj_kernel" in ran) == bool(xp), ran
        assert any(k.startswith("lstm_cell_split_kernel") for k in ran), ran      # layers 1 and 2 still run as cells at T = 1
        outs.append(res)
    for xp, other in zip(("all", False), outs[1:]):
        for i, (a, b) in enumerate(zip(outs[0], other)):
            assert a.tobytes() == b.tobytes(), (xp, i)


@pytest.mark.parametrize("T", [1, 3])
def test_every_lstm_tiling_gives_the_bits_of_auto(T):
    from deepsignal_amd import engine
    c = _case(T)
    outs = {}
    for tiling in engine.LSTM_TILINGS:
        eng = _engine(c["w"], T, debug=True, precision="fp32", lstm_tiling=tiling)
        try:
            res = []
            for n in SIZES[T]:
                res.extend(eng.run(*_args(c["feats"], n)))
                res.extend(eng.intermediate(k, (n, T, 256)) for k in LSTM_TAPS)
            outs[tiling] = res
        finally:
            eng.close()
    for tiling, res in outs.items():
        for i, (a, b) in enumerate(zip(outs["auto"], res)):
            assert a.tobytes() == b.tobytes(), (tiling, i)


@pytest.mark.parametrize("T", [1, 3])
def test_fp16x2_against_its_statement(T):
    """Bars of tests/test_gpu_fp16x2.py: the LSTM taps within test_gpu_split's STATEMENT_RTOL of the CPU statement of the same
    arithmetic, act within 1e-5 of it."""
    import fp16x2_statement as st
    from test_gpu_split import STATEMENT_RTOL
    c = _case(T)
    n = 70
    s_act, s_pred, taps = st.forward_fp16x2(c["w"], {k: c["feats"][k][:n] for k in KEYS}, return_taps=True)
    eng = _engine(c["w"], T, debug=True, precision="fp16x2", split_dense_min_n=1)
    try:
        act, pred = eng.run(*_args(c["feats"], n))
        got = _taps(eng, LSTM_TAPS, taps, n)
    finally:
        eng.close()
    for name, g in got.items():
        e = float(np.abs(g - taps[name]).max()) / max(1.0, float(np.abs(taps[name]).max()))
        print("T=%d fp16x2 %-10s %.3g" % (T, name, e))
        assert e <= STATEMENT_RTOL, (name, e)
    assert np.isfinite(act).all() and np.abs(act - s_act).max() <= 1e-5


@pytest.mark.parametrize("precision", ["bf16", "bf16_all"])
@pytest.mark.parametrize("T", [1, 3])
def test_bf16_modes_against_their_statement(T, precision):
    """The 3e-3 of tests/test_gpu_parity.py::test_other_kmer_and_signal_lengths against torch_statement.forward_bf16."""
    from oracle import torch_statement
    c = _case(T)
    n = 70
    feats = {k: c["feats"][k][:n] for k in KEYS}
    e_act, _ = torch_statement.forward_bf16(c["w"], feats, lstm_bf16=precision == "bf16_all")
    eng = _engine(c["w"], T, precision=precision)
    try:
        act, pred = eng.run(*_args(c["feats"], n))
    finally:
        eng.close()
    d = float(np.abs(act - e_act).max())
    print("T=%d %s |d act| %.3g" % (T, precision, d))
    assert act.shape == (n, 2) and np.isfinite(act).all() and d <= 3e-3


def test_sixteen_forwards_in_flight_at_one_step():
    """16 run_device forwards of 33 sites, each on its own data, over 4 slots and never synchronised, against a one-slot engine
    synchronised after every forward: byte for byte (the pattern of tests/test_gpu_run_ahead_bits.py)."""
    from deepsignal_amd import weights as W
    from test_gpu_run_ahead_bits import _DeviceBatches, _moved
    T, n, forwards = 1, 33, 16
    w = W.random_weights(seed=33, lstm_bias_std=0.1, **_geom(T))
    feats = end_features(forwards * n, 6600, T, S)
    batches = _DeviceBatches(feats, n, forwards)
    one = _engine(w, T, precision="fp32", fold_fc=False, slots=1)
    four = _engine(w, T, precision="fp32", fold_fc=False, slots=4)
    try:
        assert one.slots == 1 and four.slots == 4
        want = batches.run(one, sync_every=True)
        assert all(np.isfinite(a).all() for a, _ in want) and len({a.tobytes() for a, _ in want}) == forwards
        for rep in range(3):      # eager, captured, replayed
            got = batches.run(four, sync_every=False)
            moved = _moved(got, want)
            assert not moved, "pass %d: forwards %s differ from the synchronised one-slot engine's bytes" % (rep, moved)
    finally:
        one.close()
        four.close()
    # ... and the bytes are the oracle's values
    from oracle import oracle
    o_act, o_pred = oracle.forward(w, {k: feats[k][:n] for k in KEYS}, "f32", **_geom(T))
    _check_outputs(want[0][0], want[0][1], o_act, o_pred)
