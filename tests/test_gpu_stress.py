"""GPU parity in the regime a TRAINED model lives in (reference arithmetic: layers.py:45-72 LSTM cells,
layers.py:80-139 BN + inception, model.py:100-108 sigmoid / argmax).

`random_weights` never leaves the linear part of any sigmoid / tanh and gives every site of a batch the same label. The
`stress_weights` fixture (weights.stress_weights + the committed head of tests/golden/stress_golden.npz) has LSTM gate
pre-activations of std ~1.5 (|h| up to 0.99), a tenth of the BN channels at gamma 1.5 - 3, logits spanning about +-10 with
anti-correlated columns, and both labels in every batch; `balanced_weights` keeps the benign scale but has both labels.

What can be asked of fp32 here: the fp32 and the float64 CPU oracle ALREADY differ by 3 - 5e-5 on the sigmoid outputs of
these sets (a centred read-out of features whose common mode is 13x their site-to-site variation cancels digits; a
saturating recurrent net amplifies rounding), so `1e-5 of the fp32 oracle` is not a meaningful bar -- two correct fp32
evaluations with different summation orders differ by more. The bars, all against the FLOAT64 oracle as the arbiter:

  * every intermediate tensor: HIP's distance to float64 <= NOISE_FACTOR x the fp32 oracle's own distance to float64
    (the larger of: this batch, a fixed 96-site batch) + a floor of 2e-6 x the tensor's scale (the HIP path must be as good an fp32 evaluation as the oracle's, not equal
    to it);
  * sigmoid outputs and normalised probabilities within 1e-4 of float64 (the north star's gate);
  * labels equal wherever the float64 margin |p1 - p0| exceeds 1e-3, AND both labels hold >= 20 % of the batch.

The measured distances are printed (pytest -s) and written to gpurun_out/stress_parity.json; DESIGN.md section 2 quotes them.
"""
import json
import os

import numpy as np
import pytest

from deepsignal_amd import synth

pytestmark = pytest.mark.gpu

NOISE_FACTOR = 4.0
FLOOR_REL = 2e-6
OUT_ATOL = 1e-4          # BASELINE.json north_star: outputs within 1e-4 of the reference
LABEL_MARGIN = 1e-3
KEYS = ("kmer", "means", "stds", "sanums", "signals")
# DS_PRECISION_BF16X3 (three bf16 terms per fp32 operand, six products per MAC, fp32 accumulate) is an fp32-class evaluation and is
# held to the bars of native fp32, unchanged
FP32_CLASS = ["fp32", "bf16x3"]
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _engine(weights, **kw):
    from deepsignal_amd.engine import Engine
    eng = Engine(**kw)
    eng.load_weights(weights)
    return eng


def _norm(a):
    return a / a.sum(axis=1, keepdims=True)


def _record(tag, rec):
    path = os.path.join(ROOT, "gpurun_out", "stress_parity.json")
    try:
        os.makedirs(os.path.dirname(path), exist_ok=True)
        old = json.load(open(path)) if os.path.exists(path) else {}
        old[tag] = rec
        json.dump(old, open(path, "w"), indent=1, sort_keys=True)
    except OSError:
        pass


def _check_outputs_f64(act, pred, a64, p64, need_balance=True):
    assert np.isfinite(act).all()
    d_act = float(np.abs(act - a64).max())
    d_pn = float(np.abs(_norm(act) - _norm(a64)).max())
    assert d_act <= OUT_ATOL and d_pn <= OUT_ATOL, (d_act, d_pn)
    decided = np.abs(a64[:, 1] - a64[:, 0]) > LABEL_MARGIN
    assert (pred[decided] == p64[decided]).all()
    share = float(pred.mean())
    if need_balance:
        assert 0.2 <= share <= 0.8, "label check would be vacuous: label-1 share %.3f" % share
    return d_act, d_pn, share


_NOISE = {}


def _fp32_noise(which, w):
    """Per tensor: the fp32 oracle's distance to the float64 oracle on a fixed 96-site batch -- the size of fp32 rounding
    noise on this weight set (a batch of one site is too small a sample to estimate it from)."""
    if which not in _NOISE:
        from oracle import oracle
        feats = synth.synthetic_features(96, seed=901)
        _, _, t32 = oracle.forward(w, feats, "f32", taps=True)
        _, _, t64 = oracle.forward(w, feats, "f64", taps=True)
        _NOISE[which] = {k: float(np.abs(t32[k] - t64[k]).max()) for k in t64}
    return _NOISE[which]


@pytest.mark.parametrize("precision", FP32_CLASS)
@pytest.mark.parametrize("which", ["balanced", "stress"])
@pytest.mark.parametrize("n", [1, 130, 512])
def test_layerwise_parity_in_the_trained_regime(request, which, n, precision):
    from oracle import oracle
    w = request.getfixturevalue(which + "_weights")
    noise = _fp32_noise(which, w)
    feats = synth.synthetic_features(n, seed=900 + n)
    eng = _engine(w, max_batch=512, debug=True, precision=precision)
    act, pred = eng.run(*(feats[k] for k in KEYS))
    a32, p32, t32 = oracle.forward(w, feats, "f32", taps=True)
    a64, p64, t64 = oracle.forward(w, feats, "f64", taps=True)
    rows, bad = {}, {}
    for name, ref in t64.items():
        got = eng.intermediate(name, ref.shape)
        scale = max(1.0, float(np.abs(ref).max()))
        e_hip = float(np.abs(got - ref).max())
        e_o32 = float(np.abs(t32[name] - ref).max())
        tol = NOISE_FACTOR * max(e_o32, noise[name]) + FLOOR_REL * scale
        rows[name] = {"max_abs": scale, "hip_vs_f64": e_hip, "oracle_f32_vs_f64": e_o32, "hip_vs_oracle_f32": float(np.abs(got - t32[name]).max())}
        if not e_hip <= tol:
            bad[name] = (e_hip, tol)
    if which == "stress":
        h = t64["lstm_fw_l2"]
        assert float(np.abs(h).max()) > 0.9, "the stress set no longer saturates the LSTM"
        assert n == 1 or float(np.abs(t64["logits"]).max()) > 8.0, "the stress set's logits no longer span +-10"
    d_act, d_pn, share = _check_outputs_f64(act, pred, a64, p64, need_balance=n >= 100)
    rec = {"n": n, "max_abs_d_act_vs_f64": d_act, "max_abs_d_pnorm_vs_f64": d_pn,
           "oracle_f32_d_act_vs_f64": float(np.abs(a32 - a64).max()),
           "oracle_f32_d_pnorm_vs_f64": float(np.abs(_norm(a32) - _norm(a64)).max()),
           "hip_d_act_vs_oracle_f32": float(np.abs(act - a32).max()),
           "label1_share": share, "logit_range": [float(t64["logits"].min()), float(t64["logits"].max())],
           "max_abs_h": float(np.abs(t64["lstm_fw_l2"]).max()), "taps": rows}
    _record("%s_n%d_three_step%s" % (which, n, "" if precision == "fp32" else "_" + precision), rec)
    print("\n%s n=%d: HIP vs f64 |d act| %.2e |d p_norm| %.2e   (fp32 oracle vs f64: %.2e / %.2e; HIP vs fp32 oracle %.2e)  label-1 share %.2f"
          % (which, n, d_act, d_pn, rec["oracle_f32_d_act_vs_f64"], rec["oracle_f32_d_pnorm_vs_f64"], rec["hip_d_act_vs_oracle_f32"], share))
    worst = sorted(rows.items(), key=lambda kv: -kv[1]["hip_vs_f64"] / (kv[1]["oracle_f32_vs_f64"] + FLOOR_REL * kv[1]["max_abs"]))[:4]
    for k, v in worst:
        print("   %-12s |x| %8.3g  HIP-f64 %.2e  o32-f64 %.2e" % (k, v["max_abs"], v["hip_vs_f64"], v["oracle_f32_vs_f64"]))
    assert not bad, "intermediates further from float64 than %gx the fp32 oracle: %s" % (NOISE_FACTOR, bad)
    eng.close()


@pytest.mark.parametrize("precision", FP32_CLASS)
@pytest.mark.parametrize("which", ["balanced", "stress"])
def test_default_engine_folded_joint_and_pipelined_slots(request, which, precision):
    """The product's default engine (joint model folded into one 6032 x 2 matrix, 8 slots, captured graphs) on the same
    sets: a ragged 549-site call, then the same sites alone and in a sub-batch give the same bits."""
    from oracle import oracle
    w = request.getfixturevalue(which + "_weights")
    n = 512 + 37
    feats = synth.synthetic_features(n, seed=31)
    eng = _engine(w, max_batch=512, precision=precision)
    act, pred = eng.run(*(feats[k] for k in KEYS))
    a64, p64 = oracle.forward(w, feats, "f64")
    d_act, d_pn, share = _check_outputs_f64(act, pred, a64, p64)
    a32, _ = oracle.forward(w, feats, "f32")
    _record("%s_n549_folded%s" % (which, "" if precision == "fp32" else "_" + precision), {"max_abs_d_act_vs_f64": d_act, "max_abs_d_pnorm_vs_f64": d_pn, "label1_share": share,
                                       "oracle_f32_d_act_vs_f64": float(np.abs(a32 - a64).max())})
    print("\n%s folded n=%d: |d act| %.2e |d p_norm| %.2e (fp32 oracle: %.2e), label-1 share %.2f"
          % (which, n, d_act, d_pn, float(np.abs(a32 - a64).max()), share))
    a1, p1 = eng.run(*(feats[k][7:8] for k in KEYS))
    assert np.array_equal(a1[0], act[7]) and p1[0] == pred[7]
    a2, p2 = eng.run(*(feats[k][100:177] for k in KEYS))
    assert np.array_equal(a2, act[100:177]) and np.array_equal(p2, pred[100:177])
    eng.close()


@pytest.mark.parametrize("precision", FP32_CLASS)
def test_stress_golden_vectors_replayed_on_the_gpu(stress_weights, precision):
    """The committed float64 vectors of the stress set (48 sites, all-N k-mer / truncated / all-zero windows among them)."""
    g = np.load(os.path.join(ROOT, "tests", "golden", "stress_golden.npz"))
    feats = {k: g["in_" + k] for k in KEYS}
    for fold in (True, False):
        eng = _engine(stress_weights, max_batch=64, debug=not fold, fold_fc=fold, precision=precision)
        act, pred = eng.run(*(feats[k] for k in KEYS))
        _check_outputs_f64(act, pred, g["act"], g["pred"])
        if not fold:
            fw = eng.intermediate("lstm_fw_l2", (48, 17, 256))[:, -1, :]
            bw = eng.intermediate("lstm_bw_l2", (48, 17, 256))[:, 0, :]
            assert np.abs(fw - g["lstm_fw_l2_last"]).max() <= 5e-5 and np.abs(bw - g["lstm_bw_l2_first"]).max() <= 5e-5
            lg = eng.intermediate("logits", (48, 2))
            assert np.abs(lg - g["logits"]).max() <= 2e-3 * max(1.0, float(np.abs(g["logits"]).max()))
        eng.close()


@pytest.mark.parametrize("layer,sign", [(0, 20.0), (1, -20.0), (2, 20.0)])
def test_saturated_gates(stress_weights, layer, sign):
    """Gate pre-activations of +-20 on one whole layer (all four gates of both directions: sigmoid = 0 or 1 and tanh = +-1
    to the last bit, exp() of +-20 inside fast_sigmoid / fast_tanh) and all-N k-mers on a third of the sites. The outputs
    must stay finite and keep the float64 oracle's values; a saturated layer forgets its input, so the tolerance of the
    unsaturated case holds a fortiori."""
    from oracle import oracle
    w = dict(stress_weights)
    for d in ("fw", "bw"):
        k = "modelem/%s/multi_rnn_cell/cell_%d/lstm_cell/bias" % (d, layer)
        w[k] = (w[k] + np.float32(sign)).astype(np.float32)
    n = 96
    feats = synth.synthetic_features(n, seed=555 + layer)
    feats["kmer"][::3, :] = 4
    for fold in (True, False):
        eng = _engine(w, max_batch=128, fold_fc=fold, debug=not fold)
        act, pred = eng.run(*(feats[k] for k in KEYS))
        a64, p64, t64 = oracle.forward(w, feats, "f64", taps=True)
        assert np.isfinite(act).all()
        assert float(np.abs(act - a64).max()) <= OUT_ATOL
        decided = np.abs(a64[:, 1] - a64[:, 0]) > LABEL_MARGIN
        assert (pred[decided] == p64[decided]).all()
        if not fold:
            for d in ("fw", "bw"):
                name = "lstm_%s_l%d" % (d, layer)
                got = eng.intermediate(name, t64[name].shape)
                assert np.isfinite(got).all() and float(np.abs(got - t64[name]).max()) <= 2e-5, name
        eng.close()


def test_extreme_logits_do_not_break_sigmoid_or_argmax(stress_weights):
    """Head scaled x40: logits of several hundred; sigmoid must give exactly 0 / 1 without NaN (1 / (1 + exp(+-400))),
    argmax must follow the logits (model.py:100,108)."""
    from oracle import oracle
    w = dict(stress_weights)
    w["dense_1/kernel"] = (w["dense_1/kernel"] * np.float32(40.0)).astype(np.float32)
    feats = synth.synthetic_features(64, seed=99)
    for fold in (True, False):
        eng = _engine(w, max_batch=64, fold_fc=fold)
        act, pred = eng.run(*(feats[k] for k in KEYS))
        a64, p64, t64 = oracle.forward(w, feats, "f64", taps=True)
        assert np.isfinite(act).all() and act.min() >= 0.0 and act.max() <= 1.0
        assert float(np.abs(t64["logits"]).max()) > 100.0
        far = np.abs(t64["logits"][:, 1] - t64["logits"][:, 0]) > 1.0
        assert (pred[far] == np.argmax(t64["logits"], axis=1)[far]).all()
        assert float(np.abs(act - a64).max()) <= 2e-3        # logits' fp32 noise x 40 moves the few unsaturated outputs
        eng.close()


@pytest.mark.parametrize("variant", [dict(kmer_len=9, signal_len=100), dict(kmer_len=21, signal_len=128), dict(is_cnn=False),
                                     dict(is_rnn=False), dict(is_base=False),
                                     # long windows: widths above the fused kernels' 96 rows run the layer-granular path
                                     dict(signal_len=385), dict(kmer_len=13, signal_len=800)])
def test_trained_regime_on_other_geometries_and_model_variants(variant):
    """The stress scale (LSTM kernels x 3.5, bias std 0.6, hot BN channels) on the CLI's other shapes (--kmer_len /
    --cent_signals_len, deepsignal.py:258-263) and on the Model(is_cnn, is_rnn, is_base) switches (model.py:28-29,59-75,89-95):
    the head is centred here, from the float64 oracle's fc1 of a probe batch, so both labels occur; same bars as above."""
    from deepsignal_amd import weights as W
    from oracle import oracle
    geom = {k: v for k, v in variant.items() if k in ("kmer_len", "signal_len")}
    w = W.stress_weights(777, **variant)
    probe = synth.synthetic_features(96, seed=778, **geom)
    _, _, taps = oracle.forward(w, probe, "f64", taps=True, **variant)
    W.install_head(w, W.centred_head(taps["fc1"], w["dense_1/kernel"][:, 0], 3.5, 779))
    n = 200
    feats = synth.synthetic_features(n, seed=780, **geom)
    a64, p64 = oracle.forward(w, feats, "f64", **variant)
    a32, _ = oracle.forward(w, feats, "f32", **variant)
    for fold, precision in ((True, "fp32"), (False, "fp32"), (True, "bf16x3")):
        eng = _engine(w, max_batch=256, fold_fc=fold, precision=precision, **variant)
        act, pred = eng.run(*(feats[k] for k in KEYS))
        d_act, d_pn, share = _check_outputs_f64(act, pred, a64, p64)
        eng.close()
        print("\n%s fold=%s %s: |d act| %.2e (fp32 oracle %.2e), label-1 share %.2f" % (variant, fold, precision, d_act, float(np.abs(a32 - a64).max()), share))
