"""DS_PRECISION_FP16X2 on the GPU: fp32 operands carried as two fp16 terms, three products per MAC, fp32 accumulate
(deepsignal_amd/csrc/ds_split.hip + ds_split_kernels.inc compiled for TermsHf2; contract: include/deepsignal_hip.h).

The reference is the CPU statement of the SAME arithmetic (tests/fp16x2_statement.py::forward_fp16x2, held to the float64 oracle by
tests/test_fp16x2_statement.py): engine and statement differ in the fp32 summation order only, so the bar is test_gpu_split's
STATEMENT_RTOL. That comparison is also the measurement of whether v_mfma_f32_32x32x16_f16 keeps subnormal inputs on gfx950 (h1 is
subnormal whenever |x| < 0.125): a flushing MFMA misses the statement by orders of magnitude (2.7e-3 / 1.6e-2 on act in emulation).
The trained-regime bars against float64 are test_gpu_stress's, imported unchanged.
"""
import numpy as np
import pytest

import fp16x2_statement as st
from deepsignal_amd import synth
from test_gpu_split import STATEMENT_RTOL
from test_gpu_stress import FLOOR_REL, NOISE_FACTOR, _check_outputs_f64, _fp32_noise

pytestmark = pytest.mark.gpu
KEYS = ("kmer", "means", "stds", "sanums", "signals")
STATEMENT_TAPS = ("stem_conv2", "stem_conv3", "signal_feat", "fc1")


def _engine(weights, **kw):
    from deepsignal_amd.engine import Engine
    kw.setdefault("precision", "fp16x2")
    eng = Engine(**kw)
    eng.load_weights(weights)
    return eng


def _args(feats, n=None):
    return [feats[k][:n] for k in KEYS]


def _same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


@pytest.mark.parametrize("which", ["small", "stress"])
def test_engine_against_the_cpu_statement_of_the_same_arithmetic(request, which):
    w = request.getfixturevalue(which + "_weights")
    n = 96
    feats = synth.synthetic_features(n, seed=4100)
    eng = _engine(w, max_batch=128, debug=True, split_dense_min_n=1)
    act, pred = eng.run(*_args(feats))
    s_act, s_pred, taps = st.forward_fp16x2(w, feats, return_taps=True)
    worst = {}
    for name, ref in taps.items():
        if not (name.startswith("module") or name.startswith("lstm") or name in STATEMENT_TAPS):
            continue
        got = eng.intermediate(name, ref.shape)
        scale = max(1.0, float(np.abs(ref).max()))
        # (the stress LSTM taps: the slack test_gpu_split gives them -- v_exp_f32 / v_rcp_f32 here, libm there, amplified by saturating gates)
        worst[name] = float(np.abs(got - ref).max()) / scale / (4.0 if which == "stress" and name.startswith("lstm") else 1.0)
    d_act = float(np.abs(act - s_act).max())
    print("\n%s: engine vs forward_fp16x2, relative to the tensor's scale: %s; |d act| %.2e" % (which, {k: "%.1e" % v for k, v in worst.items()}, d_act))
    eng.close()
    bad = {k: v for k, v in worst.items() if not v <= STATEMENT_RTOL}
    assert not bad, bad
    assert d_act <= (1e-5 if which == "small" else 1e-4)


def test_the_fp16x2_kernels_are_the_ones_that_run(small_weights):
    """The profiler's names: the three-step engine launches every split kernel class, and on this handle each reports its fp16x2 instantiation.
    (The names follow the handle's term format, as the launchers do; that the two-term code really ran is what the statement test shows:
    the weight panels and the h images of this handle hold fp16 terms, and a bf16 MFMA on them gives garbage.)"""
    feats = synth.synthetic_features(96, seed=4101)
    eng = _engine(small_weights, max_batch=96, fold_fc=False, split_dense_min_n=1)
    eng.set_graph(False)
    eng.set_profiling(1)
    eng.run(*_args(feats))
    ran = {k["name"]: k["launches"] for k in eng.kernel_stats() if k["launches"]}
    eng.close()
    for prefix in ("stem23_fp16x2_kernel", "inception_fused_fp16x2_kernel", "lstm_cell_fp16x2_kernel", "lstm_xproj_fp16x2_kernel", "dense_fp16x2_kernel"):
        assert any(name.startswith(prefix) for name in ran), (prefix, ran)
    # ... and neither the three-term kernels nor the native fp32 / bf16 ones did
    assert not any(name.startswith(("stem23_split_kernel", "inception_fused_split_kernel", "lstm_cell_split_kernel", "lstm_xproj_kernel", "dense_split_kernel",
                                    "stem23_kernel", "stem23_bf16_kernel", "inception_fused_kernel", "inception_fused_bf16", "lstm_cell_lds_kernel",
                                    "lstm_cell_kernel", "lstm_cell_bf16_kernel", "gemm_kernel<1,3,4,1", "gemm_kernel<4,2,1,4")) for name in ran), ran


@pytest.mark.parametrize("which", ["balanced", "stress"])
@pytest.mark.parametrize("n", [1, 130])
def test_layerwise_parity_with_float64_in_the_trained_regime(request, which, n):
    from oracle import oracle
    w = request.getfixturevalue(which + "_weights")
    noise = _fp32_noise(which, w)
    feats = synth.synthetic_features(n, seed=900 + n)
    eng = _engine(w, max_batch=512, debug=True)
    act, pred = eng.run(*_args(feats))
    a32, p32, t32 = oracle.forward(w, feats, "f32", taps=True)
    a64, p64, t64 = oracle.forward(w, feats, "f64", taps=True)
    bad = {}
    for name, ref in t64.items():
        got = eng.intermediate(name, ref.shape)
        scale = max(1.0, float(np.abs(ref).max()))
        e_hip, e_o32 = float(np.abs(got - ref).max()), float(np.abs(t32[name] - ref).max())
        tol = NOISE_FACTOR * max(e_o32, noise[name]) + FLOOR_REL * scale
        if not e_hip <= tol:
            bad[name] = (e_hip, tol)
    eng.close()
    d_act, d_pn, share = _check_outputs_f64(act, pred, a64, p64, need_balance=n >= 100)
    print("\n%s n=%d: fp16x2 vs f64 |d act| %.2e |d p_norm| %.2e (fp32 oracle vs f64 %.2e)" % (which, n, d_act, d_pn, float(np.abs(a32 - a64).max())))
    assert not bad, "intermediates further from float64 than %gx the fp32 oracle: %s" % (NOISE_FACTOR, bad)


@pytest.mark.parametrize("which", ["balanced", "stress"])
def test_default_engine_folded_joint_ragged_single_and_sub_batch(request, which):
    from oracle import oracle
    w = request.getfixturevalue(which + "_weights")
    n = 549
    feats = synth.synthetic_features(n, seed=1449)
    eng = _engine(w, max_batch=512)
    act, pred = eng.run(*_args(feats))
    a1, p1 = eng.run(*[feats[k][300:301] for k in KEYS])
    a2, p2 = eng.run(*[feats[k][100:233] for k in KEYS])
    eng.close()
    a64, p64 = oracle.forward(w, feats, "f64")
    _check_outputs_f64(act, pred, a64, p64)
    assert _same_bits(a1, act[300:301]) and _same_bits(p1, pred[300:301])
    assert _same_bits(a2, act[100:233]) and _same_bits(p2, pred[100:233])


def test_chained_launch_gives_the_bits_of_one_launch_per_module(small_weights):
    feats = synth.synthetic_features(333, seed=812)
    chained = _engine(small_weights, max_batch=333, slots=1)
    a1, p1 = chained.run(*_args(feats))
    a1s, p1s = chained.run(*_args(feats, 77))
    chained.close()
    single = _engine(small_weights, max_batch=333, slots=1, chain_modules=False)
    a2, p2 = single.run(*_args(feats))
    single.close()
    assert _same_bits(a1, a2) and _same_bits(p1, p2)
    assert _same_bits(a1s, a1[:77]) and _same_bits(p1s, p1[:77])


def test_cell_tilings_give_the_same_bits(small_weights):
    """64 x 64, 64 x 128, 128 x 128 by four and by eight waves: four 32-site m-tiles, the last ragged (100 sites)."""
    feats = synth.synthetic_features(100, seed=906)
    outs = []
    for tiling in ("narrow", "lds1", "wide", "wide8"):
        eng = _engine(small_weights, max_batch=100, slots=1, lstm_tiling=tiling)
        outs.append(eng.run(*_args(feats)))
        eng.close()
    for a, p in outs[1:]:
        assert _same_bits(a, outs[0][0]) and _same_bits(p, outs[0][1])


def test_dense_in_ranges_of_k(small_weights):
    """dense(J, J): the 256 x 192 tile with K in 4 ranges (max_batch 512) and 2 (1,024), ragged m-blocks and one m-tile, against the native
    fp32 engine (the dense is linear in its inputs: the fp32 bar of test_gpu_split), and a site's bits independent of n."""
    feats = synth.synthetic_features(513, seed=4107)
    for n_max, sizes in ((512, (512, 300, 32, 5)), (1024, (513,))):
        ref = _engine(small_weights, max_batch=n_max, slots=1, precision="fp32", fold_fc=False)
        eng = _engine(small_weights, max_batch=n_max, slots=1, fold_fc=False)
        full = None
        for n in sizes:
            a0, p0 = ref.run(*_args(feats, n))
            a1, p1 = eng.run(*_args(feats, n))
            f0 = ref.intermediate("fc1", (n, 6032))
            f1 = eng.intermediate("fc1", (n, 6032))
            assert np.abs(f1 - f0).max() <= 2e-5 * max(1.0, float(np.abs(f0).max())), (n_max, n, float(np.abs(f1 - f0).max()))
            assert np.abs(a1 - a0).max() <= 2e-5 and np.array_equal(p0, p1), (n_max, n, float(np.abs(a1 - a0).max()))
            if full is None:
                full = (a1, f1)
            else:
                assert _same_bits(a1, full[0][:n]) and _same_bits(f1, full[1][:n]), (n_max, n)
        ref.close(); eng.close()


@pytest.mark.parametrize("variant", [dict(is_base=False), dict(is_rnn=False), dict(is_cnn=False)])
def test_model_variants_against_the_statement(variant):
    from deepsignal_amd import weights as W
    w = W.random_weights(seed=21, lstm_bias_std=0.1, **variant)
    feats = synth.synthetic_features(33, seed=78)
    eng = _engine(w, max_batch=64, split_dense_min_n=1, **variant)
    act, pred = eng.run(*_args(feats))
    eng.close()
    s_act, s_pred = st.forward_fp16x2(w, feats, **variant)
    assert np.isfinite(act).all() and np.abs(act - s_act).max() <= 1e-5, float(np.abs(act - s_act).max())


def test_short_geometry_against_the_statement():
    import hostile_cases as hc
    from deepsignal_amd import weights as W
    g = hc.GEOMETRIES["short"]
    w = W.random_weights(seed=33, lstm_bias_std=0.1, **g)
    feats = synth.synthetic_features(33, seed=77, **g)
    eng = _engine(w, max_batch=64, **g)
    act, pred = eng.run(*_args(feats))
    eng.close()
    s_act, s_pred = st.forward_fp16x2(w, feats)
    assert np.abs(act - s_act).max() <= 1e-5


def test_a_site_beyond_the_fp16_range_is_nan_and_its_neighbours_are_untouched(small_weights):
    """One directed case: site 40's signals scaled until a conv_layer2 input (a stem_pool value, ReLU output) exceeds 65504. h0 = Inf,
    h1 = -Inf, and every product with them is NaN, in the engine as in the statement; the other sites keep their bits."""
    n, at = 96, 40
    feats = synth.synthetic_features(n, seed=4111)
    plain = _engine(small_weights, max_batch=128, debug=True)
    a0, p0 = plain.run(*_args(feats))
    s0, _, taps = st.forward_fp16x2(small_weights, feats, return_taps=True)
    peak = float(np.abs(taps["stem_pool"][at]).max())
    assert peak > 0
    hot = {k: v.copy() for k, v in feats.items()}
    hot["signals"][at] *= np.float32(4.0 * st.FP16_MAX / peak)       # conv1 is linear up to its (small) BN shift: well beyond the range
    a1, p1 = plain.run(*_args(hot))
    plain.close()
    s1, _, taps1 = st.forward_fp16x2(small_weights, hot, return_taps=True)
    assert float(np.abs(taps1["stem_pool"][at]).max()) > st.FP16_MAX
    assert np.isnan(s1[at]).all() and np.isnan(a1[at]).all()
    others = np.arange(n) != at
    assert np.isfinite(a1[others]).all() and _same_bits(a1[others], a0[others]) and _same_bits(p1[others], p0[others])
    assert np.abs(a1[others] - s1[others]).max() <= 1e-5


_PLAIN = {}


@pytest.mark.parametrize("batch", ["b0", "b1", "b2", "b3", "b4"])
def test_hostile_batches_against_the_statement(small_weights, batch):
    """tests/hostile_cases.py: NaN exactly where the statement's act is NaN (a signal sample of +-1e30 leaves the fp16 range: NaN in
    both), finite entries within ACT_ATOL of it, and a plain site's bits are the ones it has in the plain batch."""
    import hostile_cases as hc
    from test_gpu_parity import ACT_ATOL
    eng = _engine(small_weights, max_batch=hc.MAX_BATCH)
    if "bits" not in _PLAIN:
        _PLAIN["bits"] = eng.run(*[hc.plain("default")[k] for k in hc.KEYS])
    f = hc.hostile("default", batch)
    act, pred = eng.run(*[f[k] for k in hc.KEYS])
    eng.close()
    s_act, s_pred = st.forward_fp16x2(small_weights, f)
    print("\n%s: NaN sites engine %s statement %s" % (batch, np.nonzero(np.isnan(act).any(axis=1))[0].tolist(), np.nonzero(np.isnan(s_act).any(axis=1))[0].tolist()))
    msg = hc.compare_nonfinite(act, s_act, atol=ACT_ATOL)
    assert msg is None, msg
    for i, name in hc.case_names(batch).items():
        if name in ("sig_one_1e30", "sig_one_minus_1e30"):
            assert np.isnan(act[i]).all() and np.isnan(s_act[i]).all(), name
    others = np.ones(hc.N, bool)
    others[list(hc.HOSTILE_AT)] = False
    a0, p0 = _PLAIN["bits"]
    assert _same_bits(act[others], a0[others]) and _same_bits(pred[others], p0[others])


def test_eight_slots_in_flight_match_one_slot(small_weights):
    feats = synth.synthetic_features(8 * 64, seed=515)
    one = _engine(small_weights, max_batch=64, slots=1)
    ref = [one.run(*[feats[k][64 * i:64 * i + 64] for k in KEYS]) for i in range(8)]
    one.close()
    eight = _engine(small_weights, max_batch=64, slots=8)
    a, p = eight.run(*_args(feats))        # 512 sites through an engine of 64: eight forwards in flight
    eight.close()
    for i in range(8):
        assert _same_bits(a[64 * i:64 * i + 64], ref[i][0]) and _same_bits(p[64 * i:64 * i + 64], ref[i][1])


def test_cascade_rechecks_in_fp16x2(stress_weights):
    """bf16_all with recheck_precision fp16x2: the selected sites carry the fp16x2 engine's bits, the others the coarse engine's."""
    from test_gpu_recheck import _median_margin, _select
    feats = synth.synthetic_features(300, seed=31)
    coarse = _engine(stress_weights, max_batch=512, precision="bf16_all")
    ac, pc = coarse.run(*_args(feats))
    fine = _engine(stress_weights, max_batch=512)
    af, pf = fine.run(*_args(feats))
    margin = _median_margin(ac)
    sel = _select(ac, margin)
    assert 0 < sel.sum() < len(sel)
    coarse.set_recheck(fine, margin)
    ak, pk = coarse.run(*_args(feats))
    coarse.close(); fine.close()
    assert _same_bits(ak[sel], af[sel]) and _same_bits(pk[sel], pf[sel])
    assert _same_bits(ak[~sel], ac[~sel]) and _same_bits(pk[~sel], pc[~sel])


def test_the_mode_refuses_what_it_does_not_implement():
    from deepsignal_amd.call_modifications import check_recheck_args
    from deepsignal_amd.engine import Engine
    with pytest.raises(RuntimeError, match="FP16X2"):
        Engine(max_batch=64, precision="fp16x2", no_fused=True)
    with pytest.raises(ValueError, match="nothing to recheck"):
        check_recheck_args("fp16x2", 0.05, "fp32")
    check_recheck_args("bf16_all", 0.05, "fp16x2")


def test_cli_call_mods_in_fp16x2(balanced_weights, tmp_path):
    """`call_mods --precision fp16x2`, feature TSV -> result TSV on 256 rows: the rows of the fp32 run with the same labels wherever the
    fp32 probabilities are further apart than the label margin, and probabilities within the output bar of each other."""
    from deepsignal_amd import weights as W
    from deepsignal_amd.deepsignal import main
    from test_gpu_recheck import _write_feature_tsv
    from test_gpu_stress import LABEL_MARGIN, OUT_ATOL
    n = 256
    feats = synth.synthetic_features(n, seed=4801)
    tsv, dsw = str(tmp_path / "features.tsv"), str(tmp_path / "model.dsw")
    _write_feature_tsv(tsv, feats, ["read_%04d" % (i // 20) for i in range(n)])
    W.save_weights(dsw, balanced_weights)
    rows = {}
    for prec in ("fp32", "fp16x2"):
        out = str(tmp_path / (prec + ".tsv"))
        assert main(["call_mods", "-i", tsv, "-m", dsw, "-o", out, "--engine_batch", "512", "--precision", prec]) == 0
        rows[prec] = [l.rstrip("\n").split("\t") for l in open(out)]
    assert len(rows["fp32"]) == len(rows["fp16x2"]) == n
    flips = 0
    for a, b in zip(rows["fp32"], rows["fp16x2"]):
        assert a[:6] == b[:6] and a[9:] == b[9:]                      # site, read and k-mer columns
        p0, p1, q0, q1 = float(a[6]), float(a[7]), float(b[6]), float(b[7])
        assert abs(p0 - q0) <= 2 * OUT_ATOL and abs(p1 - q1) <= 2 * OUT_ATOL      # (each run within OUT_ATOL of float64)
        if abs(p1 - p0) > LABEL_MARGIN:
            assert a[8] == b[8]
        flips += a[8] != b[8]
    labels = [r[8] for r in rows["fp16x2"]]
    assert 0.2 * n <= labels.count("1") <= 0.8 * n, "label check would be vacuous"
    print("\ncall_mods fp16x2 vs fp32: %d of %d labels differ (all inside the margin)" % (flips, n))
