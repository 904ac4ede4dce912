"""GPU: long signal windows (--cent_signals_len, deepsignal.py:260) and the layer-granular inception path, against the oracles.

The planner (ds_engine.cpp build_plan) runs the stem's conv2 / conv3 and an inception module as fused kernels only when the
module's width is at most 96 rows. Every wider width class takes the layer-granular path: gemm_kernel with shifted SAME-padding
segments (CFG_CONV / CFG_CONV_POOL, maxpool(3, s1) on the A load; CFG_BCONV / CFG_BCONV_POOL in the bf16 modes) and the
stand-alone stride-2 max-pool kernels between width classes. The default window (360: widths 90 / 45 / 23) never reaches it.

  signal_len   w_a / w_b / w_c   what runs layer-granular
  384          96 / 48 / 24      nothing: w_a at the fused kernels' largest tile
  385          97 / 49 / 25      stem conv2/3, modules 1-3 (odd widths, pool pads (1, 1)); unfused -> fused hand-over at module 4
  800 (k 13)   200 / 100 / 50    stem, modules 1-8, maxpool_s2 after module 3; the pool after module 8 folds into module 9
  1537         385 / 193 / 97    everything, both stand-alone pools, the head at J = 23,792
  360 + DS_TUNE_NO_FUSED         the layer-granular path at the default shape

Bars are those of tests/test_gpu_parity.py (fp32 class) and tests/test_gpu_bf16.py (bf16 modes against the emulated statement),
restated here, not widened.
"""
import numpy as np
import pytest

from deepsignal_amd import spec, synth

pytestmark = pytest.mark.gpu

# tests/test_gpu_parity.py
INTERMEDIATE_RTOL = 2e-5
ACT_ATOL = 1e-5
# tests/test_gpu_bf16.py
EMU_TAP_TOL_ULPS = 4.0
EMU_TAP_MEAN_ULPS = 0.25
EMU_ACT_ATOL = 3e-3

KEYS = ("kmer", "means", "stds", "sanums", "signals")
G384, G385, G800, G1537 = dict(signal_len=384), dict(signal_len=385), dict(kmer_len=13, signal_len=800), dict(signal_len=1537)
GEOMS = [pytest.param(G384, id="s384"), pytest.param(G385, id="s385"), pytest.param(G800, id="k13s800"),
         pytest.param(G1537, id="s1537")]


def _ulp(x):
    """bf16 spacing (8 significant bits) at magnitude x"""
    return 2.0 ** (np.floor(np.log2(max(float(x), 1e-30))) - 7)


def _norm(act):
    return act / act.sum(axis=1, keepdims=True)


def _check_outputs(act, pred, o_act, o_pred):
    assert np.isfinite(act).all()
    assert np.abs(act - o_act).max() <= ACT_ATOL
    assert np.abs(_norm(act) - _norm(o_act)).max() <= ACT_ATOL
    decided = np.abs(o_act[:, 1] - o_act[:, 0]) > 1e-3
    assert (pred[decided] == o_pred[decided]).all()


def _engine(weights, **kw):
    from deepsignal_amd.engine import Engine
    eng = Engine(**kw)
    eng.load_weights(weights)
    return eng


@pytest.fixture(scope="module")
def long_weights():
    """One weight set per geometry for the whole module (dense/kernel is J x J: 2.3 GB of fp32 at signal_len 1537)."""
    from deepsignal_amd import weights as W
    cache = {}

    def get(geom):
        key = tuple(sorted(geom.items()))
        if key not in cache:
            cache[key] = W.random_weights(seed=51, lstm_bias_std=0.1, **geom)
        return cache[key]
    yield get
    cache.clear()


@pytest.fixture(scope="module")
def oracle_taps(long_weights):
    """fp32 C oracle with taps, per (geometry, n): shared by the fp32 and bf16x3 legs."""
    from oracle import oracle
    cache = {}

    def get(geom, n):
        key = (tuple(sorted(geom.items())), n)
        if key not in cache:
            feats = _features(n, geom)
            cache[key] = (feats,) + tuple(oracle.forward(long_weights(geom), feats, "f32", taps=True, **geom))
        return cache[key]
    yield get
    cache.clear()


def _features(n, geom, seed=None):
    feats = synth.synthetic_features(n, seed=700 + n if seed is None else seed, **geom)
    if n > 2:
        feats["signals"][1, -5:] = 0.0       # a right-padded short window: zeros up to the last row of every width
        feats["signals"][2, :3] = 4.5        # a hot left edge: the first rows' SAME padding and pool clamps decide the max
    return feats


def _fp32_layerwise(eng, taps, label):
    """eng: an Engine (its debug taps) or a dict of taps"""
    worst = {}
    for name, ref in taps.items():
        got = eng[name] if isinstance(eng, dict) else eng.intermediate(name, ref.shape)
        err = float(np.abs(got - ref).max())
        worst[name] = (err, INTERMEDIATE_RTOL * max(1.0, float(np.abs(ref).max())))
    bad = {k: v for k, v in worst.items() if not v[0] <= v[1]}
    k = max(worst, key=lambda t: worst[t][0] / worst[t][1])
    print("\n%s: worst tap %s |d| %.2e = %.3f of its bar" % (label, k, worst[k][0], worst[k][0] / worst[k][1]))
    assert not bad, "%s: intermediates out of tolerance: %s" % (label, bad)


def _bf16_layerwise(eng, taps, precision, label):
    """eng: an Engine (its debug taps) or a dict of taps"""
    bad, ratio = {}, {}
    for name, ref in taps.items():
        got = eng[name] if isinstance(eng, dict) else eng.intermediate(name, ref.shape)
        err = float(np.abs(got - ref).max())
        if (name.startswith("lstm_") and precision == "bf16") or name in ("fc1", "logits"):
            tol = (2e-5 if name.startswith("lstm_") else 1e-2) * max(1.0, float(np.abs(ref).max()))
        else:
            u = _ulp(max(1.0, float(np.abs(ref).max())))
            tol = EMU_TAP_TOL_ULPS * u
            mean = float(np.abs(got - ref).mean())
            if not mean <= EMU_TAP_MEAN_ULPS * u:
                bad[name + ":mean"] = (mean, EMU_TAP_MEAN_ULPS * u)
        ratio[name] = err / tol
        if not err <= tol:
            bad[name] = (err, tol)
    k = max(ratio, key=ratio.get)
    print("\n%s: worst tap %s at %.3f of its bar" % (label, k, ratio[k]))
    assert not bad, "%s: bf16 intermediates out of tolerance: %s" % (label, bad)


# ---- (a) layer by layer against the fp32 C oracle -------------------------------------------------------------------------

@pytest.mark.parametrize("precision", ["fp32", "bf16x3"])
@pytest.mark.parametrize("geom", GEOMS)
def test_layerwise_vs_oracle_at_long_windows(long_weights, oracle_taps, geom, precision):
    """Every tap of a debug forward within the fp32 parity bars, for one site and for 37 (37 x W rows: 128-row GEMM tiles
    straddle sites); at 800 also 32 sites (6,400 rows = 50 full tiles)."""
    sizes = [1, 37] + ([32] if geom == G800 else [])
    eng = _engine(long_weights(geom), max_batch=max(sizes), debug=True, slots=1, precision=precision, **geom)
    for n in sizes:
        feats, o_act, o_pred, taps = oracle_taps(geom, n)
        act, pred = eng.run(*(feats[k] for k in KEYS))
        label = "%s %s n=%d" % (geom, precision, n)
        _fp32_layerwise(eng, taps, label)
        _check_outputs(act, pred, o_act, o_pred)
        print("%s: max |d act| %.2e" % (label, float(np.abs(act - o_act).max())))
    eng.close()


# ---- (b) the product path: folded head, captured graphs, looped forwards with a ragged tail --------------------------------

PRODUCT_CASES = [pytest.param(g, p, f, id="%s-%s-%s" % (gid, p, "folded" if f else "three_step"))
                 for g, gid in ((G384, "s384"), (G385, "s385"), (G800, "k13s800"), (G1537, "s1537"))
                 for p in ("fp32", "bf16x3") for f in (True, False)
                 if f or g in (G385, G800)]


@pytest.mark.parametrize("geom,precision,fold", PRODUCT_CASES)
def test_product_path_at_long_windows(long_weights, geom, precision, fold):
    """The engine as call_mods drives it (no debug): max_batch below n, so ds_forward loops and ends on a ragged tail; every
    site against the oracle. fold=False keeps avgpool7 + dense(J, J) + head (bf16x3: the split dense GEMM at J = 12,512)."""
    from oracle import oracle
    n, mb = (101, 48) if geom != G1537 else (40, 16)
    w = long_weights(geom)
    feats = _features(n, geom, seed=900 + n)
    eng = _engine(w, max_batch=mb, precision=precision, fold_fc=fold, **geom)
    act, pred = eng.run(*(feats[k] for k in KEYS))
    o_act, o_pred = oracle.forward(w, feats, "f32", **geom)
    print("\n%s %s fold=%s: max |d act| %.2e" % (geom, precision, fold, float(np.abs(act - o_act).max())))
    _check_outputs(act, pred, o_act, o_pred)
    # graph replay of a recurring size gives the same bits
    a2, p2 = eng.run(*(feats[k][:mb] for k in KEYS))
    assert np.array_equal(a2, act[:mb]) and np.array_equal(p2, pred[:mb])
    eng.close()


# ---- (c) batch-composition independence ------------------------------------------------------------------------------------

@pytest.mark.parametrize("precision", ["fp32", "bf16x3", "bf16", "bf16_all"])
@pytest.mark.parametrize("geom", [pytest.param(G385, id="s385"), pytest.param(G800, id="k13s800")])
def test_long_window_batch_composition_independence(long_weights, geom, precision):
    """One forward of 256 sites against the same sites as a ragged sub-batch at an odd offset: the row tiles of the
    layer-granular GEMMs straddle different sites then, and a site's bits must not notice."""
    feats = _features(256, geom, seed=1256)
    eng = _engine(long_weights(geom), max_batch=256, precision=precision, **geom)
    act, pred = eng.run(*(feats[k] for k in KEYS))
    assert np.isfinite(act).all()
    a2, p2 = eng.run(*(feats[k][37:138] for k in KEYS))
    assert np.array_equal(a2, act[37:138]) and np.array_equal(p2, pred[37:138])
    eng.close()


# ---- (d) bf16 / bf16_all against the emulated statement --------------------------------------------------------------------

@pytest.mark.parametrize("precision", ["bf16", "bf16_all"])
@pytest.mark.parametrize("geom", GEOMS)
def test_bf16_layerwise_vs_emulated_statement_at_long_windows(long_weights, geom, precision):
    """CFG_BCONV / CFG_BCONV_POOL and maxpool_s2_bf16_kernel against oracle/torch_statement.forward_bf16, which rounds to bf16
    at the engine's points; bars of tests/test_gpu_bf16.py."""
    from oracle import torch_statement
    n = 24
    w = long_weights(geom)
    feats = _features(n, geom, seed=1300)
    eng = _engine(w, max_batch=32, debug=True, slots=1, precision=precision, **geom)
    act, pred = eng.run(*(feats[k] for k in KEYS))
    e_act, _, taps = torch_statement.forward_bf16(w, feats, return_taps=True, lstm_bf16=precision == "bf16_all")
    _bf16_layerwise(eng, taps, precision, "%s %s" % (geom, precision))
    assert np.isfinite(act).all()
    print("%s %s: max |d act| %.2e" % (geom, precision, float(np.abs(act - e_act).max())))
    assert np.abs(act - e_act).max() <= EMU_ACT_ATOL
    eng.close()


# ---- (e) DS_TUNE_NO_FUSED at the default geometry --------------------------------------------------------------------------

@pytest.mark.parametrize("precision", ["fp32", "bf16", "bf16_all"])
def test_no_fused_diagnostic_at_the_default_geometry(small_weights, precision):
    """DS_TUNE_NO_FUSED runs the layer-granular path at the default shape: layer by layer against the oracle (fp32) or the
    emulated statement (bf16 modes), and against the fused engine on the same sites. The two paths sum K in different orders,
    so they are held to the parity bars, not to equal bits (include/deepsignal_hip.h). Measured on 37 sites: fp32 3.0e-7 on act,
    3.0e-6 on the worst module tap; bf16 / bf16_all 7.4e-4 on act, 2.3e-2 on module 11 (within 4 bf16 ulps of its range: a
    flipped bf16 rounding carried downstream, as between either path and the statement)."""
    from oracle import oracle, torch_statement
    n = 37
    feats = _features(n, dict(signal_len=360), seed=1400)
    args = [feats[k] for k in KEYS]
    d = spec.net_dims()
    shapes = {"stem_pool": (n, d.w_a, 64), "stem_conv2": (n, d.w_a, 128), "stem_conv3": (n, d.w_a, 256), "logits": (n, 2)}
    shapes.update({"module%d" % m: (n, d.module_width(m), 240) for m in range(1, 12)})
    outs = {}
    for no_fused in (True, False):
        eng = _engine(small_weights, max_batch=64, debug=True, slots=1, precision=precision, no_fused=no_fused)
        act, pred = eng.run(*args)
        outs[no_fused] = (act, pred, {k: eng.intermediate(k, shape) for k, shape in shapes.items()})
        if no_fused:
            label = "no_fused %s" % precision
            if precision == "fp32":
                o_act, o_pred, taps = oracle.forward(small_weights, feats, "f32", taps=True)
                _fp32_layerwise(eng, taps, label)
                _check_outputs(act, pred, o_act, o_pred)
            else:
                e_act, _, taps = torch_statement.forward_bf16(small_weights, feats, return_taps=True, lstm_bf16=precision == "bf16_all")
                _bf16_layerwise(eng, taps, precision, label)
                assert np.abs(act - e_act).max() <= EMU_ACT_ATOL
        eng.close()
    (a_u, p_u, t_u), (a_f, p_f, t_f) = outs[True], outs[False]
    print("\nno_fused vs fused %s: max |d act| %.3e, taps %s" % (precision, float(np.abs(a_u - a_f).max()),
                                                                  {k: "%.1e" % float(np.abs(t_u[k] - t_f[k]).max()) for k in t_u}))
    label = "no_fused vs fused %s" % precision
    if precision == "fp32":
        _fp32_layerwise(t_u, t_f, label)
        _check_outputs(a_u, p_u, a_f, p_f)
    else:
        _bf16_layerwise(t_u, t_f, precision, label)
        assert np.isfinite(a_u).all() and np.abs(a_u - a_f).max() <= EMU_ACT_ATOL


# ---- (f) call_mods at 800 signal columns -----------------------------------------------------------------------------------

class _OracleEngine:
    def __init__(self, weights, geom):
        self.w, self.geom = weights, geom

    def run(self, kmer, means, stds, sanums, signals):
        from oracle import oracle
        feats = {"kmer": np.asarray(kmer, np.int32), "means": np.asarray(means, np.float32),
                 "stds": np.asarray(stds, np.float32), "sanums": np.asarray(sanums, np.float32),
                 "signals": np.asarray(signals, np.float32)}
        return oracle.forward(self.w, feats, "f32", **self.geom)


def test_call_mods_cli_at_800_signal_columns(long_weights, tmp_path):
    """`call_mods -x 13 -y 800`: the native TSV reader at 800 signal columns, batcher, engine and writer, diffed against the
    same harness driven by the oracle (as test_gpu_pipeline.py::test_call_mods_cli_1k_rows_batch32)."""
    from deepsignal_amd import call_modifications as cm, weights as W
    from deepsignal_amd.deepsignal import main
    from test_gpu_pipeline import _write_feature_tsv
    n = 100
    w = long_weights(G800)
    feats = _features(n, G800, seed=1500)
    reads = ["read_%03d" % (i // 7) for i in range(n)]
    tsv, wfile = str(tmp_path / "features.tsv"), str(tmp_path / "model.dsw")
    out_gpu, out_cpu = str(tmp_path / "gpu.tsv"), str(tmp_path / "cpu.tsv")
    _write_feature_tsv(tsv, feats, reads)
    W.save_weights(wfile, w)
    assert main(["call_mods", "-i", tsv, "-m", wfile, "-o", out_gpu, "-x", "13", "-y", "800", "-b", "32", "--nproc", "1",
                 "--engine_batch", "64"]) == 0
    cm.call_mods(tsv, wfile, out_cpu, 13, 800, 32, 0.001, 2, 1, False, True, True, True, None,
                 engine=_OracleEngine(w, G800), f5_batch_num=5)
    g = [l.rstrip("\n").split("\t") for l in open(out_gpu)]
    c = [l.rstrip("\n").split("\t") for l in open(out_cpu)]
    assert len(g) == len(c) == n
    for rg, rc in zip(g, c):
        assert len(rg) == 10 and rg[:6] == rc[:6] and rg[9] == rc[9] and len(rg[9]) == 13
        p0, p1 = float(rg[6]), float(rg[7])
        assert abs(p0 - float(rc[6])) <= 1e-5 and abs(p1 - float(rc[7])) <= 1e-5
        assert abs(p0 + p1 - 1.0) <= 1e-6
        if abs(float(rc[7]) - float(rc[6])) > 1e-3:
            assert rg[8] == rc[8]
    assert [r[4] for r in g] == reads
