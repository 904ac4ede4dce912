"""GPU: the forward on non-finite, extreme and out-of-vocabulary inputs (tests/hostile_cases.py), held to the contract of
include/deepsignal_hip.h (ds_forward) and DESIGN.md section 2:

  1. isolation   -- a site's act / pred bits do not depend on any other site's values, in this call or in the call that used
                    the slot before, non-finite values included;
  2. visibility  -- act is NaN exactly where the reference's is (never a finite number in place of a NaN); where the reference
                    is finite the usual bar of the precision holds (an Inf on an LSTM feature saturates the gates; 1e30 is a number);
  3. codes       -- 0..1023 select the embedding row, anything below acts as 0, anything above as 1023, is_base = no ignores them.

References: `oracle.forward(..., "f32")` for the fp32 class (fp32, bf16x3), `torch_statement.forward_bf16` for the bf16 modes;
tests/test_oracle_nonfinite.py pins those to each other on the same cases. The bars are the ones of test_gpu_parity.py
(ACT_ATOL, INTERMEDIATE_RTOL, label margin 1e-3) and test_gpu_bf16.py (EMU_ACT_ATOL, label margin 2e-2), unchanged; a tap's
scale is taken per site, so that the 1e30 sites do not widen the bar of their neighbours.
"""
import numpy as np
import pytest

import hostile_cases as hc
from deepsignal_amd import weights as W
from test_gpu_bf16 import EMU_ACT_ATOL, FP32_LABEL_MARGIN
from test_gpu_parity import ACT_ATOL, FP32_CLASS, INTERMEDIATE_RTOL

pytestmark = pytest.mark.gpu

PRECISIONS = ["fp32", "bf16x3", "bf16", "bf16_all"]
ALL_BATCHES = hc.DIRECTED_BATCHES + ("iso",)


def _engine(weights, geom="default", **kw):
    from deepsignal_amd.engine import Engine
    kw.setdefault("max_batch", hc.MAX_BATCH)
    eng = Engine(**dict(hc.GEOMETRIES[geom], **kw))
    eng.load_weights(weights)
    return eng


def _args(f):
    return [f[k] for k in hc.KEYS]


def _same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


@pytest.fixture(scope="module")
def geom_weights(small_weights):
    return {"default": small_weights,
            "short": W.random_weights(seed=33, lstm_bias_std=0.1, **hc.GEOMETRIES["short"])}


_REF = {}


def _reference(geom_weights, geom, batch, kind):
    """(act, pred, taps or None) of one hostile batch, computed once. kind: "f32" (C oracle, with taps), "bf16" / "bf16_all"
    (torch_statement.forward_bf16). The statements are per-site functions, so the float64 bf16 statement runs on the plain
    batch once and on the five hostile sites of every batch."""
    key = (geom, batch, kind)
    if key in _REF:
        return _REF[key]
    w, g = geom_weights[geom], hc.GEOMETRIES[geom]
    if kind == "f32":
        from oracle import oracle
        out = oracle.forward(w, hc.hostile(geom, batch), "f32", taps=True, **g)
    else:
        from oracle import torch_statement
        if batch == "plain":
            a, p = torch_statement.forward_bf16(w, hc.plain(geom), lstm_bf16=kind == "bf16_all")
        else:
            a, p = (x.copy() for x in _reference(geom_weights, geom, "plain", kind)[:2])
            ha, hp = torch_statement.forward_bf16(w, hc.only_hostile_sites(geom, batch), lstm_bf16=kind == "bf16_all")
            a[list(hc.HOSTILE_AT)], p[list(hc.HOSTILE_AT)] = ha, hp
        out = (a, p, None)
    _REF[key] = out
    return out


def _check_batch(tag, batch, act, pred, r_act, r_pred, atol, margin):
    sel = hc.directed_sites(batch)
    print("%s %s: NaN sites engine %s reference %s; max |d act| over finite entries %.3e" % (
        tag, batch, np.nonzero(np.isnan(act).any(axis=1))[0].tolist(), np.nonzero(np.isnan(r_act).any(axis=1))[0].tolist(),
        float(np.nanmax(np.abs(act[sel] - r_act[sel])))))
    m = hc.compare_nonfinite(act[sel], r_act[sel], atol=atol)
    assert m is None, "%s %s act (cases %s): %s" % (tag, batch, hc.case_names(batch), m)
    srt = np.sort(r_act[sel], axis=1)
    decided = srt[:, -1] - srt[:, -2] > margin            # False for a NaN site
    assert (pred[sel][decided] == r_pred[sel][decided]).all(), (tag, batch)


@pytest.mark.parametrize("geom", list(hc.GEOMETRIES))
@pytest.mark.parametrize("variant", ["folded", "three_step", "debug"])
@pytest.mark.parametrize("precision", FP32_CLASS)
def test_fp32_class_nan_mask_and_values_vs_oracle(geom_weights, precision, variant, geom):
    kw = {"folded": dict(), "three_step": dict(fold_fc=False), "debug": dict(debug=True)}[variant]
    eng = _engine(geom_weights[geom], geom, precision=precision, **kw)
    for batch in hc.DIRECTED_BATCHES:
        act, pred = eng.run(*_args(hc.hostile(geom, batch)))
        r_act, r_pred, taps = _reference(geom_weights, geom, batch, "f32")
        tag = "%s/%s/%s" % (precision, variant, geom)
        _check_batch(tag, batch, act, pred, r_act, r_pred, ACT_ATOL, 1e-3)
        if variant == "debug":
            sel = hc.directed_sites(batch)
            bad = {}
            for name, ref in taps.items():
                m = hc.compare_nonfinite(eng.intermediate(name, ref.shape)[sel], ref[sel], rtol=INTERMEDIATE_RTOL)
                if m:
                    bad[name] = m
            assert not bad, "%s %s taps (cases %s): %s" % (tag, batch, hc.case_names(batch), bad)
    # -0.0 everywhere gives what +0.0 everywhere gives, within the bar
    b, neg, pos = hc.ZERO_TWINS
    act, pred = eng.run(*_args(hc.hostile(geom, b)))
    assert np.abs(act[neg] - act[pos]).max() <= ACT_ATOL
    eng.close()


@pytest.mark.parametrize("geom", list(hc.GEOMETRIES))
@pytest.mark.parametrize("precision", ["bf16", "bf16_all"])
def test_bf16_nan_mask_and_values_vs_emulated_statement(geom_weights, precision, geom):
    eng = _engine(geom_weights[geom], geom, precision=precision)
    for batch in hc.DIRECTED_BATCHES:
        act, pred = eng.run(*_args(hc.hostile(geom, batch)))
        r_act, r_pred, _ = _reference(geom_weights, geom, batch, precision)
        _check_batch("%s/%s" % (precision, geom), batch, act, pred, r_act, r_pred, EMU_ACT_ATOL, FP32_LABEL_MARGIN)
    b, neg, pos = hc.ZERO_TWINS
    act, pred = eng.run(*_args(hc.hostile(geom, b)))
    assert np.abs(act[neg] - act[pos]).max() <= EMU_ACT_ATOL
    eng.close()


@pytest.mark.parametrize("geom", list(hc.GEOMETRIES))
@pytest.mark.parametrize("precision", PRECISIONS)
def test_hostile_sites_leave_their_neighbours_bits_alone(geom_weights, precision, geom):
    """Every finite site of a hostile batch has the exact bits it has in the same batch with the hostile sites replaced by
    plain data: no 0 * x masking of padding or halo rows, no row of a neighbour read past a site's end, in any tile."""
    eng = _engine(geom_weights[geom], geom, precision=precision)
    p_act, p_pred = eng.run(*_args(hc.plain(geom)))
    assert np.isfinite(p_act).all()
    keep = np.array([i for i in range(hc.N) if i not in hc.HOSTILE_AT])
    for batch in ALL_BATCHES:
        act, pred = eng.run(*_args(hc.hostile(geom, batch)))
        diff = keep[(act[keep].view(np.uint32) != p_act[keep].view(np.uint32)).any(axis=1) | (pred[keep] != p_pred[keep])]
        assert diff.size == 0, "%s/%s %s: sites %s changed with their neighbours %s" % (
            precision, geom, batch, diff.tolist(), hc.case_names(batch))
    eng.close()


@pytest.mark.parametrize("geom", list(hc.GEOMETRIES))
@pytest.mark.parametrize("precision", ["fp32", "bf16_all", "bf16x3"])
def test_a_nan_batch_leaves_nothing_behind_in_the_slot(geom_weights, precision, geom):
    """One slot: 128 sites that are NaN in every input fill every workspace row with NaN; the 70-site batch (ragged m-tile,
    partial fused tiles) and a 1-site batch that follow must give the bits of an engine that never saw a NaN."""
    plain = hc.plain(geom)
    fresh = _engine(geom_weights[geom], geom, precision=precision, slots=1)
    f_act, f_pred = fresh.run(*_args(plain))
    f1_act, f1_pred = fresh.run(*(a[:1] for a in _args(plain)))
    fresh.close()
    assert np.isfinite(f_act).all()
    eng = _engine(geom_weights[geom], geom, precision=precision, slots=1)
    nan = hc.all_nan_batch(geom, hc.MAX_BATCH)
    n_act, _ = eng.run(*_args(nan))
    assert np.isnan(n_act).all(), "a site that is NaN in every input came out finite: %s" % n_act[~np.isnan(n_act).all(axis=1)][:4]
    act, pred = eng.run(*_args(plain))
    assert _same_bits(act, f_act) and _same_bits(pred, f_pred)
    eng.run(*_args(nan))
    act, pred = eng.run(*(a[:1] for a in _args(plain)))
    assert _same_bits(act, f1_act) and _same_bits(pred, f1_pred)
    eng.close()


@pytest.mark.parametrize("precision", PRECISIONS)
def test_every_route_gives_the_same_bits_nan_positions_included(small_weights, precision):
    """run, submit / wait, submit_parts and run_device (eager first, then the captured graph replayed) on the hostile batches."""
    import torch
    eng = _engine(small_weights, precision=precision, slots=1)
    dev = torch.device("cuda", 0)
    for batch in ALL_BATCHES:
        f = hc.hostile("default", batch)
        act, pred = eng.run(*_args(f))
        a, p = eng.wait(eng.submit(*_args(f)))
        assert _same_bits(a, act) and _same_bits(p, pred), (batch, "submit")
        cuts = [0, 1, 1, 32, 33, 69, hc.N]
        a, p = eng.wait(eng.submit_parts([tuple(x[s:e] for x in _args(f)) for s, e in zip(cuts[:-1], cuts[1:])]))
        assert _same_bits(a, act) and _same_bits(p, pred), (batch, "submit_parts")
        d = [torch.from_numpy(x).to(dev) for x in _args(f)]
        for rep in range(4):                                   # the size recurs: captured, then replayed at least twice
            d_act = torch.zeros((hc.N, 2), dtype=torch.float32, device=dev)
            d_pred = torch.full((hc.N,), -1, dtype=torch.int32, device=dev)
            eng.run_device(hc.N, *(x.data_ptr() for x in d), d_act.data_ptr(), d_pred.data_ptr())
            eng.sync()
            assert _same_bits(d_act.cpu().numpy(), act) and _same_bits(d_pred.cpu().numpy(), pred), (batch, "run_device", rep)
    eng.close()


def _coded_features():
    """The plain batch with codes drawn from the whole vocabulary; rows 5, 1022 and 1023 are forced to appear (the suite's
    other batches only ever read rows 0..4 of the 1024 the table kernel builds at load)."""
    f = {k: v.copy() for k, v in hc.plain("default").items()}
    f["kmer"] = np.random.default_rng(77).integers(0, 1024, size=f["kmer"].shape, dtype=np.int32)
    f["kmer"][0, 0], f["kmer"][31, 8], f["kmer"][69, 16] = 5, 1022, 1023
    f["kmer"][32, :] = 1023
    return f


@pytest.mark.parametrize("precision", FP32_CLASS)
def test_codes_of_the_whole_vocabulary_vs_oracle(small_weights, precision):
    from oracle import oracle
    f = _coded_features()
    o_act, o_pred, taps = oracle.forward(small_weights, f, "f32", taps=True)
    dbg = _engine(small_weights, precision=precision, debug=True)
    dbg.run(*_args(f))
    for name in ("lstm_fw_l0", "lstm_bw_l0", "lstm_fw_l2", "lstm_bw_l2"):
        err = float(np.abs(dbg.intermediate(name, taps[name].shape) - taps[name]).max())
        assert err <= INTERMEDIATE_RTOL * max(1.0, float(np.abs(taps[name]).max())), (name, err)
    dbg.close()
    eng = _engine(small_weights, precision=precision)
    act, pred = eng.run(*_args(f))
    eng.close()
    assert np.isfinite(act).all() and np.abs(act - o_act).max() <= ACT_ATOL
    decided = np.abs(o_act[:, 1] - o_act[:, 0]) > 1e-3
    assert (pred[decided] == o_pred[decided]).all()


# lstm_xproj_kernel (bf16x3) clamps for the cells whose initial values it computes: first step only, every step, none
@pytest.mark.parametrize("precision,lstm_xproj", [(p, True) for p in PRECISIONS] + [("bf16x3", "all"), ("bf16x3", False)])
def test_out_of_vocabulary_codes_act_as_the_nearest_row(small_weights, precision, lstm_xproj):
    """-1 and INT32_MIN give the bits of 0, 1024 and INT32_MAX those of 1023: the clamp every layer-0 cell and the input
    projection kernel share (reads stay inside the table by construction). The oracle is never given such a code."""
    f = _coded_features()
    lo, hi = np.iinfo(np.int32).min, np.iinfo(np.int32).max
    planted = {(0, 0): -1, (0, 16): hi, (31, 3): lo, (32, 8): 1024, (33, 0): hi, (33, 1): lo, (69, 16): -1, (69, 0): 1024}
    wild, tame = f["kmer"].copy(), f["kmer"].copy()
    for (i, t), code in planted.items():
        wild[i, t] = code
        tame[i, t] = 0 if code < 0 else 1023
    eng = _engine(small_weights, precision=precision, lstm_xproj=lstm_xproj)
    a_t, p_t = eng.run(tame, *_args(f)[1:])
    a_w, p_w = eng.run(wild, *_args(f)[1:])
    eng.close()
    assert np.isfinite(a_t).all() and _same_bits(a_w, a_t) and _same_bits(p_w, p_t)


@pytest.mark.parametrize("precision", FP32_CLASS)
def test_without_is_base_the_codes_are_ignored(precision):
    w = W.random_weights(seed=21, lstm_bias_std=0.1, is_base=False)
    f = hc.plain("default")
    eng = _engine(w, precision=precision, is_base=False)
    act, pred = eng.run(*_args(f))
    rng = np.random.default_rng(3)
    wild = rng.integers(np.iinfo(np.int32).min, np.iinfo(np.int32).max, size=f["kmer"].shape, dtype=np.int32)
    a2, p2 = eng.run(wild, *_args(f)[1:])
    eng.close()
    assert np.isfinite(act).all() and _same_bits(a2, act) and _same_bits(p2, pred)
