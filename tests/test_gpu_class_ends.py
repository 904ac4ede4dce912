"""GPU: the heads at the ends of class_num. ds_create accepts class_num in [1, 16]; the rest of the suite runs 2 and, in a handful
of cases, 3. Held here: C = 1 and C = 16 against the fp32 C oracle (tests/test_oracle.py pins it to both torch statements at these
class counts), kmer_len 5, signal_len 40, max_batch 128, n = 1 / 33 / 70.

The branch each case exists for (ds_kernels.hip):

  fp32 folded        head_folded_kernel, fp32 branch, generic C != 2 path: accv[16] / part[4][16], whose top index only C = 16 uses
  fp32 three-step    head_kernel, generic C != 2 path, same arrays
  bf16x3 three-step  head_kernel adding the `nparts` partial products of the split dense while it reads its row
  bf16_all folded    head_folded_kernel, bf16 branch, against torch_statement.forward_bf16 at the 3e-3 of test_other_kmer_and_signal_lengths
  C = 1              the argmax over one column: pred is constant 0 and act has shape (n, 1)
  C = 16 on device   scatter_outputs_kernel copies n * C words into caller memory: banded outputs (tests/guard_bands.py)
  scaled columns     random weights give every site of a batch the same label; column c of dense_1/kernel centred and scaled
                     (c = 0, 7, 15: first, middle, the top index) makes class c the winner on the sites where its logit is
                     positive, about half of them, so the kernel's argmax produces that value and is checked against the oracle's

Bars: logits at test_gpu_parity's INTERMEDIATE_RTOL, act at its ACT_ATOL, pred equal to the oracle's wherever the two largest
oracle act values of a site differ by more than 1e-3 (test_class_num_three's rule). The scaled columns: see their test."""
import numpy as np
import pytest

import guard_bands as gb
from test_gpu_parity import ACT_ATOL, INTERMEDIATE_RTOL
from test_oracle import end_features

pytestmark = pytest.mark.gpu

KEYS = ("kmer", "means", "stds", "sanums", "signals")
T, S, MAX_BATCH = 5, 40, 128
GEOM = dict(kmer_len=T, signal_len=S)
SIZES = (1, 33, 70)
ENGINES = {"fp32-folded": dict(precision="fp32"),
           "fp32-three_step": dict(precision="fp32", fold_fc=False),
           "bf16x3-three_step": dict(precision="bf16x3", fold_fc=False, split_dense_min_n=1)}
LOGIT_STD = 1.5

_CASES = {}


def _case(C, column=None):
    """Weights (column `column` of the last layer scaled, if given), 70 sites, the fp32 oracle on them: computed once."""
    if (C, column) not in _CASES:
        from deepsignal_amd import weights as W
        from oracle import oracle
        w = W.random_weights(seed=8, lstm_bias_std=0.1, class_num=C, **GEOM)
        feats = end_features(max(SIZES), 19, T, S)
        if column is not None:
            # every logit of a random-weights batch has one sign (the joint features' common mode), so a plain factor makes the column
            # win everywhere or nowhere: weights.centred_head takes the batch mean out of the column's direction and scales it to
            # a standard deviation of LOGIT_STD over the batch, against |logits| < 1 in the other columns
            _, _, taps = oracle.forward(w, feats, "f64", taps=True, class_num=C, **GEOM)
            assert float(np.abs(taps["logits"]).max()) < 1.0
            w = dict(w)
            k = w["dense_1/kernel"].copy()
            k[:, column] = W.centred_head(taps["fc1"], k[:, column], LOGIT_STD, 800 + column)[:, 0]
            w["dense_1/kernel"] = k
        _CASES[(C, column)] = (w, feats, oracle.forward(w, feats, "f32", taps=True, class_num=C, **GEOM))
        if column is not None:
            _CASES[(C, column)] += (oracle.forward(w, feats, "f64", taps=True, class_num=C, **GEOM),)
    return _CASES[(C, column)]


def _engine(w, C, **kw):
    from deepsignal_amd.engine import Engine
    kw.setdefault("slots", 1)
    eng = Engine(max_batch=MAX_BATCH, class_num=C, **GEOM, **kw)
    eng.load_weights(w)
    return eng


def _args(feats, n):
    return [feats[k][:n] for k in KEYS]


def _decided(o_act):
    if o_act.shape[1] == 1:
        return np.ones(len(o_act), bool)
    srt = np.sort(o_act, axis=1)
    return srt[:, -1] - srt[:, -2] > 1e-3


def _check_head(eng, feats, n, C, o_act, o_pred, o_logits, tag):
    act, pred = eng.run(*_args(feats, n))
    logits = eng.intermediate("logits", (n, C))
    assert act.shape == (n, C) and act.dtype == np.float32 and pred.shape == (n,) and pred.dtype == np.int32
    e_l, e_a = float(np.abs(logits - o_logits[:n]).max()), float(np.abs(act - o_act[:n]).max())
    print("%s C=%d n=%d |d logits| %.3g |d act| %.3g" % (tag, C, n, e_l, e_a))
    assert np.isfinite(logits).all() and e_l <= INTERMEDIATE_RTOL * max(1.0, float(np.abs(o_logits[:n]).max()))
    assert np.isfinite(act).all() and e_a <= ACT_ATOL
    assert ((pred >= 0) & (pred < C)).all()
    d = _decided(o_act[:n])
    assert (pred[d] == o_pred[:n][d]).all()
    if C == 1:
        assert not pred.any()
    return act, pred


@pytest.mark.parametrize("tag", sorted(ENGINES))
@pytest.mark.parametrize("C", [1, 16])
def test_fp32_class_heads_against_the_oracle(C, tag):
    w, feats, (o_act, o_pred, o_taps) = _case(C)
    assert o_act.shape == (max(SIZES), C)
    eng = _engine(w, C, **ENGINES[tag])
    try:
        for n in SIZES:
            _check_head(eng, feats, n, C, o_act, o_pred, o_taps["logits"], tag)
    finally:
        eng.close()


@pytest.mark.parametrize("tag", sorted(ENGINES))
@pytest.mark.parametrize("column", [0, 7, 15])
def test_every_scaled_column_wins_and_is_the_oracles_label(column, tag):
    """A centred column cancels the features' common mode, and with it digits: on these weights the fp32 ORACLE's logits are 1e-4 from
    the float64 oracle's, so the bars are the ones tests/test_gpu_stress.py holds centred heads to, against float64: logits within
    NOISE_FACTOR x the fp32 oracle's own distance + FLOOR_REL of their scale, act within OUT_ATOL, labels equal beyond LABEL_MARGIN."""
    from test_gpu_stress import FLOOR_REL, LABEL_MARGIN, NOISE_FACTOR, OUT_ATOL
    C = 16
    w, feats, (_, _, t32), (a64, p64, t64) = _case(C, column)
    n = max(SIZES)
    srt = np.sort(a64, axis=1)
    decided = srt[:, -1] - srt[:, -2] > LABEL_MARGIN
    wins = (p64 == column) & decided
    assert n // 5 <= wins.sum() <= n - n // 5, "column %d should win on a good part of the sites: %d of %d" % (column, wins.sum(), n)
    assert len(set(p64[decided & ~wins].tolist())) == 1      # ... and the class random weights favour on the others
    scale = max(1.0, float(np.abs(t64["logits"]).max()))
    tol = NOISE_FACTOR * float(np.abs(t32["logits"] - t64["logits"]).max()) + FLOOR_REL * scale
    eng = _engine(w, C, **ENGINES[tag])
    try:
        for m in (33, n):
            act, pred = eng.run(*_args(feats, m))
            logits = eng.intermediate("logits", (m, C))
            e_l, e_a = float(np.abs(logits - t64["logits"][:m]).max()), float(np.abs(act - a64[:m]).max())
            print("%s column %d n=%d vs f64: |d logits| %.3g (tol %.3g) |d act| %.3g" % (tag, column, m, e_l, tol, e_a))
            assert np.isfinite(logits).all() and e_l <= tol
            assert np.isfinite(act).all() and e_a <= OUT_ATOL
            assert (pred[decided[:m]] == p64[:m][decided[:m]]).all()
            assert (pred[wins[:m]] == column).all() and wins[:m].any()
    finally:
        eng.close()


@pytest.mark.parametrize("C", [1, 16])
def test_bf16_all_folded_head_against_its_statement(C):
    from oracle import torch_statement
    w, feats, _ = _case(C)
    eng = _engine(w, C, precision="bf16_all")
    try:
        for n in SIZES:
            act, pred = eng.run(*_args(feats, n))
            e_act, e_pred = torch_statement.forward_bf16(w, {k: feats[k][:n] for k in KEYS}, lstm_bf16=True)
            d = float(np.abs(act - e_act).max())
            print("bf16_all C=%d n=%d |d act| %.3g" % (C, n, d))
            assert act.shape == e_act.shape == (n, C) and np.isfinite(act).all() and d <= 3e-3
            assert ((pred >= 0) & (pred < C)).all()
            if C > 1:       # two values each within 3e-3 of the statement's keep their order when those are more than 6e-3 apart
                srt = np.sort(e_act, axis=1)
                far = srt[:, -1] - srt[:, -2] > 2 * 3e-3
                assert (pred[far] == e_pred[far]).all()
            else:
                assert not pred.any()
    finally:
        eng.close()


@pytest.mark.parametrize("slots", [1, 3])
@pytest.mark.parametrize("tag", ["fp32-folded", "fp32-three_step"])
def test_sixteen_classes_on_the_device_write_n_times_16_floats(tag, slots):
    """ds_forward_device at C = 16 into banded device tensors: four runs per size (eager, captured, replayed twice); every one of the
    n * 16 floats and n labels is written, the bands stay intact and the bytes are those of ds_forward on the same rows."""
    import torch
    C = 16
    w, feats, _ = _case(C)
    eng = _engine(w, C, slots=slots, **ENGINES[tag])
    dev = torch.device("cuda", 0)
    try:
        for n in SIZES:
            act, pred = eng.run(*_args(feats, n))
            d_in = [torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in _args(feats, n)]
            d_act = gb.banded((n, C), np.float32, MAX_BATCH, device="cuda:0", what="d_act")
            d_pred = gb.banded((n,), np.int32, MAX_BATCH, device="cuda:0", what="d_pred")
            torch.cuda.synchronize()
            for rep in range(4):
                d_act.refill()
                d_pred.refill()
                torch.cuda.synchronize()
                rc = gb.call(eng._lib, "ds_forward_device", eng._h, n, *(x.data_ptr() for x in d_in), d_act, d_pred)
                assert rc == 0, eng._lib.ds_last_error(eng._h)
                eng.sync()
                d_act.check("d_act, n = %d, run %d" % (n, rep))
                d_pred.check("d_pred, n = %d, run %d" % (n, rep))
                assert d_act.written(n * C) and d_pred.written(n)
                gb.same_bytes(d_act, act, "d_act, n = %d, run %d" % (n, rep))
                gb.same_bytes(d_pred, pred, "d_pred, n = %d, run %d" % (n, rep))
    finally:
        eng.close()
