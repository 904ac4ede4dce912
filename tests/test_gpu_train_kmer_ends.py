"""GPU: the training step (ds_train_step / ds_train_step_base, ds_train_eval) at the ends of kmer_len, in the form and with the bars
of tests/test_gpu_train_grad.py and tests/test_gpu_train_base_grad.py, which run T = 17 and T = 5: masks bit for bit against
ds_train_mask_reference, lr = 0 leaves every parameter's bytes alone, loss, pred and every gradient against the float64 statement
(tests/train_statement.py, tests/train_statement_base.py; tests/test_train_statement*.py hold them to central differences at T = 1, 3).

Bars, unchanged: per tensor e = max|g_gpu - g_64| / max|g_64| <= 4 x max(e_32, 1e-6) with e_32 the float32 statement's distance on
the same case; loss |d| <= 4 x max(|loss_32 - loss_64|, 2^-22 |loss_64|). New here: an LSTM `kernel` is held in two parts, the
input rows [0:in] and the recurrent rows [in:], each by its own max|g_64| and its own e_32: under one tensor-wide scale a wrong
recurrent half hides behind the larger input half.

The branch of dstr::Trainer::step (ds_train.hip) each case exists for:

  T = 1    `if (T > 1)` skips the recurrent-half weight-gradient product and reduce_slabs_kernel runs with ns = T - 1 = 0: the rows
           [in:] of all six kernels' gradients are exactly 0.0f, whatever `slab` (reused scratch) held; every `t > 0` product of the
           forward and backward sweeps is skipped, c.last is true for every cell and DH is never read
  n = 1, T = 1, is_base    the embedding-gradient sort at total = n * T = 1: one chunk, one non-zero row
  T = 3    = the number of layers: two recurrent steps, the shortest sum over slabs
  T = 65   the longest here: 64 slabs per recurrent half, activations of 6 x 65 cells (ds_train_begin refuses no T)
  stress   saturating gates at T = 3
  Adam at T = 1    m = v = 0 on the all-zero recurrent rows gives a zero update: they keep their initial bytes
  ds_train_eval at T = 1, 3    changes no tensor, and after ds_train_sync_weights the inference forward's act is sigmoid of its logits
"""
import numpy as np
import pytest
import torch

import train_statement as ts
import train_statement_base as tsb
from deepsignal_amd import spec

pytestmark = pytest.mark.gpu

MAX_BATCH = 96
SEED = 99
HID = spec.HIDDEN
#         n   T  keep pos_weight weights   codes (is_base)
CASES = [(1, 1, 1.0, 1.0, "glorot", "acgt"),
         (33, 1, 0.5, 3.0, "glorot", "wide"),
         (70, 3, 0.5, 1.0, "glorot", "hostile"),
         (33, 3, 1.0, 1.0, "stress", "one"),
         (33, 65, 0.5, 1.0, "glorot", "wide")]
LSTM_KERNELS = [spec.lstm_tensor(d, l, "kernel") for d in ("fw", "bw") for l in range(spec.LSTM_LAYERS)]


def _st(is_base):
    return tsb if is_base else ts


def _weights(kind, T, is_base):
    from deepsignal_amd import weights
    if kind == "stress":       # saturating gates
        return weights.stress_weights(is_cnn=False, is_base=is_base, kmer_len=T)
    return weights.random_weights(seed=7, is_cnn=False, is_base=is_base, kmer_len=T)


def _engine(w, T, is_base):
    from deepsignal_amd.engine import Engine
    eng = Engine(kmer_len=T, max_batch=MAX_BATCH, is_cnn=False, is_base=is_base)
    eng.load_weights(w)
    return eng


def _batch(n, T, seed, kind="acgt"):
    return tsb.train_features(n, T, seed, kind), np.random.default_rng(seed + 1).integers(0, 2, n).astype(np.int32)


def _step(eng, feats, labels, lr, is_base):
    return eng.train_step(feats["means"], feats["stds"], feats["sanums"], labels, lr, kmer=feats["kmer"] if is_base else None)


def _parts(name, g):
    """[(label, array)]: an LSTM kernel as its input rows and its recurrent rows, any other tensor whole."""
    if name in LSTM_KERNELS:
        cut = g.shape[0] - HID
        return [(name + " [0:in]", g[:cut]), (name + " [in:]", g[cut:])]
    return [(name, g)]


def _check_gradients(tag, st, grads, g64, g32, T):
    failures, worst = [], 0.0
    for name in st.tensor_names():
        for (label, g), (_, r64), (_, r32) in zip(_parts(name, grads[name]), _parts(name, g64[name]), _parts(name, g32[name])):
            if T == 1 and label.endswith("[in:]"):
                assert not r64.any() and not r32.any()
                if not (g == 0).all():
                    failures.append((label, "not all 0.0f: %d elements, max |g| %g" % (int((g != 0).sum()), float(np.abs(g).max()))))
                continue
            e, e32 = st.rel_err(g, r64), st.rel_err(r32, r64)
            bar = 4 * max(e32, 1e-6)
            print("%s %-58s e_gpu %.3g  e_32 %.3g  bar %.3g" % (tag, label, e, e32, bar))
            worst = max(worst, e)
            if not e <= bar:
                failures.append((label, e, bar))
    return failures, worst


@pytest.mark.parametrize("is_base", [False, True], ids=["rnn", "base"])
@pytest.mark.parametrize("n,T,keep_prob,pos_weight,wkind,ckind", CASES)
def test_gradients_loss_and_masks(n, T, keep_prob, pos_weight, wkind, ckind, is_base):
    from deepsignal_amd import engine
    st = _st(is_base)
    w = _weights(wkind, T, is_base)
    feats, labels = _batch(n, T, 1000 + n, ckind)
    eng = _engine(w, T, is_base)
    try:
        eng.train_begin(keep_prob=keep_prob, pos_weight=pos_weight, seed=SEED, base=is_base)
        loss, pred = _step(eng, feats, labels, 0.0, is_base)
        masks = {s: eng.train_mask(s, n) for s in engine.MASK_STREAMS}
        grads = eng.train_grads()
        after = eng.train_tensors()
    finally:
        eng.close()
    assert set(grads) == set(st.tensor_names())
    for s, m in masks.items():
        assert (m == engine.train_mask_reference(SEED, 0, s, n, T, keep_prob)).all(), s
        if keep_prob == 1.0:
            assert m.all()
    for name in st.tensor_names():     # lr = 0: not a bit of a parameter moves
        assert after[name].tobytes() == np.ascontiguousarray(w[name], np.float32).tobytes(), name
    if is_base:
        hit = np.zeros(grads[tsb.EMBEDDING].shape[0], bool)
        hit[tsb.clamp_codes(feats["kmer"])] = True
        assert not grads[tsb.EMBEDDING][~hit].view(np.uint32).any(), "a row no code selects is not all +0.0"

    loss64, logits64, g64 = st.step(w, feats, labels, masks, keep_prob, pos_weight, torch.float64)
    loss32, _, g32 = st.step(w, feats, labels, masks, keep_prob, pos_weight, torch.float32)
    tag = "n=%d T=%d %s" % (n, T, "base" if is_base else "rnn")
    failures, worst = _check_gradients(tag, st, grads, g64, g32, T)
    loss_bar = 4 * max(abs(loss32 - loss64), 2.0 ** -22 * abs(loss64))
    print("%s loss gpu %.9g  f64 %.9g  |d| %.3g  bar %.3g  worst gradient distance %.3g" % (tag, loss, loss64, abs(loss - loss64), loss_bar, worst))
    assert not failures, failures
    assert np.isfinite(loss) and abs(loss - loss64) <= loss_bar
    gap = np.abs(logits64[:, 1] - logits64[:, 0]) if pos_weight == 1.0 else np.abs(logits64[:, 1])
    decided = gap > loss_bar
    assert (pred[decided] == st.pred_of(logits64, pos_weight)[decided]).all()


def _recurrent_rows(grads):
    return {name: grads[name][grads[name].shape[0] - HID:] for name in LSTM_KERNELS}


@pytest.mark.parametrize("is_base", [False, True], ids=["rnn", "base"])
def test_recurrent_rows_are_zero_at_one_step_whatever_the_scratch_held(is_base):
    """`slab` is scratch every weight-gradient product writes: a 70-row T = 1 step right after a step on ANOTHER handle (T = 3, whose
    freed or neighbouring memory is full of slabs), then after a 33-row step with other rows on the SAME handle (whose input-half
    slabs are in `slab`). The second step's gradient is also the statement's for its 70 rows alone."""
    from deepsignal_amd import engine
    st = _st(is_base)
    w3, w1 = _weights("glorot", 3, is_base), _weights("glorot", 1, is_base)
    other = _engine(w3, 3, is_base)
    eng = None
    try:
        other.train_begin(keep_prob=0.5, seed=3, base=is_base)
        f3, l3 = _batch(70, 3, 40)
        _step(other, f3, l3, 1e-3, is_base)
        assert any(r.any() for r in _recurrent_rows(other.train_grads()).values())      # T = 3 has recurrent gradients
        eng = _engine(w1, 1, is_base)
        eng.train_begin(keep_prob=0.5, seed=8, base=is_base)
        fa, la = _batch(70, 1, 41)
        _step(eng, fa, la, 0.0, is_base)
        for name, rec in _recurrent_rows(eng.train_grads()).items():
            assert rec.shape == (HID, 4 * HID) and (rec == 0).all(), ("first step", name, int((rec != 0).sum()))
        fb, lb = _batch(33, 1, 42, "wide")
        _step(eng, fb, lb, 0.0, is_base)
        fc, lc = _batch(70, 1, 43, "hostile")
        loss, _ = _step(eng, fc, lc, 0.0, is_base)
        grads = eng.train_grads()
    finally:
        other.close()
        if eng is not None:
            eng.close()
    for name, rec in _recurrent_rows(grads).items():
        assert (rec == 0).all(), ("third step", name, int((rec != 0).sum()))
    masks = {s: engine.train_mask_reference(8, 2, s, 70, 1, 0.5) for s in engine.MASK_STREAMS}
    loss64, _, g64 = st.step(w1, fc, lc, masks, 0.5, 1.0, torch.float64)
    loss32, _, g32 = st.step(w1, fc, lc, masks, 0.5, 1.0, torch.float32)
    failures, _ = _check_gradients("after two steps, %s" % ("base" if is_base else "rnn"), st, grads, g64, g32, 1)
    assert not failures, failures
    assert abs(loss - loss64) <= 4 * max(abs(loss32 - loss64), 2.0 ** -22 * abs(loss64))


@pytest.mark.parametrize("code", [2, -7, 2 ** 31 - 1])
def test_one_entry_gives_the_embedding_gradient_one_row(code):
    """n = 1, T = 1, is_base: the sort of the embedding gradient runs at total = 1. Exactly one row is non-zero, the (clamped)
    code's; it is the statement's, and every other row is 0.0f."""
    w = _weights("glorot", 1, True)
    feats, _ = _batch(1, 1, 50)
    feats["kmer"][0, 0] = code
    labels = np.array([1], np.int32)
    eng = _engine(w, 1, True)
    try:
        eng.train_begin(keep_prob=1.0, seed=1, base=True)
        _step(eng, feats, labels, 0.0, True)
        g = eng.train_grad(tsb.EMBEDDING)
    finally:
        eng.close()
    row = int(tsb.clamp_codes(feats["kmer"])[0, 0])
    _, _, g64 = tsb.step(w, feats, labels, None, 1.0, 1.0, torch.float64)
    _, _, g32 = tsb.step(w, feats, labels, None, 1.0, 1.0, torch.float32)
    assert list(np.nonzero(np.abs(g64[tsb.EMBEDDING]).max(axis=1))[0]) == [row]
    assert list(np.nonzero(np.abs(g).max(axis=1))[0]) == [row]
    others = np.arange(g.shape[0]) != row
    assert (g[others] == 0).all()
    e, e32 = tsb.rel_err(g[row], g64[tsb.EMBEDDING][row]), tsb.rel_err(g32[tsb.EMBEDDING][row], g64[tsb.EMBEDDING][row])
    print("code %d -> row %d: e_gpu %.3g e_32 %.3g" % (code, row, e, e32))
    assert e <= 4 * max(e32, 1e-6)


@pytest.mark.parametrize("is_base", [False, True], ids=["rnn", "base"])
def test_adam_at_one_step(is_base):
    """tests/test_gpu_train_step.py::test_adam_in_isolation at T = 1: three steps, the expected parameters are the numpy float64 Adam
    applied to the GPU's own gradients; bar one ulp of theta plus 1e-5 lr. The recurrent rows have m = v = 0 throughout: their update
    is 0 / (0 + epsilon) and they keep their initial bytes."""
    st = _st(is_base)
    w, lr, T = _weights("glorot", 1, is_base), 1e-3, 1
    eng = _engine(w, T, is_base)
    try:
        eng.train_begin(keep_prob=0.5, seed=1, base=is_base)
        opt = ts.Adam({k: w[k] for k in st.tensor_names()})
        for s in range(3):
            feats, labels = _batch(16, T, 50 + s)
            _step(eng, feats, labels, lr, is_base)
            opt.update(eng.train_grads(), lr)
            got = eng.train_tensors()
            for name in st.tensor_names():
                bar = np.spacing(np.abs(got[name])).astype(np.float64) + 1e-5 * lr
                d = np.abs(got[name].astype(np.float64) - opt.p[name])
                print("step %d %-50s worst |d| / bar %.3g" % (s, name, float((d / bar).max())))
                assert (d <= bar).all(), (s, name, float(d.max()))
            for name in LSTM_KERNELS:
                cut = got[name].shape[0] - HID
                assert got[name][cut:].tobytes() == np.ascontiguousarray(w[name][cut:], np.float32).tobytes(), (s, name)
                assert (got[name][:cut] != w[name][:cut]).any(), (s, name)
            opt.p = {k: v.astype(np.float64) for k, v in got.items()}     # the next step starts from the GPU's own fp32 parameters
    finally:
        eng.close()


@pytest.mark.parametrize("is_base", [False, True], ids=["rnn", "base"])
@pytest.mark.parametrize("T", [1, 3])
def test_eval_changes_nothing_and_is_the_forward(T, is_base):
    """The form of tests/test_gpu_train_base_step.py::test_eval_changes_nothing_and_is_the_forward."""
    from deepsignal_amd import engine
    from test_gpu_parity import ACT_ATOL
    st = _st(is_base)
    w, n = _weights("glorot", T, is_base), 70
    f0, l0 = _batch(n, T, 30)
    fv, lv = _batch(33, T, 32, "hostile")
    eng = _engine(w, T, is_base)
    try:
        eng.train_begin(keep_prob=0.5, pos_weight=1.0, seed=4, base=is_base)
        _step(eng, f0, l0, 1e-3, is_base)
        before = (eng.train_tensors(), eng.train_grads(), {s: eng.train_mask(s, n) for s in engine.MASK_STREAMS})
        loss, pred, logits = eng.train_eval(fv["means"], fv["stds"], fv["sanums"], lv, kmer=fv["kmer"] if is_base else None)
        after = (eng.train_tensors(), eng.train_grads(), {s: eng.train_mask(s, n) for s in engine.MASK_STREAMS})
        for b, a in zip(before, after):
            for name in b:
                assert b[name].tobytes() == a[name].tobytes(), name
        # the float64 statement on the same parameters, keep_prob 1, every mask kept: the gradient test's loss bar, the same form on the logits
        l64, g64, _ = st.step(before[0], fv, lv, None, 1.0, 1.0, torch.float64)
        l32, g32, _ = st.step(before[0], fv, lv, None, 1.0, 1.0, torch.float32)
        loss_bar = 4 * max(abs(l32 - l64), 2.0 ** -22 * abs(l64))
        logit_bar = 4 * max(float(np.abs(g32 - g64).max()), 2.0 ** -22 * float(np.abs(g64).max()))
        print("T=%d eval loss gpu %.9g f64 %.9g |d| %.3g bar %.3g; logits |d| %.3g bar %.3g" %
              (T, loss, l64, abs(loss - l64), loss_bar, float(np.abs(logits - g64).max()), logit_bar))
        assert logits.shape == (33, 2) and abs(loss - l64) <= loss_bar and np.abs(logits - g64).max() <= logit_bar
        decided = np.abs(g64[:, 1] - g64[:, 0]) > logit_bar
        assert (pred[decided] == st.pred_of(g64, 1.0)[decided]).all()
        # after the hand-over the inference forward computes sigmoid of what the evaluation pass computes
        eng.train_sync_weights()
        kmer = fv["kmer"] if is_base else np.zeros((33, T), np.int32)
        act, _ = eng.run(kmer, fv["means"], fv["stds"], fv["sanums"], np.zeros((33, 360), np.float32))
        assert act.shape == (33, 2) and np.abs(act - 1.0 / (1.0 + np.exp(-logits.astype(np.float64)))).max() <= ACT_ATOL
        assert any((before[0][k] != w[k]).any() for k in st.tensor_names())          # the parameters it handed over are trained ones
    finally:
        eng.close()
