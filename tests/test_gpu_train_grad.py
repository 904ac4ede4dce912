"""GPU: one training step of the RNN-only model (ds_train_step, lr = 0) against tests/train_statement.py in float64: dropout masks
bit for bit against ds_train_mask_reference, then loss, prediction and the gradient of all 14 tensors.

Bars. Per tensor e = max|g_gpu - g_64| / max|g_64| <= 4 x max(e_32, 1e-6), e_32 = the float32 statement's distance on the same
case (computed here). 1e-6 is the float32 statement's own level (measured 4e-7 .. 1e-6 on these shapes); the factor 4 because the
GPU adds the same terms in another order (matrix-tile order, n T-long reductions): another draw from the same error distribution.
Loss: |d| <= 4 x max(|loss_32 - loss_64|, 2^-22 |loss_64|). Handles have max_batch = 96, so partial matrix tiles occur."""
import numpy as np
import pytest
import torch

import train_statement as ts

pytestmark = pytest.mark.gpu

MAX_BATCH = 96
SEED = 99
#         n   T  keep pos_weight weights   labels
CASES = [(1, 17, 1.0, 1.0, "glorot", "ones"),
         (5, 17, 1.0, 1.0, "glorot", "zeros"),
         (33, 17, 0.5, 1.0, "glorot", "mixed"),
         (70, 5, 0.5, 3.0, "glorot", "mixed"),
         (64, 17, 0.5, 1.0, "stress", "ones")]


def _weights(kind, T):
    from deepsignal_amd import weights
    if kind == "stress":       # saturating gates
        return weights.stress_weights(is_cnn=False, is_base=False, kmer_len=T)
    return weights.random_weights(seed=7, is_cnn=False, is_base=False, kmer_len=T)


def _labels(kind, n):
    if kind == "mixed":
        return np.random.default_rng(n).integers(0, 2, n).astype(np.int32)
    return (np.ones if kind == "ones" else np.zeros)(n, np.int32)


@pytest.mark.parametrize("n,T,keep_prob,pos_weight,wkind,lkind", CASES)
def test_gradients_loss_and_masks(n, T, keep_prob, pos_weight, wkind, lkind):
    from deepsignal_amd import engine
    w = _weights(wkind, T)
    feats = ts.train_features(n, T, seed=1000 + n)
    labels = _labels(lkind, n)
    eng = engine.Engine(kmer_len=T, max_batch=MAX_BATCH, is_cnn=False, is_base=False)
    try:
        eng.load_weights(w)
        eng.train_begin(keep_prob=keep_prob, pos_weight=pos_weight, seed=SEED)
        loss, pred = eng.train_step(feats["means"], feats["stds"], feats["sanums"], labels, lr=0.0)
        masks = {s: eng.train_mask(s, n) for s in engine.MASK_STREAMS}
        grads = eng.train_grads()
        after = eng.train_tensors()
    finally:
        eng.close()
    for s, m in masks.items():
        assert (m == engine.train_mask_reference(SEED, 0, s, n, T, keep_prob)).all(), s
        if keep_prob == 1.0:
            assert m.all()
    for name in ts.tensor_names():     # lr = 0: not a bit of a parameter moves
        assert after[name].tobytes() == np.ascontiguousarray(w[name], np.float32).tobytes(), name

    loss64, logits64, g64 = ts.step(w, feats, labels, masks, keep_prob, pos_weight, torch.float64)
    loss32, _, g32 = ts.step(w, feats, labels, masks, keep_prob, pos_weight, torch.float32)
    worst = 0.0
    failures = []
    for name in ts.tensor_names():
        e, e32 = ts.rel_err(grads[name], g64[name]), ts.rel_err(g32[name], g64[name])
        bar = 4 * max(e32, 1e-6)
        print("n=%d T=%d %-50s e_gpu %.3g  e_32 %.3g  bar %.3g" % (n, T, name, e, e32, bar))
        worst = max(worst, e)
        if not e <= bar:
            failures.append((name, e, bar))
    loss_bar = 4 * max(abs(loss32 - loss64), 2.0 ** -22 * abs(loss64))
    print("n=%d T=%d loss gpu %.9g  f64 %.9g  |d| %.3g  bar %.3g  worst gradient distance %.3g" % (n, T, loss, loss64, abs(loss - loss64), loss_bar, worst))
    assert not failures, failures
    assert np.isfinite(loss) and abs(loss - loss64) <= loss_bar
    gap = np.abs(logits64[:, 1] - logits64[:, 0]) if pos_weight == 1.0 else np.abs(logits64[:, 1])
    decided = gap > loss_bar
    assert (pred[decided] == ts.pred_of(logits64, pos_weight)[decided]).all()
