"""GPU: one training step with the embedding trained (ds_train_begin_base / ds_train_step_base, lr = 0) against
tests/train_statement_base.py in float64, in the form and with the bars of tests/test_gpu_train_grad.py: dropout masks bit for bit
against ds_train_mask_reference, then loss, prediction and the gradient of all 15 tensors, `modelembedding` among them.

Bars (test_gpu_train_grad.py's, unchanged). Per tensor e = max|g_gpu - g_64| / max|g_64| <= 4 x max(e_32, 1e-6), e_32 = the float32
statement's distance on the same case. Loss: |d| <= 4 x max(|loss_32 - loss_64|, 2^-22 |loss_64|). The rows of the embedding that
no (clamped) code selects must be +0.0 bit patterns. Handles have max_batch = 96, so partial matrix tiles occur; "one" at n = 70,
T = 17 is a single run of 1,190 entries (19 chunks of the reduction), "wide" has runs of one or two entries in hundreds of rows,
"hostile" codes (-7, 1024, 2^31 - 1) land in rows 0 and 1023."""
import numpy as np
import pytest
import torch

import train_statement_base as tsb

pytestmark = pytest.mark.gpu

MAX_BATCH = 96
SEED = 99
#         n   T  keep pos_weight weights   codes
CASES = [(1, 17, 1.0, 1.0, "glorot", "acgt"),
         (5, 17, 1.0, 1.0, "glorot", "one"),
         (33, 17, 0.5, 1.0, "glorot", "wide"),
         (70, 5, 0.5, 3.0, "glorot", "hostile"),
         (70, 17, 0.5, 1.0, "stress", "one")]


def _weights(kind, T):
    from deepsignal_amd import weights
    if kind == "stress":       # saturating gates
        return weights.stress_weights(is_cnn=False, is_base=True, kmer_len=T)
    return weights.random_weights(seed=7, is_cnn=False, is_base=True, kmer_len=T)


@pytest.mark.parametrize("n,T,keep_prob,pos_weight,wkind,ckind", CASES)
def test_gradients_loss_and_masks(n, T, keep_prob, pos_weight, wkind, ckind):
    from deepsignal_amd import engine
    w = _weights(wkind, T)
    feats = tsb.train_features(n, T, seed=1000 + n, kind=ckind)
    labels = np.random.default_rng(n).integers(0, 2, n).astype(np.int32)
    eng = engine.Engine(kmer_len=T, max_batch=MAX_BATCH, is_cnn=False, is_base=True)
    try:
        eng.load_weights(w)
        eng.train_begin(keep_prob=keep_prob, pos_weight=pos_weight, seed=SEED, base=True)
        loss, pred = eng.train_step(feats["means"], feats["stds"], feats["sanums"], labels, lr=0.0, kmer=feats["kmer"])
        masks = {s: eng.train_mask(s, n) for s in engine.MASK_STREAMS}
        grads = eng.train_grads()
        after = eng.train_tensors()
    finally:
        eng.close()
    assert set(grads) == set(tsb.tensor_names()) and tsb.EMBEDDING in grads
    for s, m in masks.items():
        assert (m == engine.train_mask_reference(SEED, 0, s, n, T, keep_prob)).all(), s
        if keep_prob == 1.0:
            assert m.all()
    for name in tsb.tensor_names():     # lr = 0: not a bit of a parameter moves
        assert after[name].tobytes() == np.ascontiguousarray(w[name], np.float32).tobytes(), name

    hit = np.zeros(grads[tsb.EMBEDDING].shape[0], bool)
    hit[tsb.clamp_codes(feats["kmer"])] = True
    assert not grads[tsb.EMBEDDING][~hit].view(np.uint32).any(), "a row no code selects is not all +0.0"
    if ckind == "hostile":
        assert hit[0] and hit[-1] and np.abs(grads[tsb.EMBEDDING][[0, -1]]).max(axis=1).min() > 0

    loss64, logits64, g64 = tsb.step(w, feats, labels, masks, keep_prob, pos_weight, torch.float64)
    loss32, _, g32 = tsb.step(w, feats, labels, masks, keep_prob, pos_weight, torch.float32)
    worst = 0.0
    failures = []
    for name in tsb.tensor_names():
        e, e32 = tsb.rel_err(grads[name], g64[name]), tsb.rel_err(g32[name], g64[name])
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
    assert (pred[decided] == tsb.pred_of(logits64, pos_weight)[decided]).all()
