"""CPU: tests/train_statement_base.py (the oracle of the GPU training step with the embedding) held to first principles, the way
tests/test_train_statement.py holds train_statement: autograd against central differences in float64, `modelembedding` included;
and what the lookup's gradient is where no code points."""
import numpy as np
import pytest
import torch

import train_statement_base as tsb
from deepsignal_amd import spec, weights

N, T = 3, 5


@pytest.fixture(scope="module")
def case():
    w = weights.random_weights(seed=7, is_cnn=False, is_base=True, kmer_len=T, lstm_bias_std=0.1)
    feats = tsb.train_features(N, T, seed=11, kind="hostile")
    labels = np.array([0, 1, 1], np.int32)
    rng = np.random.default_rng(5)
    masks = {s: (rng.random(m.shape) < 0.5).astype(np.uint8) for s, m in tsb.no_masks(N, T).items()}
    return w, feats, labels, masks


@pytest.mark.parametrize("pos_weight", [1.0, 3.0])
def test_autograd_matches_central_differences(case, pos_weight):
    _central_differences(case, pos_weight)


@pytest.mark.parametrize("pos_weight", [1.0, 3.0])
@pytest.mark.parametrize("n,T", [(1, 1), (4, 1), (4, 3)])
def test_autograd_matches_central_differences_at_the_ends_of_kmer_len(n, T, pos_weight):
    """T = 1: the rows [in:] of every LSTM kernel have a gradient of exactly zero, and at n = 1 the embedding's gradient has one
    non-zero row, the (clamped) code's. T = 3 = the number of layers. tests/test_gpu_train_kmer_ends.py holds the GPU step to the
    statement at these lengths."""
    w = weights.random_weights(seed=7, is_cnn=False, is_base=True, kmer_len=T, lstm_bias_std=0.1)
    feats = tsb.train_features(n, T, seed=11, kind="hostile")
    labels = (np.arange(n) % 2 == 0).astype(np.int32)
    rng = np.random.default_rng(5)
    masks = {s: (rng.random(m.shape) < 0.5).astype(np.uint8) for s, m in tsb.no_masks(n, T).items()}
    if n == 1:      # a random two-entry mask on the logits can drop the whole loss
        masks = tsb.no_masks(n, T)
    grads = _central_differences((w, feats, labels, masks), pos_weight, ends=False)
    for direction in ("fw", "bw"):
        for layer in range(spec.LSTM_LAYERS):
            g = grads[spec.lstm_tensor(direction, layer, "kernel")]
            rec = g[g.shape[0] - spec.HIDDEN:]
            assert np.abs(g[:g.shape[0] - spec.HIDDEN]).max() > 0
            assert (rec == 0).all() if T == 1 else np.abs(rec).max() > 0
    if n * T == 1:
        row = int(tsb.clamp_codes(feats["kmer"])[0, 0])
        assert list(np.nonzero(np.abs(grads[tsb.EMBEDDING]).max(axis=1))[0]) == [row]


def _central_differences(case, pos_weight, ends=True):
    w, feats, labels, masks = case
    _, _, grads = tsb.step(w, feats, labels, masks, keep_prob=0.5, pos_weight=pos_weight)
    rng = np.random.default_rng(1)

    def loss_at(w64):
        wt = {k: torch.from_numpy(v) for k, v in w64.items()}
        return float(tsb.loss_of(tsb.logits_of(wt, feats, masks, 0.5, torch.float64), labels, pos_weight))

    w64 = {k: np.asarray(w[k], np.float64).copy() for k in tsb.tensor_names()}
    eps = 1e-5
    for name in tsb.tensor_names():
        g = grads[name]
        # the coordinates that matter most (largest gradient) and a few at random
        flat = list(np.argsort(np.abs(g).ravel())[-2:]) + list(rng.integers(0, g.size, 2))
        if name == tsb.EMBEDDING:      # ... and one in each row the codes select, the clamped ones among them
            rows = np.unique(tsb.clamp_codes(feats["kmer"]))
            assert not ends or (0 in rows and spec.VOCAB_SIZE - 1 in rows)
            flat += [int(r) * spec.EMBEDDING_SIZE + int(rng.integers(spec.EMBEDDING_SIZE)) for r in rows]
        for idx in flat:
            base = w64[name].flat[idx]
            w64[name].flat[idx] = base + eps
            up = loss_at(w64)
            w64[name].flat[idx] = base - eps
            dn = loss_at(w64)
            w64[name].flat[idx] = base
            fd = (up - dn) / (2 * eps)
            # central differences in float64: truncation ~eps^2 |f'''|, rounding ~1e-16 / eps = 1e-11
            assert abs(fd - g.flat[idx]) <= 1e-8 + 1e-6 * abs(fd), (name, idx, fd, g.flat[idx])
    return grads


def test_rows_no_code_selects_have_zero_gradient(case):
    w, feats, labels, masks = case
    _, _, grads = tsb.step(w, feats, labels, masks, keep_prob=0.5)
    g = grads[tsb.EMBEDDING]
    hit = np.zeros(spec.VOCAB_SIZE, bool)
    hit[tsb.clamp_codes(feats["kmer"])] = True
    assert (g[~hit] == 0).all()
    assert (np.abs(g[hit]).max(axis=1) > 0).all()


def test_the_codes_of_each_kind():
    for kind in ("acgt", "one", "wide", "hostile"):
        k = tsb.codes(kind, 70, 5, 3)
        assert k.dtype == np.int32 and k.shape == (70, 5)
    assert (tsb.codes("one", 4, 5, 0) == 2).all()
    wide = tsb.codes("wide", 33, 17, 1)
    assert wide.min() == 0 and wide.max() == spec.VOCAB_SIZE - 1
    hostile = tsb.codes("hostile", 70, 5, 2)
    assert {-7, 1024, 2 ** 31 - 1} <= set(hostile.ravel().tolist())
    assert set(tsb.clamp_codes(hostile).ravel().tolist()) <= {0, 1, 2, 3, spec.VOCAB_SIZE - 1}
