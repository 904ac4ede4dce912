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
            assert 0 in rows and spec.VOCAB_SIZE - 1 in rows
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
