"""CPU: tests/train_statement.py (the oracle of the GPU training step) held to first principles: its autograd gradients against
central differences, its stable loss against the textbook form, its Adam against the closed form of the first update."""
import numpy as np
import pytest
import torch

import train_statement as ts
from deepsignal_amd import spec, weights


@pytest.fixture(scope="module")
def case():
    n, T = 4, 3
    w = weights.random_weights(seed=7, is_cnn=False, is_base=False, kmer_len=T, lstm_bias_std=0.1)
    feats = ts.train_features(n, T, seed=11)
    labels = np.array([0, 1, 1, 0], np.int32)
    rng = np.random.default_rng(5)
    masks = {s: (rng.random(m.shape) < 0.5).astype(np.uint8) for s, m in ts.no_masks(n, T).items()}
    return w, feats, labels, masks


@pytest.mark.parametrize("pos_weight", [1.0, 3.0])
def test_autograd_matches_central_differences(case, pos_weight):
    _central_differences(case, pos_weight)


def _case_at(n, T):
    w = weights.random_weights(seed=7, is_cnn=False, is_base=False, kmer_len=T, lstm_bias_std=0.1)
    feats = ts.train_features(n, T, seed=11)
    labels = (np.arange(n) % 2).astype(np.int32)
    rng = np.random.default_rng(5)
    masks = {s: (rng.random(m.shape) < 0.5).astype(np.uint8) for s, m in ts.no_masks(n, T).items()}
    return w, feats, labels, masks


@pytest.mark.parametrize("pos_weight", [1.0, 3.0])
@pytest.mark.parametrize("T", [1, 3])
def test_autograd_matches_central_differences_at_the_ends_of_kmer_len(T, pos_weight):
    """T = 1: no cell has a recurrent operand, so the rows [in:] of every LSTM kernel have a gradient of exactly zero (and the
    central difference is zero too: the loss does not depend on them). T = 3 = the number of layers. tests/test_gpu_train_kmer_ends.py
    holds the GPU step to the statement at these lengths."""
    case = _case_at(5, T)
    grads = _central_differences(case, pos_weight)
    for direction in ("fw", "bw"):
        for layer in range(spec.LSTM_LAYERS):
            g = grads[spec.lstm_tensor(direction, layer, "kernel")]
            rec = g[g.shape[0] - spec.HIDDEN:]
            assert np.abs(g[:g.shape[0] - spec.HIDDEN]).max() > 0
            assert (rec == 0).all() if T == 1 else np.abs(rec).max() > 0


def _central_differences(case, pos_weight):
    w, feats, labels, masks = case
    _, _, grads = ts.step(w, feats, labels, masks, keep_prob=0.5, pos_weight=pos_weight)
    rng = np.random.default_rng(1)

    def loss_at(w64):
        wt = {k: torch.from_numpy(v) for k, v in w64.items()}
        return float(ts.loss_of(ts.logits_of(wt, feats, masks, 0.5, torch.float64), labels, pos_weight))

    w64 = {k: np.asarray(w[k], np.float64).copy() for k in ts.tensor_names()}
    eps = 1e-5
    for name in ts.tensor_names():
        g = grads[name]
        # the coordinates that matter most (largest gradient) and a few at random
        flat = list(np.argsort(np.abs(g).ravel())[-2:]) + list(rng.integers(0, g.size, 2))
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


@pytest.mark.parametrize("pos_weight", [1.0, 3.0])
def test_stable_loss_equals_textbook_form(pos_weight):
    x = torch.linspace(-12, 12, 97, dtype=torch.float64)
    for z in (0.0, 1.0):
        zt = torch.full_like(x, z)
        assert torch.allclose(ts.wce(x, zt, pos_weight), ts.wce_textbook(x, zt, pos_weight), rtol=1e-12, atol=1e-12)
    # both loss branches reduce as the model does: n x 2 terms against the one-hot labels, or n terms on column 1
    logits = torch.tensor([[0.3, -0.2], [1.5, 0.4], [-0.7, 0.9]], dtype=torch.float64)
    labels = np.array([1, 0, 1])
    got = float(ts.loss_of(logits, labels, pos_weight))
    if pos_weight == 1.0:
        onehot = torch.tensor([[0., 1.], [1., 0.], [0., 1.]], dtype=torch.float64)
        want = float(ts.wce_textbook(logits, onehot, 1.0).sum() / 6)
    else:
        want = float(ts.wce_textbook(logits[:, 1], torch.tensor([1., 0., 1.], dtype=torch.float64), pos_weight).sum() / 3)
    assert abs(got - want) <= 1e-14


def test_adam_first_step_is_lr_times_sign():
    p = {"a": np.array([1.0, -2.0, 3.0, 0.5])}
    g = {"a": np.array([0.3, -4.0, 1e-3, 0.0])}
    opt = ts.Adam(p)
    opt.update(g, lr=1e-3)
    # t = 1: m = 0.1 g, v = 0.001 g^2, lr_t = lr sqrt(0.001) / 0.1 -> update = lr g / (|g| + eps sqrt(1000) ... ) ~ lr sign(g)
    lr_t = 1e-3 * np.sqrt(1 - 0.999) / (1 - 0.9)
    want = p["a"] - lr_t * (0.1 * g["a"]) / (np.sqrt(0.001 * g["a"] ** 2) + 1e-8)
    assert np.allclose(opt.p["a"], want, rtol=0, atol=1e-18)
    assert np.allclose(opt.p["a"][:3], p["a"][:3] - 1e-3 * np.sign(g["a"][:3]), rtol=0, atol=1e-3 * 1e-3)
    assert opt.p["a"][3] == p["a"][3]
    # a second step keeps the moments
    opt.update(g, lr=1e-3)
    assert np.allclose(opt.m["a"], (1 - 0.9 ** 2) * g["a"]) and np.allclose(opt.v["a"], (1 - 0.999 ** 2) * g["a"] ** 2)
