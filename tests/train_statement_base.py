"""PyTorch-CPU statement of the RNN-only model's TRAINING graph WITH the embedding (`--is_base yes`; TEST INFRASTRUCTURE):
tests/train_statement.py with the embedding lookup in front (model.py:61-69: layer 0 reads [embedding row of the base's code (128) |
mean, std, length]) and `modelembedding` among the trained tensors. Loss, prediction rule and Adam are train_statement's own.

Codes follow the forward's contract (include/deepsignal_hip.h, "CODES"): below 0 acts as 0, above 1023 as 1023. autograd's
gradient of an index lookup is dense: the rows of the table that no code selects get exactly 0, and the dense Adam of
train_statement then moves every row's moments -- what TF's sparse Adam update does to an embedding_lookup gradient too."""
from __future__ import annotations

from typing import Dict, Optional

import numpy as np
import torch

import train_statement as ts
from deepsignal_amd import spec

wce, loss_of, pred_of, Adam, no_masks, rel_err, STREAMS = ts.wce, ts.loss_of, ts.pred_of, ts.Adam, ts.no_masks, ts.rel_err, ts.STREAMS
EMBEDDING = spec.MODEL_PREFIX + "embedding"


def tensor_names():
    return [name for name, _ in spec.tensor_table(17, 360, 2, is_cnn=False, is_rnn=True, is_base=True)]


def clamp_codes(kmer) -> np.ndarray:
    return np.clip(np.asarray(kmer, np.int64), 0, spec.VOCAB_SIZE - 1)


def logits_of(w: Dict[str, torch.Tensor], feats: Dict[str, np.ndarray], masks: Dict[str, np.ndarray], keep_prob: float, dtype):
    """logits [n, 2] of the training forward; feats holds "kmer" int [n, T] beside means / stds / sanums."""
    x3 = torch.stack([torch.from_numpy(np.asarray(feats[k], np.float32)).to(dtype) for k in ("means", "stds", "sanums")], dim=2)
    x0 = torch.cat([w[EMBEDDING][torch.from_numpy(clamp_codes(feats["kmer"]))], x3], dim=2)          # [n, T, 131]
    n, T, _ = x0.shape
    m = {k: torch.from_numpy(np.asarray(v)).to(dtype) for k, v in masks.items()}
    outs = []
    for direction in ("fw", "bw"):
        seq = x0 if direction == "fw" else torch.flip(x0, dims=[1])
        for layer in range(spec.LSTM_LAYERS):
            K = w[spec.lstm_tensor(direction, layer, "kernel")]
            b = w[spec.lstm_tensor(direction, layer, "bias")]
            mask = m["%s_l%d" % (direction, layer)]
            h = torch.zeros(n, spec.HIDDEN, dtype=dtype)
            c = torch.zeros(n, spec.HIDDEN, dtype=dtype)
            ys = []
            for t in range(T):
                z = torch.cat([seq[:, t, :], h], dim=1) @ K + b
                i, j, f, o = torch.split(z, spec.HIDDEN, dim=1)
                c = torch.sigmoid(f + spec.FORGET_BIAS) * c + torch.sigmoid(i) * torch.tanh(j)
                h = torch.sigmoid(o) * torch.tanh(c)
                ys.append(h / keep_prob * mask[:, t, :])
            seq = torch.stack(ys, dim=1)
        outs.append(seq[:, -1, :])
    joint = torch.cat(outs, dim=1)
    drop1 = (joint @ w["dense/kernel"]) / keep_prob * m["fc1"]
    return (drop1 @ w["dense_1/kernel"]) / keep_prob * m["fc2"]


def step(weights: Dict[str, np.ndarray], feats: Dict[str, np.ndarray], labels, masks: Optional[Dict[str, np.ndarray]] = None,
         keep_prob: float = 1.0, pos_weight: float = 1.0, dtype=torch.float64, exact: bool = False):
    """(loss, logits [n, 2], gradients by name) of one training forward / backward in `dtype`, all returned as float64.
    `weights` are taken through float32 first, as the engine holds them; exact=True takes float64 weights as they are."""
    n, T = np.asarray(feats["means"]).shape
    masks = no_masks(n, T) if masks is None else masks
    cast = (lambda a: np.asarray(a, np.float64)) if exact else (lambda a: np.asarray(a, np.float32))
    w = {k: torch.from_numpy(cast(weights[k])).to(dtype).requires_grad_(True) for k in tensor_names()}
    logits = logits_of(w, feats, masks, keep_prob, dtype)
    loss = loss_of(logits, labels, pos_weight)
    loss.backward()
    grads = {k: v.grad.to(torch.float64).numpy() for k, v in w.items()}
    return float(loss.detach().to(torch.float64)), logits.detach().to(torch.float64).numpy(), grads


def codes(kind: str, n: int, T: int, seed: int) -> np.ndarray:
    """int32 [n, T]: "acgt" uniform over 0 .. 3; "one" every code 2; "wide" uniform over 0 .. 1023 with 0 and 1023 forced in;
    "hostile" "acgt" with some codes set to -7, 1024 and 2^31 - 1 (they act as 0, 1023 and 1023)."""
    rng = np.random.default_rng(seed)
    if kind == "one":
        return np.full((n, T), 2, np.int32)
    if kind == "wide":
        k = rng.integers(0, spec.VOCAB_SIZE, (n, T)).astype(np.int32)
        k.flat[0], k.flat[-1] = 0, spec.VOCAB_SIZE - 1
        return k
    k = rng.integers(0, 4, (n, T)).astype(np.int32)
    if kind == "hostile":
        flat = k.reshape(-1)
        where = rng.permutation(flat.size)[:max(3, flat.size // 10)]
        flat[where] = np.resize(np.array([-7, 1024, 2 ** 31 - 1], np.int32), where.size)
    elif kind != "acgt":
        raise ValueError(kind)
    return k


def train_features(n: int, T: int, seed: int, kind: str = "acgt") -> Dict[str, np.ndarray]:
    feats = ts.train_features(n, T, seed)
    feats["kmer"] = codes(kind, n, T, seed + 17)
    return feats
