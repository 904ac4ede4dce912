"""PyTorch-CPU statement of the RNN-only model's TRAINING graph (TEST INFRASTRUCTURE): the forward with dropout masks passed in,
the weighted cross entropy, gradients from autograd, and a numpy float64 Adam. Written from the reference's behaviour
(model.py:70-116, layers.py:45-72,247-264; denoise.py:97-110), independently of deepsignal_amd/csrc/ds_train.hip.

Masks: a dict stream -> 0/1 array with streams "fw_l0" .. "bw_l2" of shape [n, T, 256] (time index in the order the stack
PROCESSES the sequence: index 0 of a bw stream is the last base), "fc1" [n, 512], "fc2" [n, 2]; None = keep everything."""
from __future__ import annotations

from typing import Dict, Optional

import numpy as np
import torch

from deepsignal_amd import spec

STREAMS = ("fw_l0", "fw_l1", "fw_l2", "bw_l0", "bw_l1", "bw_l2", "fc1", "fc2")


def tensor_names():
    return [name for name, _ in spec.tensor_table(17, 360, 2, is_cnn=False, is_rnn=True, is_base=False)]


def no_masks(n: int, T: int) -> Dict[str, np.ndarray]:
    return {s: np.ones((n, T, spec.HIDDEN) if s[2] == "_" else (n, 512 if s == "fc1" else 2), np.uint8) for s in STREAMS}


def logits_of(w: Dict[str, torch.Tensor], feats: Dict[str, np.ndarray], masks: Dict[str, np.ndarray], keep_prob: float, dtype):
    """logits [n, 2] of the training forward; `w` holds torch tensors of `dtype` (leaves when gradients are wanted)."""
    x0 = torch.stack([torch.from_numpy(np.asarray(feats[k], np.float32)).to(dtype) for k in ("means", "stds", "sanums")], dim=2)
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
                ys.append(h / keep_prob * mask[:, t, :])          # DropoutWrapper(output_keep_prob): the recurrent h is not dropped
            seq = torch.stack(ys, dim=1)
        outs.append(seq[:, -1, :])
    joint = torch.cat(outs, dim=1)
    drop1 = (joint @ w["dense/kernel"]) / keep_prob * m["fc1"]
    return (drop1 @ w["dense_1/kernel"]) / keep_prob * m["fc2"]


def wce(x: torch.Tensor, z: torch.Tensor, pos_weight: float) -> torch.Tensor:
    """tf.nn.weighted_cross_entropy_with_logits, the stable form."""
    q = 1 + (pos_weight - 1) * z
    return (1 - z) * x + q * (torch.log1p(torch.exp(-torch.abs(x))) + torch.clamp(-x, min=0))


def wce_textbook(x: torch.Tensor, z: torch.Tensor, pos_weight: float) -> torch.Tensor:
    return -pos_weight * z * torch.log(torch.sigmoid(x)) - (1 - z) * torch.log(1 - torch.sigmoid(x))


def loss_of(logits: torch.Tensor, labels: np.ndarray, pos_weight: float) -> torch.Tensor:
    lab = torch.from_numpy(np.asarray(labels)).long()
    if pos_weight == 1.0:                                         # model.py:107-110
        onehot = torch.nn.functional.one_hot(lab, 2).to(logits.dtype)
        return wce(logits, onehot, 1.0).mean()
    return wce(logits[:, 1], lab.to(logits.dtype), pos_weight).mean()      # model.py:111-116


def pred_of(logits: np.ndarray, pos_weight: float) -> np.ndarray:
    if pos_weight == 1.0:
        return (logits[:, 1] > logits[:, 0]).astype(np.int32)    # argmax, ties -> 0
    return (logits[:, 1] > 0).astype(np.int32)                    # sigmoid(logits[:, 1]) > 0.5


def step(weights: Dict[str, np.ndarray], feats: Dict[str, np.ndarray], labels, masks: Optional[Dict[str, np.ndarray]] = None,
         keep_prob: float = 1.0, pos_weight: float = 1.0, dtype=torch.float64):
    """(loss, logits [n, 2], gradients by name) of one training forward / backward in `dtype`, all returned as float64."""
    n, T = np.asarray(feats["means"]).shape
    masks = no_masks(n, T) if masks is None else masks
    w = {k: torch.from_numpy(np.asarray(weights[k], np.float32)).to(dtype).requires_grad_(True) for k in tensor_names()}
    logits = logits_of(w, feats, masks, keep_prob, dtype)
    loss = loss_of(logits, labels, pos_weight)
    loss.backward()
    grads = {k: v.grad.to(torch.float64).numpy() for k, v in w.items()}
    return float(loss.detach().to(torch.float64)), logits.detach().to(torch.float64).numpy(), grads


class Adam:
    """tf.train.AdamOptimizer in numpy float64: lr_t = lr sqrt(1 - b2^t) / (1 - b1^t), epsilon outside the bias correction."""

    def __init__(self, params: Dict[str, np.ndarray], beta1: float = 0.9, beta2: float = 0.999, epsilon: float = 1e-8):
        self.p = {k: np.asarray(v, np.float64).copy() for k, v in params.items()}
        self.m = {k: np.zeros_like(v) for k, v in self.p.items()}
        self.v = {k: np.zeros_like(v) for k, v in self.p.items()}
        self.b1, self.b2, self.eps, self.t = beta1, beta2, epsilon, 0

    def update(self, grads: Dict[str, np.ndarray], lr: float) -> None:
        self.t += 1
        lr_t = lr * np.sqrt(1 - self.b2 ** self.t) / (1 - self.b1 ** self.t)
        for k, g in grads.items():
            g = np.asarray(g, np.float64)
            self.m[k] = self.b1 * self.m[k] + (1 - self.b1) * g
            self.v[k] = self.b2 * self.v[k] + (1 - self.b2) * g * g
            self.p[k] = self.p[k] - lr_t * self.m[k] / (np.sqrt(self.v[k]) + self.eps)


def train_features(n: int, T: int, seed: int) -> Dict[str, np.ndarray]:
    """Event features at the scale extract produces: normalised means, small stds, event lengths of a few samples."""
    rng = np.random.default_rng(seed)
    return {"means": rng.normal(0.0, 1.0, (n, T)).astype(np.float32),
            "stds": rng.uniform(0.05, 0.6, (n, T)).astype(np.float32),
            "sanums": rng.integers(3, 40, (n, T)).astype(np.float32)}


def rel_err(a: np.ndarray, ref: np.ndarray) -> float:
    """max |a - ref| / max |ref|"""
    return float(np.abs(np.asarray(a, np.float64) - ref).max() / max(np.abs(ref).max(), 1e-300))
