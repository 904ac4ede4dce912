"""CPU statement of DS_PRECISION_FP16X2 (TEST INFRASTRUCTURE; the contract is in include/deepsignal_hip.h).

An fp32 operand x is carried as two fp16 terms
    h0 = fp16(x), h1 = fp16(x - h0)        round to nearest even, subnormal terms kept, no saturation; the difference in fp32
and a product a * b is the fp32-accumulated sum of a1 b0, a0 b1, a0 b0 in that order (small first) -- exactly
oracle/torch_statement.py::forward_split with terms=2 (`reversed(split_pairs(2))`), except for the number format of the terms.
So `forward_fp16x2` RUNS forward_split(terms=2) with torch_statement.split_terms swapped for the fp16 split below, inside a context
manager that puts the bf16 split back (oracle/ stays as it is; nothing else of that module is touched). Everything between the
matrix products is fp32 there as in the engine, and the scope is DS_PRECISION_BF16X3's.

A value beyond +-65504 becomes Inf in h0 and -Inf in h1; Inf * w - Inf * w is NaN, so the site comes out NaN, as in the engine.
`flush=True` is the arm of tools/split_emulation.py that flushes every term below 2^-14 to zero (an MFMA that drops fp16 subnormal
inputs): NOT the contract, kept to measure what rests on the subnormals.
"""
from __future__ import annotations

import contextlib

import torch

from oracle import torch_statement

FP16X2_SCOPE = ("modules", "stem23", "lstm", "fc1")
FP16_MAX = 65504.0
FP16_MIN_NORMAL = 2.0 ** -14


def split_terms_fp16(x: torch.Tensor, terms: int = 2, flush: bool = False):
    """The fp16 terms of an fp32 tensor, each returned as float32 (values exactly representable in fp16)."""
    x = x.to(torch.float32)
    out, r = [], x
    for _ in range(terms):
        t = r.to(torch.float16).to(torch.float32)           # round to nearest even; > 65504 + half an ulp: Inf; subnormals kept
        if flush:
            t = torch.where(t.abs() < FP16_MIN_NORMAL, torch.zeros_like(t), t)
        out.append(t)
        r = r - t                                           # exact in fp32 while t is finite; Inf - Inf = NaN never reaches a product: h1 = -Inf does
    return out


@contextlib.contextmanager
def fp16_terms(flush: bool = False):
    """torch_statement.split_terms = the fp16 split while the block runs; the bf16 split is back afterwards, also on an exception."""
    saved = torch_statement.split_terms
    torch_statement.split_terms = lambda x, terms: split_terms_fp16(x, terms, flush)
    try:
        yield
    finally:
        torch_statement.split_terms = saved


def forward_fp16x2(weights, feats, scope=FP16X2_SCOPE, return_taps: bool = False, acc_dtype=torch.float32, flush: bool = False,
                   is_cnn: bool = True, is_rnn: bool = True, is_base: bool = True):
    """act, pred[, taps] of the fp16x2 arithmetic: torch_statement.forward_split(terms=2) on fp16 terms (see the module docstring).
    The model variants (model.py:28-29,59-75,89-95: no signal model, no event model, no k-mer embedding), which forward_split does not
    take, go through `_forward_variant` below: the same arithmetic from the same helpers."""
    with fp16_terms(flush):
        if is_cnn and is_rnn and is_base:
            return torch_statement.forward_split(weights, feats, terms=2, scope=tuple(scope), acc_dtype=acc_dtype, return_taps=return_taps)
        return _forward_variant(weights, feats, tuple(scope), acc_dtype, return_taps, is_cnn, is_rnn, is_base)


def _forward_variant(weights, feats, scope, acc_dtype, return_taps, is_cnn, is_rnn, is_base):
    """forward_split(terms=2) with the is_cnn / is_rnn / is_base switches of torch_statement.forward. Runs inside fp16_terms()."""
    import numpy as np
    import torch.nn.functional as F
    from deepsignal_amd import spec
    ts, f32 = torch_statement, torch.float32
    w = {k: torch.from_numpy(np.asarray(v)).to(f32) for k, v in weights.items()}
    kmer = torch.from_numpy(feats["kmer"]).long()
    n, T = kmer.shape
    d = spec.net_dims(T, feats["signals"].shape[1], w["dense_1/kernel"].shape[1], is_cnn, is_rnn)
    taps, parts = {}, []
    mm = lambda a, b, split: ts._split_matmul(a, b, 2, acc_dtype) if split else (a.to(acc_dtype) @ b.to(acc_dtype)).to(f32)

    def conv(x, c, split):
        kf, bf = ts._fold(w, c)
        if split:
            return ts._split_conv(x, kf, bf, c, 2, acc_dtype)
        kt = kf.to(acc_dtype).permute(2, 1, 0).contiguous()
        return (F.conv1d(ts._same(x.to(acc_dtype), c.k, c.stride), kt, stride=c.stride) + bf.to(acc_dtype)[None, :, None]).to(f32)

    if is_rnn:
        extra = [torch.from_numpy(feats[k]).to(f32)[:, :, None] for k in ("means", "stds", "sanums")]
        x0 = torch.cat(([w[spec.MODEL_PREFIX + "embedding"][kmer]] if is_base else []) + extra, dim=2)
        for direction in ("fw", "bw"):
            seq = x0 if direction == "fw" else torch.flip(x0, dims=[1])
            for layer in range(spec.LSTM_LAYERS):
                K = w[spec.lstm_tensor(direction, layer, "kernel")]
                b = w[spec.lstm_tensor(direction, layer, "bias")]
                nin = K.shape[0] - spec.HIDDEN
                h = torch.zeros(n, spec.HIDDEN, dtype=f32)
                c = torch.zeros(n, spec.HIDDEN, dtype=f32)
                hs = []
                for t in range(T):
                    # layer 0's input projection is full precision (a table row plus rank-1 terms in the engine), as in forward_split
                    z = mm(seq[:, t, :], K[:nin], "lstm" in scope and layer > 0) + mm(h, K[nin:], "lstm" in scope) + b
                    i, j, f, o = torch.split(z, spec.HIDDEN, dim=1)
                    c = torch.sigmoid(f + spec.FORGET_BIAS) * c + torch.sigmoid(i) * torch.tanh(j)
                    h = torch.sigmoid(o) * torch.tanh(c)
                    hs.append(h)
                seq = torch.stack(hs, dim=1)
                taps["lstm_%s_l%d" % (direction, layer)] = seq if direction == "fw" else torch.flip(seq, dims=[1])
            parts.append(seq[:, -1, :])
    if is_cnn:
        x = torch.from_numpy(feats["signals"]).to(f32)[:, None, :]
        stem = spec.stem_convs()
        x = ts._maxpool3(torch.relu(conv(x, stem[0], False)), 2); taps["stem_pool"] = x
        x = torch.relu(conv(x, stem[1], "stem23" in scope)); taps["stem_conv2"] = x
        x = torch.relu(conv(x, stem[2], "stem23" in scope)); taps["stem_conv3"] = x
        sm = "modules" in scope
        for mth in range(1, spec.N_INCEPTION + 1):
            c = spec.inception_convs(mth, d.module_cin(mth))
            b1 = torch.relu(conv(ts._maxpool3(x, 1), c["b1"], sm))
            b2 = torch.relu(conv(x, c["b2"], sm))
            b3 = torch.relu(conv(torch.relu(conv(x, c["b3a"], sm)), c["b3b"], sm))
            b4 = torch.relu(conv(torch.relu(conv(x, c["b4a"], sm)), c["b4b"], sm))
            r = conv(torch.relu(conv(torch.relu(conv(x, c["b5a"], sm)), c["b5b"], sm)), c["b5c"], sm)
            b5 = torch.relu(conv(x, c["b5s"], sm) + r)
            x = torch.cat([b1, b2, b3, b4, b5], dim=1)
            taps["module%d" % mth] = x
            if mth in (3, 8):
                x = ts._maxpool3(x, 2)
        x = F.avg_pool1d(x, 7, stride=1, padding=3, count_include_pad=False)
        parts.append(x.permute(0, 2, 1).reshape(n, -1))
        taps["signal_feat"] = parts[-1]
    joint = torch.cat(parts, dim=1)
    fc1 = mm(joint, w["dense/kernel"], "fc1" in scope)
    logits = mm(fc1, w["dense_1/kernel"], False)
    act = torch.sigmoid(logits)
    pred = torch.argmax(act, dim=1)
    taps.update(joint=joint, fc1=fc1, logits=logits)
    if return_taps:
        out = {}
        for k, v in taps.items():
            v = v.permute(0, 2, 1) if (k.startswith("stem") or k.startswith("module")) else v
            out[k] = v.contiguous().to(torch.float32).numpy()
        return act.numpy(), pred.to(torch.int32).numpy(), out
    return act.numpy(), pred.to(torch.int32).numpy()
