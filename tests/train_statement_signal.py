"""PyTorch-CPU statement of the signal-only model's TRAINING graph (`--is_cnn yes --is_rnn no`; TEST INFRASTRUCTURE): the stem, the
eleven inception modules, the 1x7 average pool and the joint layers (model.py:89-95, layers.py:80-139,176-264 restated), generic in
dtype. Dropout masks are passed in, gradients come from autograd, loss and prediction rule are tests/train_statement.py's.

Batch normalisation in training mode: per channel the mean m and the biased variance v (mean squared deviation from m) over the
batch's n x W values, y = gamma (x - m) / sqrt(v + 1e-3) + beta. With training=False the moving statistics of `weights` stand in.

DECISIONS. The graph is piecewise smooth: every ReLU and every max pool chooses. Two float32 evaluations that differ only in their
summation order choose differently in a handful of places out of millions, and one flipped pool index moves most gradients by
1e-3 - 1e-2 of their scale, far above float32's own 1e-5. So `dec` may fix the choices: one boolean mask per ReLU (ReLU becomes
z x mask) and one window index per max-pool output (the pool becomes a gather). A free run (dec=None) makes its own choices the same
way -- the mask is z > 0, the index the first maximum of the window, which is what TensorFlow's and torch's max-pool gradients pick --
and returns them, so a run constrained to its own decisions repeats the free run bit for bit."""
from __future__ import annotations

from typing import Dict, Optional, Tuple

import numpy as np
import torch
import torch.nn.functional as F

import train_statement as ts
from deepsignal_amd import spec

loss_of, pred_of, rel_err = ts.loss_of, ts.pred_of, ts.rel_err
BRANCH_OUT = ("b1", "b2", "b3b", "b4b", "b5")        # a module's output channels, in order (layers.py:139)


def tensor_names(signal_len: int = 360):
    return [name for name, _ in spec.tensor_table(17, signal_len, 2, is_cnn=True, is_rnn=False)]


def trainable_names(signal_len: int = 360):
    return [k for k in tensor_names(signal_len) if not k.endswith(("/moving_mean", "/moving_variance"))]


def dims(signal_len: int) -> spec.NetDims:
    return spec.net_dims(17, signal_len, 2, True, False)


def no_masks(n: int, signal_len: int) -> Dict[str, np.ndarray]:
    return {"fc1": np.ones((n, dims(signal_len).joint), np.uint8), "fc2": np.ones((n, 2), np.uint8)}


def windows(x: torch.Tensor, stride: int) -> torch.Tensor:
    """[n, C, W] -> the 1x3 SAME windows [n, C, W_out, 3], pads -inf (a pad never wins)."""
    _, left, right = spec.same_pad(x.shape[-1], 3, stride)
    return F.pad(x, (left, right), value=float("-inf")).unfold(2, 3, stride)


def first_argmax(win: torch.Tensor) -> torch.Tensor:
    eq = win == win.max(-1, keepdim=True).values
    return torch.where(eq[..., 0], 0, torch.where(eq[..., 1], 1, 2))


class Run:
    """What one forward leaves behind: the decisions taken (`relu`, `pool`), the values they were taken on (`z`, `win`), the layer
    outputs by tap name as [n, W, C] (`taps`) and each conv's batch statistics (`stats`: name -> (mean, biased variance))."""

    def __init__(self, dec, training):
        self.dec, self.training = dec, training
        self.relu, self.pool, self.z, self.win, self.taps, self.stats = {}, {}, {}, {}, {}, {}

    def do_relu(self, name: str, z: torch.Tensor) -> torch.Tensor:
        mask = (z.detach() > 0) if self.dec is None else self.dec[0][name]
        self.relu[name], self.z[name] = mask, z.detach()
        y = z * mask.to(z.dtype)
        self.taps[name] = y.detach().permute(0, 2, 1)
        return y

    def do_pool(self, name: str, x: torch.Tensor, stride: int) -> torch.Tensor:
        win = windows(x, stride)
        idx = first_argmax(win.detach()) if self.dec is None else self.dec[1][name]
        self.pool[name], self.win[name] = idx, win.detach()
        return win.gather(-1, idx[..., None])[..., 0]


def conv(x: torch.Tensor, ker: torch.Tensor, c: spec.ConvBN) -> torch.Tensor:
    _, left, right = spec.same_pad(x.shape[-1], c.k, c.stride)
    return F.conv1d(F.pad(x, (left, right)), ker[0].permute(2, 1, 0).contiguous(), stride=c.stride)


def conv_bn(x, w, c: spec.ConvBN, run: Run, name: str):
    y = conv(x, w[c.kernel_name], c)
    g, b = w[c.bn_tensor("gamma")], w[c.bn_tensor("beta")]
    if run.training:
        m = y.mean(dim=(0, 2))
        v = ((y - m[None, :, None]) ** 2).mean(dim=(0, 2))
        run.stats[name] = (m.detach(), v.detach())
    else:
        m, v = w[c.bn_tensor("moving_mean")], w[c.bn_tensor("moving_variance")]
    y = (y - m[None, :, None]) * (g / torch.sqrt(v + spec.BN_EPS))[None, :, None] + b[None, :, None]
    if c.relu:
        return run.do_relu(name, y)
    run.taps[name] = y.detach().permute(0, 2, 1)
    return y


def inception(x, w, k: int, cin: int, run: Run):
    c = spec.inception_convs(k, cin)
    t = lambda key: "m%d.%s" % (k, key)
    b1 = conv_bn(run.do_pool(t("pool"), x, 1), w, c["b1"], run, t("b1"))
    b2 = conv_bn(x, w, c["b2"], run, t("b2"))
    b3 = conv_bn(conv_bn(x, w, c["b3a"], run, t("b3a")), w, c["b3b"], run, t("b3b"))
    b4 = conv_bn(conv_bn(x, w, c["b4a"], run, t("b4a")), w, c["b4b"], run, t("b4b"))
    stem = conv_bn(x, w, c["b5s"], run, t("b5s"))
    r = conv_bn(conv_bn(conv_bn(x, w, c["b5a"], run, t("b5a")), w, c["b5b"], run, t("b5b")), w, c["b5c"], run, t("b5c"))
    return torch.cat([b1, b2, b3, b4, run.do_relu(t("b5"), stem + r)], dim=1)


def logits_of(w, signals, masks, keep_prob: float, dtype, dec=None, training: bool = True) -> Tuple[torch.Tensor, Run]:
    run = Run(dec, training)
    x = torch.from_numpy(np.asarray(signals, np.float32)).to(dtype)[:, None, :]
    n, d = x.shape[0], dims(x.shape[-1])
    st = spec.stem_convs()
    x = run.do_pool("pool1", conv_bn(x, w, st[0], run, "stem1"), 2)
    x = conv_bn(x, w, st[1], run, "stem2")
    x = conv_bn(x, w, st[2], run, "stem3")
    for k in range(1, spec.N_INCEPTION + 1):
        x = inception(x, w, k, d.module_cin(k), run)
        if k in (3, 8):
            x = run.do_pool("pool%d" % (2 if k == 3 else 3), x, 2)
    x = F.avg_pool1d(x, 7, stride=1, padding=3, count_include_pad=False)
    feat = x.permute(0, 2, 1).reshape(n, -1)
    m = {k: torch.from_numpy(np.asarray(v)).to(dtype) for k, v in masks.items()}
    drop1 = (feat @ w["dense/kernel"]) / keep_prob * m["fc1"]
    logits = (drop1 @ w["dense_1/kernel"]) / keep_prob * m["fc2"]
    run.taps["feat"], run.taps["logits"] = feat.detach(), logits.detach()
    return logits, run


def step(weights: Dict[str, np.ndarray], signals, labels, masks: Optional[Dict[str, np.ndarray]] = None, keep_prob: float = 1.0,
         pos_weight: float = 1.0, dtype=torch.float64, dec=None, exact: bool = False, training: bool = True, grad: bool = True):
    """(loss, logits [n, 2], gradients of the 341 trained tensors by name, the Run) of one forward / backward in `dtype`; loss,
    logits and gradients returned as float64. `weights` are taken through float32 first, as the engine holds them; exact=True takes
    float64 weights as they are. training=False: the evaluation forward on the moving statistics (pass no masks, keep_prob 1)."""
    signals = np.asarray(signals, np.float32)
    S = signals.shape[1]
    masks = no_masks(signals.shape[0], S) if masks is None else masks
    cast = (lambda a: np.asarray(a, np.float64)) if exact else (lambda a: np.asarray(a, np.float32))
    names = trainable_names(S)
    w = {k: torch.from_numpy(cast(weights[k])).to(dtype) for k in tensor_names(S)}
    if grad:
        for k in names:
            w[k].requires_grad_(True)
    with torch.set_grad_enabled(grad):
        logits, run = logits_of(w, signals, masks, keep_prob, dtype, dec, training)
        loss = loss_of(logits, labels, pos_weight)
    grads = {}
    if grad:
        loss.backward()
        grads = {k: w[k].grad.to(torch.float64).numpy() for k in names}
    return float(loss.detach().to(torch.float64)), logits.detach().to(torch.float64).numpy(), grads, run


# ---- decisions from a set of taps [n, W, C] (the GPU's, or a Run's own): y > 0 per ReLU, first maximum per pool window ------------
def module_out(taps: Dict[str, np.ndarray], k: int) -> torch.Tensor:
    return torch.cat([torch.from_numpy(np.asarray(taps["m%d.%s" % (k, b)])) for b in BRANCH_OUT], dim=2)


def decisions_from_taps(taps: Dict[str, np.ndarray]):
    relu = {name: torch.from_numpy(np.asarray(t)).permute(0, 2, 1) > 0 for name, t in taps.items()
            if name not in ("feat", "logits") and not name.endswith((".b5s", ".b5c"))}
    pool = {}

    def choose(name, x_nwc, stride):        # the pool's output, from exact comparisons of the taps' own values
        win = windows(x_nwc.permute(0, 2, 1), stride)
        pool[name] = first_argmax(win)
        return win.max(-1).values.permute(0, 2, 1)

    x = choose("pool1", torch.from_numpy(np.asarray(taps["stem1"])), 2)
    x = torch.from_numpy(np.asarray(taps["stem3"]))
    for k in range(1, spec.N_INCEPTION + 1):
        choose("m%d.pool" % k, x, 1)
        x = module_out(taps, k)
        if k in (3, 8):
            x = choose("pool%d" % (2 if k == 3 else 3), x, 2)
    return relu, pool


def decision_differences(dec, free: Run):
    """Where `dec` differs from the free run's own decisions: [(name, places, largest margin in the free run's values, tap)]. The
    margin of a ReLU is |z| and its tap the ReLU's own; the margin of a pool is the gap between the two candidates, reported per tap
    that feeds the differing channels (`pool_feeders`), so that each place is held to the bar of the tap its values come from."""
    out = []
    for name, mask in dec[0].items():
        diff = mask != free.relu[name]
        if diff.any():
            out.append((name, int(diff.sum()), float(free.z[name][diff].abs().max()), name))
    for name, idx in dec[1].items():
        diff = idx != free.pool[name]
        if diff.any():
            win = free.win[name]
            gap = (win.gather(-1, free.pool[name][..., None]) - win.gather(-1, idx[..., None]))[..., 0].abs()
            for tap, c0, c1 in pool_feeders(name):
                d = diff[:, c0:c1]
                if d.any():
                    out.append((name, int(d.sum()), float(gap[:, c0:c1][d].max()), tap))
    return out


def pool_feeders(name: str):
    """(tap, first channel, end channel) of the taps whose values a pool compares, in the pool's channel order [n, C, W]."""
    if name == "pool1":
        return [("stem1", 0, 64)]
    k = (4 if name == "pool2" else 9) if name.startswith("pool") else int(name[1:].split(".")[0])      # the module the pool feeds
    if k == 1:
        return [("stem3", 0, 256)]
    return [("m%d.%s" % (k - 1, b), 48 * i, 48 * (i + 1)) for i, b in enumerate(BRANCH_OUT)]


# ---- moving statistics: the rule of csrc/ds_train_signal.h (moving_update), in float64 ----------------------------------------------
def moving_after(weights: Dict[str, np.ndarray], runs, decay: float = 0.9) -> Dict[str, np.ndarray]:
    """The moving statistics after training steps whose forwards are `runs` (a list of Run, one per step, in order), from `weights`'
    own and a zero-debias helper that starts at 0: moving_variance <- decay mv + (1 - decay) v N / max(N - 1, 1) (the fused batch
    norm's unbiased variance), biased_k = decay biased_{k-1} + (1 - decay) m, moving_mean = biased_k / (1 - decay^k)."""
    out = {k: np.asarray(v, np.float64).copy() for k, v in weights.items() if k.endswith(("/moving_mean", "/moving_variance"))}
    biased = {bn: np.zeros_like(out[bn + "/moving_mean"]) for bn in bn_scopes()}
    for k, run in enumerate(runs, start=1):
        for bn, tap in bn_scopes().items():
            m, v = (t.to(torch.float64).numpy() for t in run.stats[tap])
            N = run.taps[tap].shape[0] * run.taps[tap].shape[1]
            biased[bn] = decay * biased[bn] + (1 - decay) * m
            out[bn + "/moving_mean"] = biased[bn] / (1 - decay ** k)
            out[bn + "/moving_variance"] = decay * out[bn + "/moving_variance"] + (1 - decay) * v * N / max(N - 1, 1)
    return out


def bn_scopes() -> Dict[str, str]:
    """'<scope>/<bn_name>' of every conv -> its tap name."""
    out = {}
    for i, c in enumerate(spec.stem_convs()):
        out["%s/%s" % (c.scope, c.bn_name)] = "stem%d" % (i + 1)
    for k in range(1, spec.N_INCEPTION + 1):
        for key, c in spec.inception_convs(k, 256 if k == 1 else spec.INCEPTION_OUT).items():
            out["%s/%s" % (c.scope, c.bn_name)] = "m%d.%s" % (k, key)
    return out
