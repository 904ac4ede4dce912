"""GPU: one training step of the signal-only model (ds_train_begin_signal / ds_train_step_signal, lr = 0) against
tests/train_statement_signal.py.

Per case: (1) both dropout streams bit for bit against the CPU checker; (2) every tap against the FREE float64 statement,
max|d| / max|tap_64| <= 4 x max(the free float32 statement's distance on that tap, 1e-6); (3) the decisions derived from the GPU's
taps (y > 0, first maximum over the taps that feed each pool) differ from the float64 statement's own in at most 16 places, each with
a float64 margin (|z|, or the gap between the two candidates) no larger than that tap's forward bar times its scale (for a pool: the
tap that feeds the differing channel); (4) the gradients
of all 341 trained tensors against the float64 statement UNDER THE GPU'S DECISIONS, e = max|g - g_64| / max|g_64| <=
4 x max(e_32, 1e-6) with e_32 the float32 statement's distance under the same decisions (the bar of test_gpu_train_grad.py);
(5) the loss, which is 1-Lipschitz in the logits (pos_weight-Lipschitz in the second branch):
|loss - loss_64| <= max(1, pos_weight) x 4 x max(max|logits_32 - logits_64|, 2^-22 max|logits_64|), loss and logits of both
statements taken under the GPU's decisions as in (4); (6) the prediction wherever the float64 logit gap exceeds that bar; (7) with
lr = 0 not a bit of a parameter moves.

On one MI355X the taps stood at 0.41 - 0.50 of their bars, the gradients at 0.57 - 0.77 of theirs, the loss at 0.003 - 0.06 of its
bar, with 0 / 0 / 1 / 1 / 3 / 12 differing decisions (offset, real window, one row, dead, odd widths, partial tiles). "wide slabs"
and "even slabs" there: the taps at 0.25 / 0.29 of their bars, the gradients at 0.33 / 0.42 of theirs, the loss at 0.0009 / 0.003
of its bar, with 40 / 29 differing decisions against places_32 = 77 / 66 (caps 154 / 132; on another host's torch build the same
float32 statement gave places_32 = 70 / 73). With colsum_kernel made to add 128 rows of every slab whatever slab_rows is, the six
cases above passed unchanged and both wide cases failed at their first tap, stem1, 0.48 / 0.42 from the float64 statement against
a bar of 4e-6.

WIDE ROW SLABS. Every reduction over the R = n x W rows of a layer (batch-norm sums, their gradient sums, every weight gradient) is
cut into slabs of rows by slabs_of (ds_train_signal.hip; NSLAB in ds_train_signal.h), restated here as `slabs_of`. The six cases
above stay at 128 rows a slab; "wide slabs" and "even slabs" run the stem and modules 1 - 3 at longer slabs, all 64 of them (the
table at WIDE_SLABS, asserted from the rule). Their graphs take 4.4e7 / 4.1e7 decisions, where the free float32 statement alone
differs from the float64 one in `places_32` places, so their cap on differing places is max(16, 2 x places_32) -- another summation
order flips another set of about that size; every differing place is still held to its margin.

Handles have max_batch = 96 (1024 for the two wide cases). randomize_bn weights throughout, so gamma and beta matter."""
import functools
import os
import re

import numpy as np
import pytest
import torch

import train_statement_signal as tss

pytestmark = pytest.mark.gpu

MAX_BATCH = 96
MAX_BATCH_WIDE = 1024
SEED = 99
MAX_DIFFERING = 16
#         kind             signal_len  n  keep  pos_weight
CASES = [("one row",        360,  1, 1.0, 1.0),      # BN over one row's positions
         ("real window",    360,  3, 0.5, 1.0),      # widths 180 / 90 / 45 / 23
         ("odd widths",      40,  6, 0.5, 1.0),      # widths 20 / 10 / 5 / 3, odd-length stride-2 pools, asymmetric pads
         ("partial tiles",  100, 70, 0.5, 3.0),      # widths 50 / 25 / 13 / 7, partial row tiles
         ("offset",          40,  6, 0.5, 1.0),      # signals 5 + 0.2 x N(0, 1): |mean| >> std in the stem
         ("dead",           360,  5, 0.5, 1.0),      # first and last output channel of every conv kernel zeroed: v = 0
         ("wide slabs",      40, 900, 0.5, 3.0),     # slab_rows 282 / 141 in the stem and modules 1 - 3, short last slab
         ("even slabs",      40, 832, 0.5, 1.0)]     # slab_rows 260 / 130, R a multiple of them: no remainder launch

CSRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "deepsignal_amd", "csrc")
NSLAB, MIN_SLAB_ROWS = 64, 128
#                       per width 20 / 10 / 5 / 3:  (R, slab_rows, nslab, rows in the last slab)
WIDE_SLABS = {"wide slabs": [(18000, 282, 64, 234), (9000, 141, 64, 117), (4500, 128, 36, 20), (2700, 128, 22, 12)],
              "even slabs": [(16640, 260, 64, 260), (8320, 130, 64, 130), (4160, 128, 33, 64), (2496, 128, 20, 64)]}


def slabs_of(R):
    """(rows per slab, slabs) of a reduction over R rows: slabs_of in ds_train_signal.hip, NSLAB from ds_train_signal.h."""
    slab_rows = max(MIN_SLAB_ROWS, -(-R // NSLAB))
    return slab_rows, -(-R // slab_rows)


def check_slab_rule(kind, S, n):
    """The restatement is the source's, and it cuts this case's rows as WIDE_SLABS says: a change of the rule fails here, where
    it would otherwise quietly take the case out of the regime it is there for."""
    header = open(os.path.join(CSRC, "ds_train_signal.h")).read()
    source = open(os.path.join(CSRC, "ds_train_signal.hip")).read()
    assert re.search(r"constexpr int NSLAB = %d;" % NSLAB, header), "NSLAB of ds_train_signal.h is no longer %d" % NSLAB
    assert "*slab_rows = std::max(%d, (R + NSLAB - 1) / NSLAB);" % MIN_SLAB_ROWS in source, "slabs_of of ds_train_signal.hip changed"
    assert "*nslab = (R + *slab_rows - 1) / *slab_rows;" in source, "slabs_of of ds_train_signal.hip changed"
    from deepsignal_amd import spec
    widths, W = [], S
    for k in (7, 3, 3, 3):                                   # the stem conv, then the three stride-2 pools
        W = spec.same_pad(W, k, 2)[0]
        widths.append(W)
    got = []
    for W in widths:
        slab_rows, nslab = slabs_of(n * W)
        got.append((n * W, slab_rows, nslab, n * W - (nslab - 1) * slab_rows))
    assert got == WIDE_SLABS[kind], got
    for R, slab_rows, nslab, last in got[:2]:                # the stem and modules 1 - 3: the wide regime, every slab in use
        assert slab_rows > MIN_SLAB_ROWS and nslab == NSLAB
    if kind == "wide slabs":                                 # an odd slab, no multiple of the 16-row chunk, lanes split unevenly
        assert got[1][1] % 2 == 1 and got[1][1] % 16 != 0 and got[0][1] % 4 != 0 and got[0][3] < got[0][1] and got[1][3] < got[1][1]
    else:                                                    # full == nslab: R / slab_rows exact
        assert got[0][3] == got[0][1] and got[1][3] == got[1][1]


@functools.lru_cache(maxsize=None)
def case_inputs(kind, S, n):
    from deepsignal_amd import weights
    w = weights.random_weights(seed=7, signal_len=S, is_cnn=True, is_rnn=False, randomize_bn=True)
    rng = np.random.default_rng(1000 + n + S)
    signals = rng.normal(0.0, 1.0, (n, S)).astype(np.float32)
    if kind == "offset":
        signals = (5.0 + 0.2 * signals).astype(np.float32)
    if kind == "dead":
        w = dict(w)
        for name in list(w):
            if name.endswith("/kernel") and w[name].ndim == 4:
                k = w[name].copy()
                k[..., 0] = 0.0
                k[..., -1] = 0.0
                w[name] = k
    labels = rng.integers(0, 2, n).astype(np.int32)
    return w, signals, labels


@pytest.mark.parametrize("kind,S,n,keep_prob,pos_weight", CASES, ids=[c[0].replace(" ", "_") for c in CASES])
def test_taps_decisions_gradients_loss_and_masks(kind, S, n, keep_prob, pos_weight):
    from deepsignal_amd import engine
    w, signals, labels = case_inputs(kind, S, n)
    J = tss.dims(S).joint
    wide = kind in WIDE_SLABS
    if wide:
        check_slab_rule(kind, S, n)
    eng = engine.Engine(signal_len=S, max_batch=MAX_BATCH_WIDE if wide else MAX_BATCH, is_cnn=True, is_rnn=False)
    try:
        eng.load_weights(w)
        eng.train_begin(keep_prob=keep_prob, pos_weight=pos_weight, seed=SEED)
        loss, pred = eng.train_step_signal(signals, labels, lr=0.0)
        masks = {s: eng.train_mask(s, n) for s in engine.SIGNAL_MASK_STREAMS}
        taps = {name: eng.train_tap(name, n) for name in engine.signal_tap_names()}
        grads = eng.train_grads()
        after = eng.train_tensors()
    finally:
        eng.close()
    # (1) masks, (7) parameters
    assert masks["fc1"].shape == (n, J) and masks["fc2"].shape == (n, 2)
    for s, m in masks.items():
        assert (m == engine.train_mask_reference_wide(SEED, 0, s, n, m.shape[1], keep_prob)).all(), s
        if keep_prob == 1.0:
            assert m.all()
    names = tss.trainable_names(S)
    assert len(names) == 341 and set(grads) == set(names)
    for name in names:
        assert after[name].tobytes() == np.ascontiguousarray(w[name], np.float32).tobytes(), name
    assert np.isfinite(loss) and all(np.isfinite(g).all() for g in grads.values()) and all(np.isfinite(t).all() for t in taps.values())

    # (2) forward
    _, _, _, free64 = tss.step(w, signals, labels, masks, keep_prob, pos_weight, torch.float64, grad=False)
    _, _, _, free32 = tss.step(w, signals, labels, masks, keep_prob, pos_weight, torch.float32, grad=False)
    assert set(taps) == set(free64.taps)
    bars, failures = {}, []
    for name, t in taps.items():
        ref = free64.taps[name].to(torch.float64).numpy()
        e, e32 = tss.rel_err(t, ref), tss.rel_err(free32.taps[name].to(torch.float64).numpy(), ref)
        bars[name] = (4 * max(e32, 1e-6), float(np.abs(ref).max()))
        if not e <= bars[name][0]:
            failures.append((name, e, bars[name][0]))
    worst = max(tss.rel_err(t, free64.taps[k].to(torch.float64).numpy()) / bars[k][0] for k, t in taps.items())
    print("%s: %d taps, worst distance / bar %.3g" % (kind, len(taps), worst))
    assert not failures, failures

    # (3) decisions
    dec = tss.decisions_from_taps(taps)
    diffs = tss.decision_differences(dec, free64)
    places = sum(d[1] for d in diffs)
    print("%s: decisions differ from the float64 statement's in %d places: %s" % (kind, places, diffs))
    cap = MAX_DIFFERING
    if wide:      # the float32 statement's own count of differing places sets the scale; a reference value, not the GPU's
        dec_32 = tss.decisions_from_taps({k: t.numpy() for k, t in free32.taps.items()})
        places_32 = sum(d[1] for d in tss.decision_differences(dec_32, free64))
        cap = max(MAX_DIFFERING, 2 * places_32)
        print("%s: places_32 %d, the GPU's %d, cap %d" % (kind, places_32, places, cap))
    assert places <= cap
    for name, _, margin, tap in diffs:          # a pool's places are listed per tap that feeds the differing channels
        assert margin <= bars[tap][0] * bars[tap][1], (name, tap, margin)

    # (4) gradients under the GPU's decisions
    loss64, logits64, g64, _ = tss.step(w, signals, labels, masks, keep_prob, pos_weight, torch.float64, dec=dec)
    loss32, logits32, g32, _ = tss.step(w, signals, labels, masks, keep_prob, pos_weight, torch.float32, dec=dec)
    failures, worst = [], 0.0
    for name in names:
        e, e32 = tss.rel_err(grads[name], g64[name]), tss.rel_err(g32[name], g64[name])
        bar = 4 * max(e32, 1e-6)
        worst = max(worst, e / bar)
        if not e <= bar:
            failures.append((name, e, e32, bar))
    print("%s: 341 gradients, worst distance / bar %.3g, %d above" % (kind, worst, len(failures)))
    for f in failures:
        print("   above the bar: %-90s e_gpu %.3g e_32 %.3g bar %.3g" % f)
    # (5) loss, (6) prediction
    loss_bar = max(1.0, pos_weight) * 4 * max(float(np.abs(logits32 - logits64).max()), 2.0 ** -22 * float(np.abs(logits64).max()))
    print("%s: loss gpu %.9g f64 %.9g |d| %.3g bar %.3g" % (kind, loss, loss64, abs(loss - loss64), loss_bar))
    assert not failures, failures[:5]
    assert abs(loss - loss64) <= loss_bar
    gap = np.abs(logits64[:, 1] - logits64[:, 0]) if pos_weight == 1.0 else np.abs(logits64[:, 1])
    decided = gap > loss_bar
    assert (pred[decided] == tss.pred_of(logits64, pos_weight)[decided]).all()
