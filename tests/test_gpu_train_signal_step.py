"""GPU: the signal-only model's training step beyond one gradient (tests/test_gpu_train_signal_grad.py): determinism, one Adam
step and three in isolation, a narrow step right after a wide one, the moving statistics over three steps, the evaluation
pass and what it must leave alone, the hand-over to the inference plan, memorisation of a fixed batch, and the refusals."""
import numpy as np
import pytest
import torch

import train_statement_signal as tss

pytestmark = pytest.mark.gpu

S = 40
MAX_BATCH = 96
SIGNAL = dict(is_cnn=True, is_rnn=False)


def _w(signal_len=S):
    from deepsignal_amd import weights
    return weights.random_weights(seed=7, signal_len=signal_len, randomize_bn=True, **SIGNAL)


def _engine(w=None, **kw):
    from deepsignal_amd.engine import Engine
    args = dict(signal_len=S, max_batch=MAX_BATCH, **SIGNAL)
    args.update(kw)
    eng = Engine(**args)
    if w is not None:
        eng.load_weights(w)
    return eng


def _batch(n, seed, signal_len=S):
    rng = np.random.default_rng(seed)
    return rng.normal(0.0, 1.0, (n, signal_len)).astype(np.float32), rng.integers(0, 2, n).astype(np.int32)


def _same_bits(a, b):
    assert set(a) == set(b)
    for name in a:
        assert a[name].tobytes() == b[name].tobytes(), name


def test_two_runs_give_the_same_bits():
    """Two handles, and on the second a run begun over after a first one: the same losses, tensors (moving statistics included),
    gradients and taps, bit for bit."""
    w = _w()
    out = []

    def run(eng):
        eng.train_begin(keep_prob=0.5, seed=5)
        losses = []
        for s in range(3):
            sig, lab = _batch(70, 70 + s)
            losses.append(eng.train_step_signal(sig, lab, 1e-3)[0])
        return losses, eng.train_tensors(), eng.train_grads(), {k: eng.train_tap(k, 70) for k in ("stem1", "m4.b1", "m11.b5", "logits")}

    for again in (False, True):
        eng = _engine(w)
        try:
            out.append(run(eng))
            if again:
                out.append(run(eng))          # ds_train_begin_signal starts over from the loaded weights: moments, step, statistics
        finally:
            eng.close()
    for other in out[1:]:
        assert out[0][0] == other[0]
        for k in (1, 2, 3):
            _same_bits(out[0][k], other[k])


def test_one_adam_step():
    """theta_1 = theta_0 - lr g / (|g| + eps'), eps' = eps / sqrt(1 - beta2) (Adam's first step). On the GPU's own gradients every
    element is held to one ulp of theta plus 1e-5 lr (test_gpu_train_step.py's bar for Adam in isolation). On the float64
    statement's gradients under the GPU's decisions the bar adds what the gradient test allows the gradient to be off by,
    delta = 4 max(e_32, 1e-6) max|g_64|, through the step's slope: lr delta eps' / (max(|g_64| - delta, 0) + eps')^2."""
    from deepsignal_amd import engine
    w, lr, n = _w(), 1e-3, 6
    sig, lab = _batch(n, 21)
    eng = _engine(w)
    try:
        eng.train_begin(keep_prob=0.5, seed=3)
        eng.train_step_signal(sig, lab, lr)
        masks = {s: eng.train_mask(s, n) for s in ("fc1", "fc2")}
        taps = {name: eng.train_tap(name, n) for name in engine.signal_tap_names()}
        g, after = eng.train_grads(), eng.train_tensors()
    finally:
        eng.close()
    dec = tss.decisions_from_taps(taps)
    _, _, g64, _ = tss.step(w, sig, lab, masks, 0.5, 1.0, torch.float64, dec=dec)
    _, _, g32, _ = tss.step(w, sig, lab, masks, 0.5, 1.0, torch.float32, dec=dec)
    eps1 = 1e-8 / np.sqrt(1 - 0.999)
    for name in tss.trainable_names(S):
        theta0 = np.asarray(w[name], np.float64)
        ulp = np.spacing(np.abs(after[name])).astype(np.float64) + 1e-5 * lr
        own = theta0 - lr * g[name].astype(np.float64) / (np.abs(g[name].astype(np.float64)) + eps1)
        assert (np.abs(after[name] - own) <= ulp).all(), name
        delta = 4 * max(tss.rel_err(g32[name], g64[name]), 1e-6) * np.abs(g64[name]).max()
        ref = theta0 - lr * g64[name] / (np.abs(g64[name]) + eps1)
        slope = eps1 / (np.maximum(np.abs(g64[name]) - delta, 0.0) + eps1) ** 2
        assert (np.abs(after[name] - ref) <= ulp + lr * delta * slope).all(), name
        if np.abs(g[name]).max() > 1e-6:          # far above eps': the step is lr in size, far above an ulp of theta
            assert (after[name] != w[name]).any(), name


def test_adam_three_steps_in_isolation():
    """test_adam_in_isolation of test_gpu_train_step.py over this variant's block (113 kernels, beta, gamma, the J x J dense/kernel,
    dense_1/kernel). Three steps on three batches; after each the expected parameters are the numpy float64 Adam applied to the
    GPU's own gradients, from the GPU's own fp32 parameters of the step before: steps 2 and 3 run on non-zero moments and a
    bias-corrected step size. Bar: one ulp of theta plus 1e-5 lr on every element. A fourth step at lr = 0 moves no bit."""
    import train_statement as ts
    w, lr, n = _w(), 1e-3, 6
    names = tss.trainable_names(S)
    assert len(names) == 341
    eng = _engine(w)
    try:
        eng.train_begin(keep_prob=0.5, seed=1)
        opt = ts.Adam({k: np.asarray(w[k], np.float32) for k in names})
        for s in range(3):
            sig, lab = _batch(n, 50 + s)
            eng.train_step_signal(sig, lab, lr)
            g = eng.train_grads()
            assert set(g) == set(names)
            opt.update(g, lr)
            got = eng.train_tensors()
            worst = 0.0
            for name in names:
                bar = np.spacing(np.abs(got[name])).astype(np.float64) + 1e-5 * lr
                d = np.abs(got[name].astype(np.float64) - opt.p[name])
                worst = max(worst, float((d / bar).max()))
                assert (d <= bar).all(), (s, name, float(d.max()))
            print("step %d: 341 tensors, worst |d| / bar %.3g" % (s, worst))
            opt.p = {k: got[k].astype(np.float64) for k in names}     # the next step starts from the GPU's own fp32 parameters
        assert (got["dense/kernel"] != w["dense/kernel"]).any()
        sig, lab = _batch(n, 60)
        eng.train_step_signal(sig, lab, 0.0)      # lr = 0: not a bit of a parameter changes (the moments still move)
        same = eng.train_tensors()
        for name in names:
            assert same[name].tobytes() == got[name].tobytes(), name
    finally:
        eng.close()


def test_a_narrow_step_is_isolated_from_the_wide_one_before():
    """`part` ([64][2][256]) and `slab` ([64][largest kernel]) are scratch that every step reuses. Handle A takes 900 rows (R = 18000
    / 9000 / 4500 / 2700: all 64 slabs filled at the first two widths), then 6 rows (R = 120 / 60 / 30 / 18: one slab); handle B
    takes one unrelated row, then the same 6. Everything at lr = 0, so the parameters stand still, a training-mode forward uses
    batch statistics only, and the masks depend on (seed, step, row): step 1 agrees bit for bit between the two -- loss,
    predictions, every tap, all 341 gradients, both masks (the moving statistics legitimately differ). And A's step 1 is the
    float64 statement's for these 6 rows alone, at the bars of test_gpu_train_signal_grad.py: taps, decisions (at most 16 differing
    places, each inside its margin), gradients under the GPU's decisions, loss."""
    from deepsignal_amd import engine
    w, n, keep, seed = _w(), 6, 0.5, 8
    wide_s, wide_l = _batch(900, 90)
    one_s, one_l = _batch(1, 92)
    sig, lab = _batch(n, 91)
    out = []
    for first_s, first_l in ((wide_s, wide_l), (one_s, one_l)):
        eng = _engine(w, max_batch=1024)
        try:
            eng.train_begin(keep_prob=keep, seed=seed)
            eng.train_step_signal(first_s, first_l, 0.0)
            loss, pred = eng.train_step_signal(sig, lab, 0.0)
            out.append((loss, pred, {name: eng.train_tap(name, n) for name in engine.signal_tap_names()}, eng.train_grads(),
                        {s: eng.train_mask(s, n) for s in engine.SIGNAL_MASK_STREAMS}, eng.train_tensors()))
        finally:
            eng.close()
    (loss, pred, taps, grads, masks, after), other = out
    assert loss == other[0] and pred.tobytes() == other[1].tobytes()
    for k in (2, 3, 4):
        _same_bits(out[0][k], other[k])
    names = tss.trainable_names(S)
    assert len(names) == 341 and set(grads) == set(names)
    for name in names:
        assert after[name].tobytes() == np.ascontiguousarray(w[name], np.float32).tobytes(), name
    for s, m in masks.items():
        assert (m == engine.train_mask_reference_wide(seed, 1, s, n, m.shape[1], keep)).all(), s

    # the statement for the 6 rows alone
    _, _, _, free64 = tss.step(w, sig, lab, masks, keep, 1.0, torch.float64, grad=False)
    _, _, _, free32 = tss.step(w, sig, lab, masks, keep, 1.0, torch.float32, grad=False)
    assert set(taps) == set(free64.taps)
    bars = {}
    for name, t in taps.items():
        ref = free64.taps[name].to(torch.float64).numpy()
        bars[name] = (4 * max(tss.rel_err(free32.taps[name].to(torch.float64).numpy(), ref), 1e-6), float(np.abs(ref).max()))
        assert tss.rel_err(t, ref) <= bars[name][0], (name, tss.rel_err(t, ref), bars[name][0])
    dec = tss.decisions_from_taps(taps)
    diffs = tss.decision_differences(dec, free64)
    print("narrow after wide: decisions differ from the float64 statement's in %d places: %s" % (sum(d[1] for d in diffs), diffs))
    assert sum(d[1] for d in diffs) <= 16
    for name, _, margin, tap in diffs:
        assert margin <= bars[tap][0] * bars[tap][1], (name, tap, margin)
    loss64, logits64, g64, _ = tss.step(w, sig, lab, masks, keep, 1.0, torch.float64, dec=dec)
    loss32, logits32, g32, _ = tss.step(w, sig, lab, masks, keep, 1.0, torch.float32, dec=dec)
    worst = 0.0
    for name in names:
        e, bar = tss.rel_err(grads[name], g64[name]), 4 * max(tss.rel_err(g32[name], g64[name]), 1e-6)
        worst = max(worst, e / bar)
        assert e <= bar, (name, e, bar)
    loss_bar = 4 * max(float(np.abs(logits32 - logits64).max()), 2.0 ** -22 * float(np.abs(logits64).max()))
    print("narrow after wide: 341 gradients, worst distance / bar %.3g; loss gpu %.9g f64 %.9g |d| %.3g bar %.3g"
          % (worst, loss, loss64, abs(loss - loss64), loss_bar))
    assert abs(loss - loss64) <= loss_bar
    decided = np.abs(logits64[:, 1] - logits64[:, 0]) > loss_bar
    assert (pred[decided] == tss.pred_of(logits64, 1.0)[decided]).all()


def test_moving_statistics_three_steps():
    """Three lr = 0 steps on three batches: moving_mean and moving_variance against the rule (decay 0.9, zero-debiased mean, unbiased
    variance) applied to the float64 statement's batch statistics; per tensor max|d| / max|ref| <= 4 x max(the same rule on the
    float32 statement's statistics, 1e-6)."""
    w = _w()
    batches = [_batch(n, 40 + n) for n in (6, 33, 70)]
    eng = _engine(w)
    try:
        eng.train_begin(keep_prob=0.5, seed=1)
        for sig, lab in batches:
            eng.train_step_signal(sig, lab, 0.0)
        got = eng.train_tensors()
    finally:
        eng.close()
    runs64 = [tss.step(w, sig, lab, None, 1.0, 1.0, torch.float64, grad=False)[3] for sig, lab in batches]
    runs32 = [tss.step(w, sig, lab, None, 1.0, 1.0, torch.float32, grad=False)[3] for sig, lab in batches]
    ref, ref32 = tss.moving_after(w, runs64), tss.moving_after(w, runs32)
    assert len(ref) == 226
    worst = 0.0
    for name in ref:
        e, bar = tss.rel_err(got[name], ref[name]), 4 * max(tss.rel_err(ref32[name], ref[name]), 1e-6)
        worst = max(worst, e / bar)
        assert e <= bar, (name, e, bar)
        assert (got[name] != w[name]).any(), name
    print("moving statistics: worst distance / bar %.3g" % worst)
    for name in tss.trainable_names(S):       # lr = 0
        assert got[name].tobytes() == np.ascontiguousarray(w[name], np.float32).tobytes(), name


def test_eval_changes_nothing_is_the_inference_forward_and_syncs():
    from test_gpu_parity import ACT_ATOL
    w, n = _w(), 33
    s0, l0 = _batch(n, 30)
    s1, l1 = _batch(n, 31)
    sv, lv = _batch(20, 32)
    eng, ref = _engine(w), _engine(w)
    try:
        for e in (eng, ref):
            e.train_begin(keep_prob=0.5, seed=4)
            e.train_step_signal(s0, l0, 1e-3)
        before = (eng.train_tensors(), eng.train_grads(), {s: eng.train_mask(s, n) for s in ("fc1", "fc2")})
        loss, pred, logits = eng.train_eval_signal(sv, lv)
        after = (eng.train_tensors(), eng.train_grads(), {s: eng.train_mask(s, n) for s in ("fc1", "fc2")})
        for b, a in zip(before, after):
            _same_bits(b, a)
        # the taps are the step's scratch, which the evaluation has overwritten with its own 20 rows: refused until the next step
        with pytest.raises(RuntimeError, match=r"ds_train_get_tap failed \(-1\).*overwritten by an evaluation"):
            eng.train_tap("stem1", n)
        # the inference-mode statement on the handle's parameters and moving statistics
        l64, g64, _, _ = tss.step(before[0], sv, lv, None, 1.0, 1.0, torch.float64, training=False, grad=False)
        l32, g32, _, _ = tss.step(before[0], sv, lv, None, 1.0, 1.0, torch.float32, training=False, grad=False)
        logit_bar = 4 * max(float(np.abs(g32 - g64).max()), 2.0 ** -22 * float(np.abs(g64).max()))
        print("eval loss gpu %.9g f64 %.9g |d| %.3g; logits |d| %.3g bar %.3g" % (loss, l64, abs(loss - l64), float(np.abs(logits - g64).max()), logit_bar))
        assert np.abs(logits - g64).max() <= logit_bar and abs(loss - l64) <= logit_bar
        decided = np.abs(g64[:, 1] - g64[:, 0]) > logit_bar
        assert (pred[decided] == tss.pred_of(g64, 1.0)[decided]).all()
        # the next step is the one a run without the eval takes: step counter, moments, moving statistics did not move
        out = [e.train_step_signal(s1, l1, 1e-3)[0] for e in (eng, ref)]
        assert out[0] == out[1]
        assert eng.train_tap("stem1", n).tobytes() == ref.train_tap("stem1", n).tobytes()
        _same_bits(eng.train_tensors(), ref.train_tensors())
        _same_bits(eng.train_grads(), ref.train_grads())
        for s in ("fc1", "fc2"):
            assert (eng.train_mask(s, n) == ref.train_mask(s, n)).all()
        # after the hand-over the inference forward computes sigmoid of what the evaluation pass computes
        _, _, logits = eng.train_eval_signal(sv, lv)
        eng.train_sync_weights()
        z = np.zeros((20, 17), np.float32)
        act, _ = eng.run(z.astype(np.int32), z, z, z, sv)
        assert np.abs(act - 1.0 / (1.0 + np.exp(-logits.astype(np.float64)))).max() <= ACT_ATOL
    finally:
        eng.close()
        ref.close()


def test_memorises_a_fixed_batch():
    """20 steps at lr 1e-3, keep_prob 1 on 32 fixed rows with random labels bring the loss below a tenth of the first step's (the
    float32 statement reaches 1e-4 of it)."""
    w = _w()
    sig, lab = _batch(32, 77)
    eng = _engine(w)
    try:
        eng.train_begin(keep_prob=1.0, seed=0)
        losses = [eng.train_step_signal(sig, lab, 1e-3)[0] for _ in range(20)]
    finally:
        eng.close()
    print("memorisation: first %.6g last %.6g" % (losses[0], losses[-1]))
    assert np.isfinite(losses).all() and losses[-1] < 0.1 * losses[0]


def test_refusals():
    sig, lab = _batch(4, 3)
    for kw, entry, word in ((dict(is_cnn=True, is_rnn=True), "ds_train_begin", "is_cnn"),
                            (dict(is_cnn=True, is_rnn=False, class_num=3), "ds_train_begin_signal", "class_num"),
                            (dict(is_cnn=True, is_rnn=False, precision="bf16x3"), "ds_train_begin_signal", "DS_PRECISION_FP32"),
                            (dict(is_cnn=True, is_rnn=False, signal_len=4400, max_batch=1), "ds_train_begin_signal", "65535.*16 bits")):
        eng = _engine(**kw)
        try:
            with pytest.raises(RuntimeError, match=entry + r" failed \(-4\).*" + word):
                eng.train_begin()
        finally:
            eng.close()
    from deepsignal_amd import weights
    rnn = _engine(weights.random_weights(seed=7, kmer_len=5, is_cnn=False, is_base=False), kmer_len=5, is_cnn=False, is_rnn=True, is_base=False)
    try:
        # the signal entry refuses a BiLSTM handle outright, and a BiLSTM run refuses the signal step
        import ctypes
        from deepsignal_amd.engine import DsTrainConfig
        cfg = DsTrainConfig(0.5, 1.0, 0.0, 0.0, 0.0, 0)
        with pytest.raises(RuntimeError, match=r"ds_train_begin_signal failed \(-4\).*is_cnn must be 1 and is_rnn 0"):
            rnn._check(rnn._lib.ds_train_begin_signal(rnn._h, ctypes.byref(cfg)), "ds_train_begin_signal")
        rnn.train_begin()
        with pytest.raises(RuntimeError, match=r"ds_train_step_signal failed \(-1\).*BiLSTM"):
            rnn.train_step_signal(sig, lab, 1e-3)
        with pytest.raises(RuntimeError, match=r"ds_train_get_tap failed \(-1\).*signal run"):
            rnn._check(rnn._lib.ds_train_get_tap(rnn._h, b"feat", sig.ctypes.data, sig.size), "ds_train_get_tap")
    finally:
        rnn.close()
    eng = _engine(_w())
    try:
        with pytest.raises(RuntimeError, match=r"ds_train_step_signal failed \(-1\).*ds_train_begin first"):
            eng.train_step_signal(sig, lab, 1e-3)
        eng.train_begin()
        z = np.zeros((4, 17), np.float32)
        with pytest.raises(RuntimeError, match=r"ds_train_step_base failed \(-1\).*signal model"):
            eng.train_step(z, z, z, lab, 1e-3, kmer=z.astype(np.int32))
        with pytest.raises(RuntimeError, match=r"ds_train_get_tap failed \(-1\).*no step has run"):
            eng.train_tap("feat", 4)
        big_s, big_l = _batch(MAX_BATCH + 1, 5)
        with pytest.raises(RuntimeError, match=r"ds_train_step_signal failed \(-1\).*max_batch"):
            eng.train_step_signal(big_s, big_l, 1e-3)
        with pytest.raises(RuntimeError, match=r"ds_train_step_signal failed \(-1\).*max_batch"):
            eng.train_step_signal(sig[:0], lab[:0], 1e-3)
        bad = lab.copy()
        bad[1] = 2
        with pytest.raises(RuntimeError, match=r"ds_train_eval_signal failed \(-1\).*outside \{0, 1\}"):
            eng.train_eval_signal(sig, bad)
        with pytest.raises(ValueError):
            eng.train_step_signal(sig[:, :30], lab, 1e-3)
        with pytest.raises(RuntimeError, match=r"ds_train_get_grad failed \(-1\).*not trained"):
            eng._check(eng._lib.ds_train_get_grad(eng._h, b"modelsignalmconv_layer1/bn/moving_mean", sig.ctypes.data, sig.size), "ds_train_get_grad")
        with pytest.raises(RuntimeError, match=r"ds_train_get_mask failed \(-1\).*fc1 and fc2"):
            eng.train_step_signal(sig, lab, 1e-3)
            eng._check(eng._lib.ds_train_get_mask(eng._h, b"fw_l0", sig.ctypes.data, sig.size), "ds_train_get_mask")
        loss, pred = eng.train_step_signal(sig, lab, 1e-3)
        assert np.isfinite(loss) and pred.shape == (4,)
    finally:
        eng.close()
