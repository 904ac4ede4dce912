"""GPU: the training step with the embedding beyond one gradient (tests/test_gpu_train_base_grad.py): determinism, a 10-step Adam
run against the float64 statement with embedding rows that are hit once and never, ds_train_eval and what it must leave alone,
the refusals around the codes, and the is_base 0 route through the new entry points."""
import numpy as np
import pytest
import torch

import train_statement as ts
import train_statement_base as tsb

pytestmark = pytest.mark.gpu

T = 5
MAX_BATCH = 96
BASE = dict(is_cnn=False, is_base=True)
EMB = tsb.EMBEDDING


def _w(is_base=True):
    from deepsignal_amd import weights
    return weights.random_weights(seed=7, kmer_len=T, is_cnn=False, is_base=is_base)


def _engine(w=None, **kw):
    from deepsignal_amd.engine import Engine
    args = dict(kmer_len=T, max_batch=MAX_BATCH, **BASE)
    args.update(kw)
    eng = Engine(**args)
    if w is not None:
        eng.load_weights(w)
    return eng


def _batch(n, seed, kind="acgt"):
    feats = tsb.train_features(n, T, seed, kind)
    return feats, np.random.default_rng(seed + 1).integers(0, 2, n).astype(np.int32)


def _step(eng, feats, labels, lr):
    return eng.train_step(feats["means"], feats["stds"], feats["sanums"], labels, lr, kmer=feats["kmer"])


def test_two_runs_give_the_same_bits():
    w = _w()
    out = []
    for _ in range(2):
        eng = _engine(w)
        try:
            eng.train_begin(keep_prob=0.5, seed=5, base=True)
            losses = []
            for s in range(3):
                feats, labels = _batch(70, 70 + s)
                losses.append(_step(eng, feats, labels, 1e-3)[0])
            out.append((losses, eng.train_tensors(), eng.train_grads()))
        finally:
            eng.close()
    assert out[0][0] == out[1][0]
    for name in tsb.tensor_names():
        assert out[0][1][name].tobytes() == out[1][1][name].tobytes(), name
        assert out[0][2][name].tobytes() == out[1][2][name].tobytes(), name


def _statement_curve(w, batches, lr, dtype):
    opt = tsb.Adam({k: w[k] for k in tsb.tensor_names()})
    losses = []
    for feats, labels in batches:
        if dtype == torch.float64:      # the float64 run keeps float64 parameters from step to step
            l, _, grads = tsb.step(opt.p, feats, labels, None, 1.0, 1.0, dtype, exact=True)
        else:
            l, _, grads = tsb.step({k: v.astype(np.float32) for k, v in opt.p.items()}, feats, labels, None, 1.0, 1.0, dtype)
        losses.append(l)
        opt.update(grads, lr)
    return np.array(losses), opt.p


def test_ten_adam_steps_and_rows_hit_once_and_never():
    """10 steps (batches of 16, lr 1e-3, keep_prob 1), held as test_gpu_train_step.py holds its loss curve: every loss within
    4 x max(float32-statement curve distance, 2^-22 loss) of the float64 statement's. One entry of step 0 has code 9 and no later
    one: row 9 of the embedding has a zero gradient from step 1 on and still moves there, by what dense Adam on the GPU's own
    gradients gives (test_adam_in_isolation's bar: one ulp of theta plus 1e-5 lr). Row 500 is never selected and keeps its bits."""
    w, lr = _w(), 1e-3
    batches = [_batch(16, 90 + s) for s in range(10)]
    batches[0][0]["kmer"][3, 2] = 9
    assert all((b["kmer"] != 9).all() for b, _ in batches[1:]) and all((b["kmer"] != 500).all() for b, _ in batches)
    c64, _ = _statement_curve(w, batches, lr, torch.float64)
    c32, _ = _statement_curve(w, batches, lr, torch.float32)
    dist32 = float(np.abs(c32 - c64).max())
    eng = _engine(w)
    try:
        eng.train_begin(keep_prob=1.0, seed=2, base=True)
        opt = ts.Adam({EMB: w[EMB]})
        got, row9 = [], []
        for s, (feats, labels) in enumerate(batches):
            got.append(_step(eng, feats, labels, lr)[0])
            g, e = eng.train_grad(EMB), eng.train_tensor(EMB)
            opt.update({EMB: g}, lr)
            bar = np.spacing(np.abs(e)).astype(np.float64) + 1e-5 * lr
            assert (np.abs(e.astype(np.float64) - opt.p[EMB]) <= bar).all(), s
            opt.p = {EMB: e.astype(np.float64)}
            if s >= 1:
                assert not g[9].view(np.uint32).any()
            row9.append(e[9].copy())
        got = np.array(got)
        bars = 4 * np.maximum(dist32, 2.0 ** -22 * np.abs(c64))
        print("curve: first %.6f last %.6f (f64 %.6f .. %.6f), float32-statement distance %.3g, gpu distance %.3g" %
              (got[0], got[-1], c64[0], c64[-1], dist32, float(np.abs(got - c64).max())))
        assert np.isfinite(got).all() and (np.abs(got - c64) <= bars).all(), (np.abs(got - c64) / bars).max()
        assert (row9[0] != w[EMB][9]).any() and (row9[1] != row9[0]).any()       # hit in step 0; moved again in step 1 without being hit
        assert eng.train_tensor(EMB)[500].tobytes() == w[EMB][500].tobytes()
    finally:
        eng.close()


def test_eval_changes_nothing_and_is_the_forward():
    from deepsignal_amd import engine
    from test_gpu_parity import ACT_ATOL
    w, n = _w(), 70
    f0, l0 = _batch(n, 30)
    f1, l1 = _batch(n, 31)
    fv, lv = _batch(33, 32, "hostile")
    eng, ref = _engine(w), _engine(w)
    try:
        for e in (eng, ref):
            e.train_begin(keep_prob=0.5, pos_weight=1.0, seed=4, base=True)
            _step(e, f0, l0, 1e-3)
        before = (eng.train_tensors(), eng.train_grads(), {s: eng.train_mask(s, n) for s in engine.MASK_STREAMS})
        loss, pred, logits = eng.train_eval(fv["means"], fv["stds"], fv["sanums"], lv, kmer=fv["kmer"])
        after = (eng.train_tensors(), eng.train_grads(), {s: eng.train_mask(s, n) for s in engine.MASK_STREAMS})
        for b, a in zip(before, after):
            for name in b:
                assert b[name].tobytes() == a[name].tobytes(), name
        # the float64 statement on the same parameters, keep_prob 1, every mask kept; the gradient test's loss bar, and the same
        # form of bar on the logits (the float32 statement's own distance on them, or 2^-22 of their scale)
        l64, g64, _ = tsb.step(before[0], fv, lv, None, 1.0, 1.0, torch.float64)
        l32, g32, _ = tsb.step(before[0], fv, lv, None, 1.0, 1.0, torch.float32)
        loss_bar = 4 * max(abs(l32 - l64), 2.0 ** -22 * abs(l64))
        logit_bar = 4 * max(float(np.abs(g32 - g64).max()), 2.0 ** -22 * float(np.abs(g64).max()))
        print("eval loss gpu %.9g f64 %.9g |d| %.3g bar %.3g; logits |d| %.3g bar %.3g" %
              (loss, l64, abs(loss - l64), loss_bar, float(np.abs(logits - g64).max()), logit_bar))
        assert abs(loss - l64) <= loss_bar and np.abs(logits - g64).max() <= logit_bar
        decided = np.abs(g64[:, 1] - g64[:, 0]) > logit_bar
        assert (pred[decided] == tsb.pred_of(g64, 1.0)[decided]).all()
        # the next step is the one a run without the eval takes: same masks (the step counter did not move), same parameters
        # (the moments did not move), same gradients
        out = [_step(e, f1, l1, 1e-3)[0] for e in (eng, ref)]
        assert out[0] == out[1]
        for s in engine.MASK_STREAMS:
            assert (eng.train_mask(s, n) == ref.train_mask(s, n)).all() and (eng.train_mask(s, n) == engine.train_mask_reference(4, 1, s, n, T, 0.5)).all()
        ta, tb, ga, gb = eng.train_tensors(), ref.train_tensors(), eng.train_grads(), ref.train_grads()
        for name in tsb.tensor_names():
            assert ta[name].tobytes() == tb[name].tobytes() and ga[name].tobytes() == gb[name].tobytes(), name
        # after the hand-over the inference forward computes sigmoid of what the evaluation pass computes
        _, _, logits = eng.train_eval(fv["means"], fv["stds"], fv["sanums"], lv, kmer=fv["kmer"])
        eng.train_sync_weights()
        act, _ = eng.run(fv["kmer"], fv["means"], fv["stds"], fv["sanums"], np.zeros((33, 360), np.float32))
        assert np.abs(act - 1.0 / (1.0 + np.exp(-logits.astype(np.float64)))).max() <= ACT_ATOL
        assert np.abs(eng.train_tensor(EMB) - w[EMB]).max() > 0          # the embedding it handed over is a trained one
    finally:
        eng.close()
        ref.close()


def test_eval_uses_the_runs_pos_weight():
    w = _w()
    fv, lv = _batch(20, 40)
    eng = _engine(w)
    try:
        eng.train_begin(keep_prob=0.5, pos_weight=3.0, seed=1, base=True)
        loss, pred, logits = eng.train_eval(fv["means"], fv["stds"], fv["sanums"], lv, kmer=fv["kmer"])
    finally:
        eng.close()
    l64, g64, _ = tsb.step(w, fv, lv, None, 1.0, 3.0, torch.float64)
    l32, _, _ = tsb.step(w, fv, lv, None, 1.0, 3.0, torch.float32)
    assert abs(loss - l64) <= 4 * max(abs(l32 - l64), 2.0 ** -22 * abs(l64))
    decided = np.abs(g64[:, 1]) > 1e-5
    assert (pred[decided] == tsb.pred_of(g64, 3.0)[decided]).all()


def test_refusals_around_the_codes():
    feats, labels = _batch(4, 3)
    args = (feats["means"], feats["stds"], feats["sanums"])
    eng = _engine(_w())
    try:
        with pytest.raises(RuntimeError, match=r"ds_train_begin failed \(-4\).*is_base"):      # the old entry still refuses the handle
            eng.train_begin()
        with pytest.raises(RuntimeError, match=r"ds_train_step_base failed \(-1\).*ds_train_begin first"):
            eng.train_step(*args, labels, 1e-3, kmer=feats["kmer"])
        with pytest.raises(RuntimeError, match=r"ds_train_eval failed \(-1\).*ds_train_begin first"):
            eng.train_eval(*args, labels, kmer=feats["kmer"])
        eng.train_begin(base=True)
        with pytest.raises(RuntimeError, match=r"ds_train_step failed \(-1\).*k-mer codes"):     # no codes on a run that embeds them
            eng.train_step(*args, labels, 1e-3)
        with pytest.raises(RuntimeError, match=r"ds_train_eval failed \(-1\).*k-mer codes"):
            eng.train_eval(*args, labels)
        with pytest.raises(ValueError):
            eng.train_step(*args, labels, 1e-3, kmer=feats["kmer"][:, :3])
        lab = labels.copy()
        lab[1] = 2
        with pytest.raises(RuntimeError, match=r"ds_train_eval failed \(-1\).*outside \{0, 1\}"):
            eng.train_eval(*args, lab, kmer=feats["kmer"])
        loss, pred = eng.train_step(*args, labels, 1e-3, kmer=feats["kmer"])
        assert np.isfinite(loss) and pred.shape == (4,)
    finally:
        eng.close()
    for kw, word in ((dict(is_cnn=True, is_base=True), "is_cnn"), (dict(is_cnn=False, is_base=True, class_num=3), "class_num"),
                     (dict(is_cnn=False, is_base=True, precision="bf16x3"), "DS_PRECISION_FP32")):
        eng = _engine(**kw)
        try:
            with pytest.raises(RuntimeError, match=r"ds_train_begin_base failed \(-4\).*" + word):
                eng.train_begin(base=True)
        finally:
            eng.close()


def test_is_base_0_through_the_base_entries_gives_the_old_bits():
    w = _w(is_base=False)
    out = []
    for new in (False, True):
        eng = _engine(w, is_base=False)
        try:
            eng.train_begin(keep_prob=0.5, pos_weight=3.0, seed=6, base=new)
            losses = []
            for s in range(3):
                feats, labels = _batch(33, 50 + s, "wide")
                losses.append(eng.train_step(feats["means"], feats["stds"], feats["sanums"], labels, 1e-3, kmer=feats["kmer"] if new else None)[0])
            assert set(eng.train_tensors()) == set(ts.tensor_names())
            with pytest.raises(KeyError):
                eng.train_tensor(EMB)
            out.append((losses, eng.train_tensors(), eng.train_grads()))
            if new:         # the evaluation pass of this variant takes no codes
                feats, labels = _batch(33, 60)
                loss, _, _ = eng.train_eval(feats["means"], feats["stds"], feats["sanums"], labels)
                l64, _, _ = ts.step(out[-1][1], feats, labels, None, 1.0, 3.0, torch.float64)
                l32, _, _ = ts.step(out[-1][1], feats, labels, None, 1.0, 3.0, torch.float32)
                assert abs(loss - l64) <= 4 * max(abs(l32 - l64), 2.0 ** -22 * abs(l64))
        finally:
            eng.close()
    assert out[0][0] == out[1][0]
    for name in ts.tensor_names():
        assert out[0][1][name].tobytes() == out[1][1][name].tobytes() and out[0][2][name].tobytes() == out[1][2][name].tobytes(), name
