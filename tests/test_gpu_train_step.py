"""GPU: the training step beyond one gradient (tests/test_gpu_train_grad.py): Adam, determinism, isolation of a batch from what
the buffers held before, a 40-step loss curve against the float64 statement, ds_train_sync_weights, and every refusal."""

import numpy as np
import pytest
import torch

import train_statement as ts

pytestmark = pytest.mark.gpu

T = 5
MAX_BATCH = 96
RNN_ONLY = dict(is_cnn=False, is_base=False)


def _w():
    from deepsignal_amd import weights
    return weights.random_weights(seed=7, kmer_len=T, **RNN_ONLY)


def _engine(w=None, **kw):
    from deepsignal_amd.engine import Engine
    args = dict(kmer_len=T, max_batch=MAX_BATCH, **RNN_ONLY)
    args.update(kw)
    eng = Engine(**args)
    if w is not None:
        eng.load_weights(w)
    return eng


def _batch(n, seed):
    feats = ts.train_features(n, T, seed)
    return feats, np.random.default_rng(seed + 1).integers(0, 2, n).astype(np.int32)


def test_adam_in_isolation():
    """Three steps; the expected parameters are the numpy float64 Adam applied to the GPU's own gradients. Bar: one ulp of theta
    plus 1e-5 lr (about nine times the six fp32 roundings on an update bounded by (1 - b1) / sqrt(1 - b2) lr = 3.2 lr)."""
    w, lr = _w(), 1e-3
    eng = _engine(w)
    try:
        eng.train_begin(keep_prob=0.5, seed=1)
        opt = ts.Adam({k: w[k] for k in ts.tensor_names()})
        for s in range(3):
            feats, labels = _batch(16, 50 + s)
            eng.train_step(feats["means"], feats["stds"], feats["sanums"], labels, lr)
            opt.update(eng.train_grads(), lr)
            got = eng.train_tensors()
            for name in ts.tensor_names():
                bar = np.spacing(np.abs(got[name])).astype(np.float64) + 1e-5 * lr
                d = np.abs(got[name].astype(np.float64) - opt.p[name])
                print("step %d %-50s worst |d| / bar %.3g" % (s, name, float((d / bar).max())))
                assert (d <= bar).all(), (s, name, float(d.max()))
            opt.p = {k: v.astype(np.float64) for k, v in got.items()}     # the next step starts from the GPU's own fp32 parameters
        assert any((got[k] != w[k]).any() for k in ts.tensor_names())
        # lr = 0: the parameters do not change by a bit (the moments still move)
        feats, labels = _batch(16, 60)
        eng.train_step(feats["means"], feats["stds"], feats["sanums"], labels, 0.0)
        same = eng.train_tensors()
        assert all(same[k].tobytes() == got[k].tobytes() for k in ts.tensor_names())
    finally:
        eng.close()


def test_two_runs_give_the_same_bits():
    w = _w()
    out = []
    for _ in range(2):
        eng = _engine(w)
        try:
            eng.train_begin(keep_prob=0.5, seed=5)
            losses = []
            for s in range(3):
                feats, labels = _batch(33, 70 + s)
                losses.append(eng.train_step(feats["means"], feats["stds"], feats["sanums"], labels, 1e-3)[0])
            out.append((losses, eng.train_tensors()))
        finally:
            eng.close()
    assert out[0][0] == out[1][0]
    for name in ts.tensor_names():
        assert out[0][1][name].tobytes() == out[1][1][name].tobytes(), name


def test_a_batch_is_isolated_from_the_one_before():
    """A 5-row step right after a 70-row step on the same handle: its gradient is the statement's for these 5 rows alone, with the
    masks ds_train_mask_reference gives rows 0 .. 4 of step 1 (a row's mask does not depend on n)."""
    from deepsignal_amd import engine
    w = _w()
    eng = _engine(w)
    try:
        eng.train_begin(keep_prob=0.5, seed=8)
        big, big_labels = _batch(70, 80)
        eng.train_step(big["means"], big["stds"], big["sanums"], big_labels, 0.0)
        feats, labels = _batch(5, 81)
        loss, _ = eng.train_step(feats["means"], feats["stds"], feats["sanums"], labels, 0.0)
        grads = eng.train_grads()
    finally:
        eng.close()
    masks = {s: engine.train_mask_reference(8, 1, s, 5, T, 0.5) for s in engine.MASK_STREAMS}
    loss64, _, g64 = ts.step(w, feats, labels, masks, 0.5, 1.0, torch.float64)
    loss32, _, g32 = ts.step(w, feats, labels, masks, 0.5, 1.0, torch.float32)
    for name in ts.tensor_names():
        e, e32 = ts.rel_err(grads[name], g64[name]), ts.rel_err(g32[name], g64[name])
        print("%-50s e_gpu %.3g e_32 %.3g" % (name, e, e32))
        assert e <= 4 * max(e32, 1e-6), (name, e, e32)
    assert abs(loss - loss64) <= 4 * max(abs(loss32 - loss64), 2.0 ** -22 * abs(loss64))


def _statement_curve(w, batches, lr, dtype):
    opt = ts.Adam({k: w[k] for k in ts.tensor_names()})
    losses = []
    for feats, labels in batches:
        cur = {k: v.astype(np.float32) if dtype == torch.float32 else v for k, v in opt.p.items()}
        if dtype == torch.float64:
            # float64 run: parameters stay float64 (ts.step casts its input to float32 first, so feed it through the tensors directly)
            wt = {k: torch.from_numpy(v).requires_grad_(True) for k, v in cur.items()}
            n = len(labels)
            loss = ts.loss_of(ts.logits_of(wt, feats, ts.no_masks(n, T), 1.0, dtype), labels, 1.0)
            loss.backward()
            grads = {k: v.grad.numpy() for k, v in wt.items()}
            losses.append(float(loss.detach()))
        else:
            l, _, grads = ts.step(cur, feats, labels, None, 1.0, 1.0, dtype)
            losses.append(l)
        opt.update(grads, lr)
    return np.array(losses)


def test_loss_curve_and_sync_weights():
    """40 steps (64 samples in batches of 16, lr 1e-3, keep_prob 1): every loss within 4 x max(float32-statement curve distance,
    2^-22 loss) of the float64 statement's. Then the forward: without ds_train_sync_weights it is still the initial weights',
    with it the trained ones' (the existing oracle with the fetched parameters, test_model_variants' bar)."""
    from deepsignal_amd import synth
    from oracle import oracle
    w, lr = _w(), 1e-3
    feats, labels = _batch(64, 90)
    batches = [({k: v[16 * (s % 4):16 * (s % 4) + 16] for k, v in feats.items()}, labels[16 * (s % 4):16 * (s % 4) + 16]) for s in range(40)]
    c64 = _statement_curve(w, batches, lr, torch.float64)
    c32 = _statement_curve(w, batches, lr, torch.float32)
    dist32 = float(np.abs(c32 - c64).max())
    fw = synth.synthetic_features(40, seed=77, kmer_len=T)
    eng = _engine(w)
    try:
        eng.train_begin(keep_prob=1.0, seed=2)
        got = np.array([eng.train_step(b["means"], b["stds"], b["sanums"], l, lr)[0] for b, l in batches])
        bars = 4 * np.maximum(dist32, 2.0 ** -22 * np.abs(c64))
        print("curve: first %.6f last %.6f (f64 %.6f .. %.6f), float32-statement distance %.3g, gpu distance %.3g" %
              (got[0], got[-1], c64[0], c64[-1], dist32, float(np.abs(got - c64).max())))
        assert np.isfinite(got).all() and (np.abs(got - c64) <= bars).all(), (np.abs(got - c64) / bars).max()
        trained = eng.train_tensors()
        variant = dict(is_cnn=False, is_rnn=True, is_base=False)
        run = lambda: eng.run(fw["kmer"], fw["means"], fw["stds"], fw["sanums"], fw["signals"])
        act0, _ = run()
        o0, _ = oracle.forward(w, fw, "f32", kmer_len=T, **variant)
        assert np.abs(act0 - o0).max() <= 1e-5
        eng.train_sync_weights()
        act1, pred1 = run()
        o1, p1 = oracle.forward(trained, fw, "f32", kmer_len=T, **variant)
        assert np.isfinite(act1).all() and np.abs(act1 - o1).max() <= 1e-5
        norm = lambda a: a / a.sum(axis=1, keepdims=True)
        assert np.abs(norm(act1) - norm(o1)).max() <= 1e-5
        decided = np.abs(o1[:, 1] - o1[:, 0]) > 1e-3
        assert (pred1[decided] == p1[decided]).all()
        assert np.abs(o1 - o0).max() > 1e-3          # the 40 steps moved the forward by far more than the bar
        # training goes on after the sync, and a new begin starts over from the loaded weights
        eng.train_step(batches[0][0]["means"], batches[0][0]["stds"], batches[0][0]["sanums"], batches[0][1], lr)
        eng.train_begin(keep_prob=1.0, seed=2)
        again = eng.train_step(batches[0][0]["means"], batches[0][0]["stds"], batches[0][0]["sanums"], batches[0][1], lr)[0]
        assert again == got[0]
        # ... or from weights installed in their place
        w2 = {k: (v * np.float32(0.5)) for k, v in w.items()}
        eng.train_begin(keep_prob=1.0, seed=2, weights=w2)
        assert eng.train_tensor("dense/kernel").tobytes() == w2["dense/kernel"].tobytes()
    finally:
        eng.close()


def test_refusals():
    from deepsignal_amd import weights
    from deepsignal_amd.engine import Engine
    feats, labels = _batch(4, 3)
    args = (feats["means"], feats["stds"], feats["sanums"])
    # variants and precisions that are not trained
    for kw, word in ((dict(is_cnn=True, is_base=False), "is_cnn"), (dict(is_cnn=False, is_base=True), "is_base"),
                     (dict(is_cnn=False, is_base=False, precision="bf16x3"), "DS_PRECISION_FP32"),
                     (dict(is_cnn=False, is_base=False, class_num=3), "class_num")):
        eng = Engine(kmer_len=T, max_batch=8, **kw)
        try:
            with pytest.raises(RuntimeError, match=r"ds_train_begin failed \(-4\).*" + word):
                eng.train_begin()
        finally:
            eng.close()
    eng = _engine()
    try:
        with pytest.raises(RuntimeError, match=r"ds_train_begin failed \(-1\).*weights not loaded"):
            eng.train_begin()
        eng.load_weights(_w())
        with pytest.raises(RuntimeError, match=r"ds_train_step failed \(-1\).*ds_train_begin first"):
            eng.train_step(*args, labels, 1e-3)
        for what in (eng.train_sync_weights, lambda: eng.train_tensor("dense/kernel"), lambda: eng.train_mask("fc1", 4)):
            with pytest.raises(RuntimeError, match=r"\(-1\).*ds_train_begin first"):
                what()
        for kp in (0.0, -0.5, 1.5, float("nan")):
            with pytest.raises(RuntimeError, match=r"ds_train_begin failed \(-1\).*keep_prob"):
                eng.train_begin(keep_prob=kp)
        for pw in (0.0, -1.0, float("nan")):
            with pytest.raises(RuntimeError, match=r"ds_train_begin failed \(-1\).*pos_weight"):
                eng.train_begin(pos_weight=pw)
        eng.train_begin(keep_prob=0.5)
        with pytest.raises(RuntimeError, match=r"ds_train_get_mask failed \(-1\).*no step"):
            eng.train_mask("fc1", 4)
        big, big_labels = _batch(MAX_BATCH + 1, 4)
        with pytest.raises(RuntimeError, match=r"ds_train_step failed \(-1\).*max_batch"):
            eng.train_step(big["means"], big["stds"], big["sanums"], big_labels, 1e-3)
        rc = eng._lib.ds_train_step(eng._h, 0, args[0].ctypes.data, args[1].ctypes.data, args[2].ctypes.data, labels.ctypes.data,
                                    1e-3, None, None)
        assert rc == -1
        for bad in (2, -1):
            lab = labels.copy()
            lab[2] = bad
            with pytest.raises(RuntimeError, match=r"ds_train_step failed \(-1\).*outside \{0, 1\}"):
                eng.train_step(*args, lab, 1e-3)
        # pipeline tickets in flight
        fw = {"kmer": np.zeros((4, T), np.int32), "signals": np.zeros((4, 360), np.float32)}
        ticket = eng.submit(fw["kmer"], *args, fw["signals"])
        with pytest.raises(RuntimeError, match=r"ds_train_step failed \(-1\).*in flight"):
            eng.train_step(*args, labels, 1e-3)
        with pytest.raises(RuntimeError, match=r"ds_train_begin failed \(-1\).*in flight"):
            eng.train_begin()
        eng.wait(ticket)
        loss, pred = eng.train_step(*args, labels, 1e-3)
        assert np.isfinite(loss) and pred.shape == (4,)
        eng.train_end()
        with pytest.raises(RuntimeError, match=r"ds_train_step failed \(-1\).*ds_train_begin first"):
            eng.train_step(*args, labels, 1e-3)
    finally:
        eng.close()
