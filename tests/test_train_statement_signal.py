"""CPU: tests/train_statement_signal.py held to central differences (signal_len 40, n 4), the decision-constrained run shown to
repeat the free run bit for bit on the run's own decisions, the decisions recovered from a run's taps, and the inference-mode
statement against the oracle's float64 forward of the same weights."""
import numpy as np
import torch

import train_statement_signal as tss

S, N = 40, 4


def _case(seed=3, keep_prob=0.5):
    from deepsignal_amd import weights
    w = weights.random_weights(seed=7, signal_len=S, is_cnn=True, is_rnn=False, randomize_bn=True)
    rng = np.random.default_rng(seed)
    signals = rng.normal(0.0, 1.0, (N, S)).astype(np.float32)
    labels = rng.integers(0, 2, N).astype(np.int32)
    J = tss.dims(S).joint
    masks = {"fc1": (rng.random((N, J)) < keep_prob).astype(np.uint8), "fc2": np.ones((N, 2), np.uint8)}
    return w, signals, labels, masks, keep_prob


def test_names_and_shapes():
    assert len(tss.tensor_names(S)) == 113 * 5 + 2 and len(tss.trainable_names(S)) == 341
    assert len(tss.bn_scopes()) == 113
    w, signals, labels, masks, keep = _case()
    _, logits, grads, run = tss.step(w, signals, labels, masks, keep)
    d = tss.dims(S)
    assert logits.shape == (N, 2) and run.taps["feat"].shape == (N, d.joint) and run.taps["stem1"].shape == (N, d.w_conv1, 64)
    assert run.taps["m11.b5"].shape == (N, d.w_c, 48) and len(run.taps) == 3 + 11 * 11 + 2
    assert set(grads) == set(tss.trainable_names(S)) and all(grads[k].shape == w[k].shape for k in grads)


def test_gradients_against_central_differences():
    """Directional derivatives in float64 along random directions over groups of the 341 tensors. The two displaced points keep
    the base point's decisions (`dec`): the loss is smooth in between, and its derivative at the base point is the free run's
    gradient, since no ReLU input or pool gap of the base point is exactly zero (asserted)."""
    for pos_weight in (1.0, 3.0):
        w, signals, labels, masks, keep = _case()
        w64 = {k: np.asarray(v, np.float64) for k, v in w.items()}
        _, _, grads, run = tss.step(w64, signals, labels, masks, keep, pos_weight, exact=True)
        dec = (run.relu, run.pool)
        assert all(float(z.abs().min()) > 0 for z in run.z.values())
        names = tss.trainable_names(S)
        groups = {"all": names, "kernels": [k for k in names if k.endswith("/kernel") and "dense" not in k],
                  "gamma": [k for k in names if k.endswith("/gamma")], "beta": [k for k in names if k.endswith("/beta")],
                  "dense": ["dense/kernel", "dense_1/kernel"], "stem1": [k for k in names if "conv_layer1" in k]}
        rng = np.random.default_rng(11)
        for gname, members in groups.items():
            direction = {k: rng.normal(0.0, 1.0, w64[k].shape) * np.abs(w64[k]).max() for k in members}
            analytic = sum(float((grads[k] * direction[k]).sum()) for k in members)
            h = 1e-7
            vals = []
            for sign in (1.0, -1.0):
                wp = dict(w64)
                for k in members:
                    wp[k] = w64[k] + sign * h * direction[k]
                vals.append(tss.step(wp, signals, labels, masks, keep, pos_weight, dec=dec, exact=True, grad=False)[0])
            numeric = (vals[0] - vals[1]) / (2 * h)
            print("pos_weight %g %-8s analytic %.9g central %.9g" % (pos_weight, gname, analytic, numeric))
            assert abs(numeric - analytic) <= 1e-6 * max(abs(analytic), 1e-3), gname


def test_constrained_run_on_its_own_decisions_repeats_the_free_run():
    w, signals, labels, masks, keep = _case()
    for dtype in (torch.float64, torch.float32):
        l0, logits0, g0, run0 = tss.step(w, signals, labels, masks, keep, 1.0, dtype)
        l1, logits1, g1, run1 = tss.step(w, signals, labels, masks, keep, 1.0, dtype, dec=(run0.relu, run0.pool))
        assert l0 == l1 and logits0.tobytes() == logits1.tobytes()
        for k in g0:
            assert g0[k].tobytes() == g1[k].tobytes(), k
        # ... and the decisions are recoverable from the taps alone, as the GPU test recovers the GPU's
        relu, pool = tss.decisions_from_taps({k: v.numpy() for k, v in run0.taps.items()})
        assert set(relu) == set(run0.relu) and set(pool) == set(run0.pool)
        assert all(bool((relu[k] == run0.relu[k]).all()) for k in relu) and all(bool((pool[k] == run0.pool[k]).all()) for k in pool)
        assert tss.decision_differences((relu, pool), run0) == []


def test_first_maximum_on_ties():
    win = torch.tensor([[2.0, 2.0, 1.0], [float("-inf"), 3.0, 3.0], [0.0, 0.0, 0.0], [1.0, 2.0, 2.0]])
    assert tss.first_argmax(win).tolist() == [0, 1, 0, 1]


def test_inference_mode_is_the_oracles_forward():
    from oracle import torch_statement
    w, signals, labels, _, _ = _case()
    _, logits, _, _ = tss.step(w, signals, labels, None, 1.0, 1.0, torch.float64, training=False, grad=False)
    feats = {"signals": signals, "kmer": np.zeros((N, 17), np.int32), "means": np.zeros((N, 17), np.float32),
             "stds": np.zeros((N, 17), np.float32), "sanums": np.zeros((N, 17), np.float32)}
    act, _ = torch_statement.forward(w, feats, is_cnn=True, is_rnn=False)
    assert np.abs(np.asarray(act, np.float64) - 1.0 / (1.0 + np.exp(-logits))).max() <= 1e-6


def test_moving_statistics_rule():
    w, signals, labels, masks, keep = _case()
    _, _, _, run = tss.step(w, signals, labels, masks, keep, grad=False)
    after = tss.moving_after(w, [run, run])
    bn, tap = next(iter(tss.bn_scopes().items()))
    m, v = (t.numpy() for t in run.stats[tap])
    n_el = N * tss.dims(S).w_conv1
    assert np.allclose(after[bn + "/moving_mean"], m, rtol=1e-12)        # zero-debiased: two equal batches give the batch mean
    mv0 = np.asarray(w[bn + "/moving_variance"], np.float64)
    assert np.allclose(after[bn + "/moving_variance"], 0.81 * mv0 + 0.19 * v * n_el / (n_el - 1), rtol=1e-12)
