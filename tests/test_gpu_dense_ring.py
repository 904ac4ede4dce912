"""GPU: the fp32 dense(J, J) layer of the three-step joint model at batches that are a multiple of 128 -- the instantiation whose
weights come through an LDS ring (dense_ring_loop, ds_kernels.hip) -- against the untouched masked instantiation (CFG_FC, every
other batch size), against the fp32 oracle, and under co-running kernels.

The ring has four stages and the loop is unrolled by four with one exit behind every step, so the step a workgroup leaves from is
the chunk count modulo 4 (chunk = 16 k). The shipped geometry gives J = 6032 (377 chunks, residue 1), the variants without the
signal / event model J = 512 (32 chunks -- shorter than eight ring trips -- residue 0) and J = 5520 (345, residue 1); signal
lengths 344 (J = 5792, 362 chunks, residue 2) and 200 (J = 3632, 227 chunks, residue 3) add the exits those leave out.
Tolerances are tests/test_gpu_parity.py's; the bitwise checks have none."""
import numpy as np
import pytest

from deepsignal_amd import spec, synth

pytestmark = pytest.mark.gpu

INTERMEDIATE_RTOL = 2e-5      # tests/test_gpu_parity.py
ACT_ATOL = 1e-5
KEYS = ("kmer", "means", "stds", "sanums", "signals")


def _engine(weights, **kw):
    from deepsignal_amd.engine import Engine
    eng = Engine(**kw)
    eng.load_weights(weights)
    return eng


@pytest.mark.parametrize("n", [128, 256])
def test_fc1_bits_do_not_depend_on_the_instantiation(stress_weights, n):
    """fc1 of n sites (n % 128 == 0: the ring loop) equals, bit for bit, fc1 of the same sites inside a batch of n + 2 (the masked
    instantiation with the generic loop): the ring keeps every accumulator's k order."""
    J = spec.net_dims().joint
    feats = synth.synthetic_features(n + 2, seed=300 + n)
    eng = _engine(stress_weights, max_batch=n + 2, debug=True, slots=1, fold_fc=False)
    act_d, pred_d = eng.run(*(feats[k][:n] for k in KEYS))
    fc1_d = eng.intermediate("fc1", (n, J))
    act_m, pred_m = eng.run(*(feats[k] for k in KEYS))
    fc1_m = eng.intermediate("fc1", (n + 2, J))
    eng.close()
    assert np.isfinite(fc1_m).all() and float(np.abs(fc1_m).max()) > 0
    diff = fc1_d.view(np.uint32) != fc1_m[:n].view(np.uint32)
    print("n = %d: %d of %d fc1 values differ in their bits" % (n, int(diff.sum()), diff.size))
    assert not diff.any(), np.argwhere(diff)[:8]
    assert np.array_equal(act_d, act_m[:n]) and np.array_equal(pred_d, pred_m[:n])


@pytest.mark.parametrize("variant", [dict(), dict(is_cnn=False), dict(is_rnn=False), dict(signal_len=344), dict(signal_len=200)],
                         ids=["J6032_r1", "J512_r0", "J5520_r1", "J5792_r2", "J3632_r3"])
def test_three_step_model_at_128_sites_matches_the_oracle(variant):
    from deepsignal_amd import weights as W
    from oracle import oracle
    n = 128
    geom = {k: v for k, v in variant.items() if k == "signal_len"}
    dims = spec.net_dims(**variant)
    assert (dims.joint // 16) % 4 == {6032: 1, 512: 0, 5520: 1, 5792: 2, 3632: 3}[dims.joint]
    w = W.random_weights(seed=21, lstm_bias_std=0.1, **variant)
    feats = synth.synthetic_features(n, seed=77, **geom)
    eng = _engine(w, max_batch=n, debug=True, slots=1, fold_fc=False, **variant)
    act, pred = eng.run(*(feats[k] for k in KEYS))
    fc1 = eng.intermediate("fc1", (n, dims.joint))
    eng.close()
    o_act, o_pred, taps = oracle.forward(w, feats, "f32", taps=True, **variant)
    assert "fc1" in taps and taps["fc1"].shape == fc1.shape
    err, tol = float(np.abs(fc1 - taps["fc1"]).max()), INTERMEDIATE_RTOL * max(1.0, float(np.abs(taps["fc1"]).max()))
    print("J = %d: fc1 max error %.3g (bar %.3g), act max error %.3g" % (dims.joint, err, tol, float(np.abs(act - o_act).max())))
    assert err <= tol
    assert np.isfinite(act).all() and np.abs(act - o_act).max() <= ACT_ATOL
    norm = lambda a: a / a.sum(axis=1, keepdims=True)
    assert np.abs(norm(act) - norm(o_act)).max() <= ACT_ATOL
    decided = np.abs(o_act[:, 1] - o_act[:, 0]) > 1e-3
    assert (pred[decided] == o_pred[decided]).all()


def test_eight_slots_in_flight_match_one_slot(stress_weights):
    """64 forwards of 128 sites through eight slots: the dense workgroups run beside other forwards' chain, cell and stem
    kernels (and share CUs with them); every forward must give the bits of the one-slot engine."""
    n, nbatch, nfwd = 128, 4, 64
    feats = synth.synthetic_features(n * nbatch, seed=41)
    part = lambda j: [feats[k][j * n:(j + 1) * n] for k in KEYS]
    one = _engine(stress_weights, max_batch=n, slots=1, fold_fc=False)
    ref = [one.run(*part(j)) for j in range(nbatch)]
    one.close()
    eng = _engine(stress_weights, max_batch=n, slots=8, fold_fc=False)
    tickets, bad = [], []
    for i in range(nfwd + 8):
        if i >= 8:
            act, pred = eng.wait(tickets[i - 8])
            r = ref[(i - 8) % nbatch]
            if not (np.array_equal(act, r[0]) and np.array_equal(pred, r[1])):
                bad.append(i - 8)
        if i < nfwd:
            tickets.append(eng.submit(*part(i % nbatch)))
    eng.close()
    assert not bad, "forwards that differ from the one-slot run: %s" % bad
