"""CPU (-m "not gpu"): the three CPU statements of the forward on NON-FINITE and extreme inputs (tests/hostile_cases.py).

tests/test_gpu_hostile_inputs.py holds the HIP engine to `oracle.forward(..., "f32")` and `torch_statement.forward_bf16` on
these cases, so the references are pinned to each other here first: the C oracle (float32 and float64), torch_statement
(functional ops) and nn_statement (library modules) must put their NaNs in the same places -- in `act` and in every tap they
share -- and agree on the finite entries within the bars of tests/test_oracle.py; `forward_bf16` (both BiLSTM forms) must
put the NaNs of `act` where the float64 oracle does (float64 statements: 1e-7 on `act`, 1e-6 of
the tensor's scale on a tap; float32 oracle: 2e-6 on `act`). The library semantics are the reference: ReLU and max-pool
propagate NaN (torch.relu, F.max_pool1d), and argmax takes the first NaN.

A case on which they do not agree has no reference and is listed in hostile_cases.DROPPED with the reason; at least one case
of every family must survive, and no finite result of the committed goldens may have moved.
"""
import os

import numpy as np
import pytest
import torch

import hostile_cases as hc
from deepsignal_amd import weights
from oracle import nn_statement, oracle, torch_statement

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def geom_weights(small_weights):
    return {"default": small_weights,
            "short": weights.random_weights(seed=33, lstm_bias_std=0.1, **hc.GEOMETRIES["short"])}


def _disagreements(w, feats, geom):
    """{site row: [messages]} over the hostile sites of one batch."""
    g = hc.GEOMETRIES[geom]
    o64 = oracle.forward(w, feats, "f64", taps=True, **g)
    o32 = oracle.forward(w, feats, "f32", taps=True, **g)
    ts = torch_statement.forward(w, feats, torch.float64, True)
    nn = nn_statement.forward(w, feats, torch.float64, True)
    bf = {flag: torch_statement.forward_bf16(w, feats, lstm_bf16=flag) for flag in (False, True)}
    assert set(ts[2]) == set(o64[2]) and set(nn[2]) <= set(o64[2])
    out = {}

    def note(row, msg):
        out.setdefault(row, []).append(msg)

    for row in range(len(hc.HOSTILE_AT)):
        one = lambda a: a[row:row + 1]
        for tag, other in (("torch_statement", ts), ("nn_statement", nn)):
            m = hc.compare_nonfinite(one(other[0]), one(o64[0]), atol=1e-7)
            if m:
                note(row, "%s act: %s" % (tag, m))
            if not np.array_equal(one(other[1]), one(o64[1])):
                note(row, "%s pred %s != %s" % (tag, one(other[1]), one(o64[1])))
            for k, v in other[2].items():
                m = hc.compare_nonfinite(one(v), one(o64[2][k]), rtol=1e-6)
                if m:
                    note(row, "%s %s: %s" % (tag, k, m))
        m = hc.compare_nonfinite(one(o32[0]), one(o64[0]), atol=2e-6)
        if m:
            note(row, "oracle f32 act: %s" % m)
        for k, v in o32[2].items():
            if not np.array_equal(np.isnan(one(v)), np.isnan(one(o64[2][k]))):
                note(row, "oracle f32 %s: NaN mask differs from f64" % k)
        # the reference of the bf16 modes: it rounds where the engine rounds, so its finite values are its own, but its NaNs
        # must sit where the float64 oracle's do (a bf16 rounding neither makes nor loses a NaN; the 1e30 cases stay finite)
        for lstm_bf16 in (False, True):
            if not np.array_equal(np.isnan(one(bf[lstm_bf16][0])), np.isnan(one(o64[0]))):
                note(row, "forward_bf16(lstm_bf16=%s) act: NaN mask differs from the f64 oracle" % lstm_bf16)
            if not np.isfinite(one(bf[lstm_bf16][0])[~np.isnan(one(o64[0]))]).all():
                note(row, "forward_bf16(lstm_bf16=%s) act: infinite where the f64 oracle is finite" % lstm_bf16)
    return out, o64


@pytest.mark.parametrize("geom", list(hc.GEOMETRIES))
@pytest.mark.parametrize("batch", hc.DIRECTED_BATCHES)
def test_statements_agree_on_nan_masks_and_finite_values(geom_weights, geom, batch):
    feats = hc.only_hostile_sites(geom, batch)
    bad, o64 = _disagreements(geom_weights[geom], feats, geom)
    names = [c[0] for c in hc.BATCHES[batch]]
    live = {names[r]: msgs for r, msgs in bad.items() if names[r] not in hc.DROPPED}
    assert not live, live
    act = o64[0]
    for r, n in enumerate(names):
        if n.startswith("zeros_") or "pinf" in n or "ninf" in n or "1e30" in n:
            continue
        assert np.isnan(act[r]).all(), "%s: a NaN input must reach both outputs of the reference, got %s" % (n, act[r])


def test_every_family_keeps_a_directed_case():
    assert hc.surviving_families() == set(hc.FAMILIES)
    for b in hc.BATCHES.values():
        assert len(b) == len(hc.HOSTILE_AT)
    assert set(hc.DROPPED) <= {c[0] for b in hc.DIRECTED_BATCHES for c in hc.BATCHES[b]}


def test_what_the_reference_makes_of_infinities_and_huge_values(geom_weights):
    """The directed cases are only worth their place if the reference is FINITE on some of them (an Inf on an LSTM feature
    saturates the gates; 1e30 is a number) and NaN on others (an all-Inf window meets weights of both signs)."""
    w = geom_weights["default"]
    finite, nan = [], []
    for batch in hc.DIRECTED_BATCHES:
        act, _ = oracle.forward(w, hc.only_hostile_sites("default", batch), "f32")
        for r, c in enumerate(hc.BATCHES[batch]):
            (finite if np.isfinite(act[r]).all() else nan).append(c[0])
    print("finite in the reference:", finite, "\nNaN in the reference:", nan)
    for n in ("sanums_pinf_t0", "means_pinf_mid", "stds_ninf_t0", "means_ninf_last", "stds_pinf_last", "sanums_ninf_mid",
              "means_1e30_mid", "zeros_negative", "zeros_positive"):
        assert n in finite, n
    assert "sig_all_pinf" in nan


def test_signed_zero_twins_agree(geom_weights):
    batch, neg, pos = hc.ZERO_TWINS
    r_neg, r_pos = hc.HOSTILE_AT.index(neg), hc.HOSTILE_AT.index(pos)
    for geom in hc.GEOMETRIES:
        feats = hc.only_hostile_sites(geom, batch)
        assert np.signbit(feats["signals"][r_neg]).all() and not np.signbit(feats["signals"][r_pos]).any()
        a64, p64 = oracle.forward(geom_weights[geom], feats, "f64", **hc.GEOMETRIES[geom])
        assert np.abs(a64[r_neg] - a64[r_pos]).max() < 1e-7 and p64[r_neg] == p64[r_pos]


def test_goldens_replay_bit_for_bit():
    """Making the C oracle NaN-honest (ReLU of the residual branch, max-pools, argmax) may not move a finite result."""
    g = np.load(os.path.join(GOLDEN, "forward_golden.npz"))
    w = weights.random_weights(seed=int(g["weight_seed"]), lstm_bias_std=float(g["lstm_bias_std"]))
    feats = {k[3:]: g[k] for k in g.files if k.startswith("in_")}
    act, pred, taps = oracle.forward(w, feats, "f64", taps=True)
    assert np.array_equal(act, g["act"]) and np.array_equal(pred, g["pred"])
    assert np.array_equal(taps["logits"], g["logits"]) and np.array_equal(taps["module11"], g["module11"])
    s = np.load(os.path.join(GOLDEN, "stress_golden.npz"))
    ws = weights.stress_weights(int(s["stress_seed"]), head=s["stress_head"])
    feats = {k: s["in_" + k] for k in hc.KEYS}
    act, pred, taps = oracle.forward(ws, feats, "f64", taps=True)
    assert np.abs(act - s["act"]).max() < 1e-9 and np.array_equal(pred, s["pred"])
    assert np.abs(taps["logits"] - s["logits"]).max() < 1e-6
