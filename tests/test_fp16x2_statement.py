"""The CPU statement of DS_PRECISION_FP16X2 (tests/fp16x2_statement.py): the term split does what the contract says, and the arithmetic
-- two fp16 terms, three products per MAC, no scaling -- is an fp32-class evaluation of the network on the three weight sets of the
parity tests, by the bars the GPU engines are held to (tests/test_gpu_stress.py; its constants are imported, not copied).

No GPU involved: this is the side of the comparison the GPU tests (tests/test_gpu_fp16x2.py) hold the engine to.
Measured when the statement was written (n = 130, max |d act| to float64: fp16x2 / fp32 oracle): small 4.2e-7 / 8.1e-7,
balanced 3.0e-5 / 3.0e-5, stress 2.3e-5 / 3.6e-5.
"""
import numpy as np
import pytest
import torch

from deepsignal_amd import synth
from test_gpu_stress import FLOOR_REL, LABEL_MARGIN, NOISE_FACTOR, OUT_ATOL, _fp32_noise

import fp16x2_statement as st

N_SITES = 130


def _sum(x, **kw):
    h0, h1 = st.split_terms_fp16(torch.from_numpy(x), **kw)
    return h0.numpy(), h1.numpy()


def test_two_terms_hold_any_value_of_22_significant_bits_exactly():
    rng = np.random.default_rng(11)
    # 22-bit significands at exponents from 2^-3 (below: h1 runs out of fp16's subnormal range) to just under 2^16
    m = rng.integers(1 << 21, 1 << 22, size=200_000).astype(np.float64)
    e = rng.integers(-3 - 21, 15 - 21 + 1, size=m.size)
    x = (m * np.exp2(e) * rng.choice([-1.0, 1.0], size=m.size)).astype(np.float32)
    assert np.array_equal(x.astype(np.float64), m * np.exp2(e) * np.sign(x))      # (the values are fp32 numbers)
    x = x[np.abs(x) <= st.FP16_MAX]
    h0, h1 = _sum(x)
    assert np.array_equal(h0.astype(np.float64) + h1.astype(np.float64), x.astype(np.float64))
    # every term is an fp16 number
    for t in (h0, h1):
        assert np.array_equal(t.astype(np.float16).astype(np.float32), t)


def test_two_terms_are_within_2_to_the_minus_22_of_any_fp32_value_in_range():
    rng = np.random.default_rng(12)
    x = np.exp2(rng.uniform(-3.0, np.log2(st.FP16_MAX), size=400_000)).astype(np.float32) * rng.choice([-1.0, 1.0], size=400_000).astype(np.float32)
    x = np.concatenate([x, np.float32([0.125, -0.125, st.FP16_MAX, -st.FP16_MAX, 1.0, 0.1, 18.8])])
    h0, h1 = _sum(x)
    rel = np.abs(h0.astype(np.float64) + h1.astype(np.float64) - x.astype(np.float64)) / np.abs(x.astype(np.float64))
    assert rel.max() <= 2.0 ** -22, rel.max()
    # subnormal second terms are kept: below |x| = 0.125 ... 2^-3 x 2^-11 = 2^-14 is where h1 leaves the normal range
    small = np.float32([0.1, 0.01, 0.001])
    assert (np.abs(_sum(small)[1]) > 0).all() and (np.abs(_sum(small)[1]) < st.FP16_MIN_NORMAL).all()
    assert (_sum(small, flush=True)[1] == 0).all()


def test_a_value_beyond_the_fp16_range_becomes_inf_and_its_product_nan():
    x = np.float32([65520.0, 1e5, -7e4, 3.4e38, 65519.0])
    h0, h1 = _sum(x)
    assert np.array_equal(h0[:4], np.float32([np.inf, np.inf, -np.inf, np.inf])) and np.array_equal(h1[:4], -h0[:4])
    assert h0[4] == 65504.0 and h1[4] == 15.0           # the largest value that still rounds to a finite h0: exact in two terms
    a = torch.tensor([[1e5, 1.0]], dtype=torch.float32)
    with st.fp16_terms():
        from oracle import torch_statement
        y = torch_statement._split_matmul(a, torch.ones(2, 1), 2, torch.float32)
    assert torch.isnan(y).all()
    # ... and the bf16 split is back
    assert torch_statement.split_terms(torch.tensor([1.0 + 2.0 ** -9]), 1)[0].item() == 1.0


@pytest.mark.parametrize("which", ["small", "balanced", "stress"])
def test_the_statement_is_an_fp32_class_evaluation(request, which):
    from oracle import oracle
    w = request.getfixturevalue(which + "_weights")
    noise = _fp32_noise(which, w)
    feats = synth.synthetic_features(N_SITES, seed=900 + N_SITES)
    a32, p32, t32 = oracle.forward(w, feats, "f32", taps=True)
    a64, p64, t64 = oracle.forward(w, feats, "f64", taps=True)
    act, pred, taps = st.forward_fp16x2(w, feats, return_taps=True)
    assert np.isfinite(act).all()
    bad = {}
    for name, ref in t64.items():
        if name not in taps:
            continue
        scale = max(1.0, float(np.abs(ref).max()))
        e_st = float(np.abs(taps[name].reshape(ref.shape) - ref).max())
        e_o32 = float(np.abs(t32[name] - ref).max())
        tol = NOISE_FACTOR * max(e_o32, noise[name]) + FLOOR_REL * scale
        if not e_st <= tol:
            bad[name] = (e_st, tol)
    d_act, d_o32 = float(np.abs(act - a64).max()), float(np.abs(a32 - a64).max())
    print("\n%s n=%d: fp16x2 statement vs f64 |d act| %.2e   (fp32 oracle vs f64: %.2e)" % (which, N_SITES, d_act, d_o32))
    assert not bad, "taps further from float64 than %gx the fp32 oracle: %s" % (NOISE_FACTOR, bad)
    assert d_act <= OUT_ATOL
    assert d_act <= 1.5 * d_o32, (d_act, d_o32)
    decided = np.abs(a64[:, 1] - a64[:, 0]) > LABEL_MARGIN
    assert (pred[decided] == p64[decided]).all()


def test_the_variant_path_is_the_arithmetic_of_forward_split(small_weights):
    """forward_fp16x2 runs forward_split for the full model and its own walk of the same helpers for the model variants: on the full model
    the two give the same bits."""
    feats = synth.synthetic_features(9, seed=5)
    a, p, taps = st.forward_fp16x2(small_weights, feats, return_taps=True)
    with st.fp16_terms():
        b, q, tv = st._forward_variant(small_weights, feats, st.FP16X2_SCOPE, torch.float32, True, True, True, True)
    assert np.array_equal(a, b) and np.array_equal(p, q)
    assert set(taps) == set(tv) and all(np.array_equal(taps[k], tv[k]) for k in taps)
