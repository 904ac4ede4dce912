"""GPU: the native fp32 fused inception kernel's 48-channel branches, range by range.

The kernel computes channels 0..31 of b3b / b4b on 32x32x2 MFMA tiles and channels 32..47 on 16x16x4 tiles, from a weight
image of their own (ds_engine.cpp pack_b_rem16). Every module output is compared per channel range -- 0..47 (b1), 96..143
(b3b), 144..191 (b4b) -- against the layer-granular path (DS_TUNE_NO_FUSED: gemm_kernel, which shares no code with the
fused kernel) and against the fp32 oracle, so a wrong remainder image shows up as channels 32..47 of its range and not as a
diluted maximum over 240 channels. The bars are the per-tensor bars of the fused-vs-oracle parity test (test_gpu_parity),
imported, not copied.

Sizes at signal_len 360 (module widths 90, 45, 23 rows per site; fuse_min_tiles=1 lets a small batch tile as a big one does):
  n = 1   a tile of one site at every width (all three instantiations: 3, 2 and 1 m-tiles)
  n = 5   W = 45: two sites per tile, the last tile ragged (one site: its other rows go through the dump row)
  n = 9   the same with five tiles
  n = 13  W = 23: four sites per tile (92 of 96 rows), the last tile holds one site of four; W = 45 ragged as well
          (at n = 5 and 9 the planner's rule -- fewest padded rows -- keeps W = 23 at one site per tile)
One case runs the stress weights: hot BN channels and large biases exercise the bias-as-initial-accumulator path."""
import numpy as np
import pytest

from deepsignal_amd import spec, synth
from test_gpu_parity import ACT_ATOL, INTERMEDIATE_RTOL

pytestmark = pytest.mark.gpu

KEYS = ("kmer", "means", "stds", "sanums", "signals")
RANGES = {"b1": (0, 48), "b3b": (96, 144), "b4b": (144, 192)}


def _engine(weights, **kw):
    from deepsignal_amd.engine import Engine
    eng = Engine(**kw)
    eng.load_weights(weights)
    return eng


def _modules(eng, n):
    d = spec.net_dims()
    return {"module%d" % m: eng.intermediate("module%d" % m, (n, d.module_width(m), 240)) for m in range(1, 12)}


def _compare(got, ref, label):
    """per module and channel range against the tensor's bar; the remainder channels are reported on their own"""
    bad, worst = {}, (0.0, None)
    for name in ref:
        tol = INTERMEDIATE_RTOL * max(1.0, float(np.abs(ref[name]).max()))
        parts = dict(RANGES)
        parts.update({k + "[32:48]": (lo + 32, hi) for k, (lo, hi) in RANGES.items()})
        parts["all"] = (0, 240)
        for part, (lo, hi) in parts.items():
            err = float(np.abs(got[name][..., lo:hi] - ref[name][..., lo:hi]).max())
            if err / tol > worst[0]:
                worst = (err / tol, "%s %s |d| %.2e" % (name, part, err))
            if not err <= tol:
                bad["%s %s" % (name, part)] = (err, tol)
    print("\n%s: worst %s = %.3f of its bar" % (label, worst[1], worst[0]))
    assert not bad, "%s: out of tolerance: %s" % (label, bad)


def _run_case(weights, n, seed):
    from oracle import oracle
    feats = synth.synthetic_features(n, seed=seed, signal_len=360)
    args = [feats[k] for k in KEYS]
    outs = {}
    for no_fused in (False, True):
        eng = _engine(weights, max_batch=64, debug=True, slots=1, precision="fp32", no_fused=no_fused, fuse_min_tiles=1)
        act, pred = eng.run(*args)
        outs[no_fused] = (act, _modules(eng, n))
        eng.close()
    o_act, o_pred, taps = oracle.forward(weights, feats, "f32", taps=True)
    o_mod = {k: v for k, v in taps.items() if k.startswith("module")}
    assert len(o_mod) == 11
    return outs[False], outs[True], (o_act, o_mod)


@pytest.mark.parametrize("n", [1, 5, 9, 13])
def test_fused_module_channel_ranges(small_weights, n):
    (f_act, f_mod), (u_act, u_mod), (o_act, o_mod) = _run_case(small_weights, n, 2100 + n)
    assert all(np.isfinite(v).all() for v in f_mod.values())
    _compare(f_mod, u_mod, "n=%d fused vs layer-granular" % n)
    _compare(f_mod, o_mod, "n=%d fused vs fp32 oracle" % n)
    assert np.abs(f_act - o_act).max() <= ACT_ATOL and np.abs(f_act - u_act).max() <= ACT_ATOL


def test_fused_module_channel_ranges_with_stress_weights(stress_weights):
    n = 9
    (f_act, f_mod), (u_act, u_mod), (o_act, o_mod) = _run_case(stress_weights, n, 2200)
    assert all(np.isfinite(v).all() for v in f_mod.values())
    _compare(f_mod, u_mod, "stress n=%d fused vs layer-granular" % n)
    _compare(f_mod, o_mod, "stress n=%d fused vs fp32 oracle" % n)
