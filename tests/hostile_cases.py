"""Hostile feature batches shared by tests/test_oracle_nonfinite.py (CPU) and tests/test_gpu_hostile_inputs.py (GPU).

Real feature files carry `nan`, `-nan`, `inf` and overflowed (`1e400` -> inf) tokens, and a client of the C ABI may pass any
int32 as a k-mer code. A batch here is the plain seeded batch of 70 sites (three 32-site m-tiles with max_batch = 128, the
last one ragged; several whole sites per fused tile from module 4 on, up to twelve at the short geometry) with FIVE hostile
sites planted at 0, 31, 32, 33 and 69: first / last row of an m-tile, neighbours inside one tile, the last row of the ragged
tail. Every other site is untouched, which is what the isolation tests lean on.

A case is (name, families, edit): `edit(f, i, T, S)` rewrites site i of the feature dict f in place. NaNs are written as bit
patterns through a uint32 view so that the sign and the payload arrive as stated (np.copysign(np.nan, -1) cast to float32 is
NAN_NEG; 0x7FFFFFFF / 0xFFFFFFFF have every mantissa bit set: a round-to-nearest-even bf16 conversion done by adding 0x7FFF
to the bits would carry out of the mantissa there).

DIRECTED cases are compared with the CPU statements (NaN mask and values). ISOLATION_ONLY cases are planted too but only
their neighbours are looked at: a single NaN sample is dropped or kept by a max-pool depending on the statement, so there
is no reference for the site itself.
"""
from __future__ import annotations

import numpy as np

from deepsignal_amd import synth

KEYS = ("kmer", "means", "stds", "sanums", "signals")
N = 70
MAX_BATCH = 128
HOSTILE_AT = (0, 31, 32, 33, 69)
SEED = 2024
GEOMETRIES = {"default": dict(), "short": dict(kmer_len=9, signal_len=100)}

NAN_POS, NAN_NEG, NAN_7F, NAN_FF = 0x7FC00000, 0xFFC00000, 0x7FFFFFFF, 0xFFFFFFFF
PINF, NINF = 0x7F800000, 0xFF800000
FAMILIES = ("signals", "features", "nan_forms", "signed_zero")


def _bits(a):
    return a.view(np.uint32)


def _sig(bits, where):
    """where(S) -> slice of the window"""
    def edit(f, i, T, S):
        _bits(f["signals"])[i, where(S)] = bits
    return edit


def _sig_value(value, where):
    def edit(f, i, T, S):
        f["signals"][i, where(S)] = value
    return edit


def _feat(key, bits, when):
    """when(T) -> the time step"""
    def edit(f, i, T, S):
        _bits(f[key])[i, when(T)] = bits
    return edit


def _feat_value(key, value, when):
    def edit(f, i, T, S):
        f[key][i, when(T)] = value
    return edit


def _zeros(value):
    def edit(f, i, T, S):
        f["kmer"][i, :] = 0                      # the two twins differ in the sign of their zeros and in nothing else
        for k in ("means", "stds", "sanums", "signals"):
            f[k][i, :] = value
    return edit


def _everything_nan(f, i, T, S):
    for k in ("means", "stds", "sanums", "signals"):
        _bits(f[k])[i, :] = NAN_POS


_all = lambda S: slice(0, S)
_start = lambda S: slice(0, 16)
_mid = lambda S: slice(S // 2 - 8, S // 2 + 8)
_end = lambda S: slice(S - 16, S)
_one = lambda S: slice(S // 2, S // 2 + 1)
_t0 = lambda T: 0
_tm = lambda T: T // 2
_tl = lambda T: T - 1

# The directed set, five cases per batch in the order of HOSTILE_AT. The features family is a Latin square over
# (means, stds, sanums) x (NaN, +inf, -inf) x (t = 0, T/2, T-1) plus one 1e30.
BATCHES = {
    "b0": [("sig_all_nan", ("signals", "nan_forms"), _sig(NAN_POS, _all)),
           ("means_nan_t0", ("features", "nan_forms"), _feat("means", NAN_POS, _t0)),
           ("sig_run_mid_neg_nan", ("nan_forms",), _sig(NAN_NEG, _mid)),
           ("sanums_pinf_t0", ("features",), _feat("sanums", PINF, _t0)),
           ("sig_one_1e30", ("signals",), _sig_value(np.float32(1e30), _one))],
    "b1": [("sig_run_start_nan", ("signals",), _sig(NAN_POS, _start)),
           ("means_pinf_mid", ("features",), _feat("means", PINF, _tm)),
           ("sig_run_mid_nan_7fffffff", ("nan_forms",), _sig(NAN_7F, _mid)),
           ("stds_ninf_t0", ("features",), _feat("stds", NINF, _t0)),
           ("sig_all_pinf", ("signals",), _sig(PINF, _all))],
    "b2": [("sig_run_mid_nan", ("signals",), _sig(NAN_POS, _mid)),
           ("stds_nan_mid", ("features",), _feat("stds", NAN_POS, _tm)),
           ("sig_run_mid_nan_ffffffff", ("nan_forms",), _sig(NAN_FF, _mid)),
           ("means_ninf_last", ("features",), _feat("means", NINF, _tl)),
           ("sig_one_minus_1e30", ("signals",), _sig_value(np.float32(-1e30), _one))],
    "b3": [("sig_run_end_nan", ("signals",), _sig(NAN_POS, _end)),
           ("sanums_nan_last", ("features",), _feat("sanums", NAN_POS, _tl)),
           ("sig_all_neg_nan", ("nan_forms",), _sig(NAN_NEG, _all)),
           ("stds_pinf_last", ("features",), _feat("stds", PINF, _tl)),
           ("means_1e30_mid", ("features",), _feat_value("means", np.float32(1e30), _tm))],
    "b4": [("zeros_negative", ("signed_zero",), _zeros(np.float32(-0.0))),
           ("zeros_positive", ("signed_zero",), _zeros(np.float32(0.0))),
           ("means_neg_nan_mid", ("nan_forms",), _feat("means", NAN_NEG, _tm)),
           ("stds_nan_ffffffff_last", ("nan_forms",), _feat("stds", NAN_FF, _tl)),
           ("sanums_ninf_mid", ("features",), _feat("sanums", NINF, _tm))],
    # isolation only: single samples (a max-pool may or may not drop them) and a site that is NaN in every input
    "iso": [("sig_single_nan_first", (), _sig(NAN_POS, lambda S: slice(0, 1))),
            ("sig_single_nan_mid", (), _sig(NAN_POS, _one)),
            ("everything_nan", (), _everything_nan),
            ("sig_single_neg_nan_odd", (), _sig(NAN_NEG, lambda S: slice(S // 2 + 1, S // 2 + 2))),
            ("sig_single_nan_last", (), _sig(NAN_POS, lambda S: slice(S - 1, S)))],
}

# Directed cases on which the CPU statements disagree (tests/test_oracle_nonfinite.py decides): name -> why. They stay in
# their batch, so their neighbours are still checked, but the site itself has no reference. Empty: the statements agree on
# every case above.
DROPPED = {
}

ISOLATION_ONLY = {c[0] for c in BATCHES["iso"]} | set(DROPPED)
DIRECTED_BATCHES = ("b0", "b1", "b2", "b3", "b4")
ZERO_TWINS = ("b4", HOSTILE_AT[0], HOSTILE_AT[1])        # (batch, the -0.0 site, its +0.0 twin)


def surviving_families():
    return {fam for b in DIRECTED_BATCHES for name, fams, _ in BATCHES[b] if name not in DROPPED for fam in fams}


def plain(geom: str):
    f = synth.synthetic_features(N, seed=SEED, **GEOMETRIES[geom])
    return {k: f[k] for k in KEYS}


def hostile(geom: str, batch: str):
    """The plain batch with the five cases of `batch` planted at HOSTILE_AT."""
    f = {k: v.copy() for k, v in plain(geom).items()}
    T, S = f["kmer"].shape[1], f["signals"].shape[1]
    for i, (_, _, edit) in zip(HOSTILE_AT, BATCHES[batch]):
        edit(f, i, T, S)
    return f


def directed_sites(batch: str):
    """Indices of `batch` whose outputs have a reference: everything but the isolation-only cases."""
    skip = {i for i, c in zip(HOSTILE_AT, BATCHES[batch]) if c[0] in ISOLATION_ONLY}
    return np.array([i for i in range(N) if i not in skip])


def case_names(batch: str):
    return dict(zip(HOSTILE_AT, (c[0] for c in BATCHES[batch])))


def only_hostile_sites(geom: str, batch: str):
    """The five hostile sites of a batch as a batch of their own (the CPU statements are per-site functions)."""
    f = hostile(geom, batch)
    return {k: v[list(HOSTILE_AT)] for k, v in f.items()}


def all_nan_batch(geom: str, n: int):
    """n sites that are NaN in every float input (stale-workspace test)."""
    g = GEOMETRIES[geom]
    T, S = g.get("kmer_len", 17), g.get("signal_len", 360)
    nan = lambda w: np.full((n, w), np.nan, np.float32)
    return {"kmer": np.zeros((n, T), np.int32), "means": nan(T), "stds": nan(T), "sanums": nan(T), "signals": nan(S)}


def compare_nonfinite(got, ref, atol=None, rtol=None):
    """None if `got` matches `ref` in the sense of the contract, else a message: equal NaN masks, equal infinities, finite
    entries within atol (absolute) or rtol * max(1, largest finite |ref| OF THE SAME SITE). A finite number in place of a NaN
    is the failure this whole file is about, so the mask comes first."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    if got.shape != ref.shape:
        return "shape %s != %s" % (got.shape, ref.shape)
    g2, r2 = got.reshape(got.shape[0], -1), ref.reshape(ref.shape[0], -1)
    gn, rn = np.isnan(g2), np.isnan(r2)
    if not np.array_equal(gn, rn):
        rows = np.nonzero((gn != rn).any(axis=1))[0]
        return "NaN masks differ at sites %s (finite where the reference is NaN: %d entries, NaN where it is finite: %d)" % (
            rows[:8].tolist(), int((rn & ~gn).sum()), int((gn & ~rn).sum()))
    gi, ri = np.isinf(g2), np.isinf(r2)
    if not (np.array_equal(gi, ri) and np.array_equal(g2[ri], r2[ri])):
        return "infinities differ at sites %s" % np.nonzero((gi != ri).any(axis=1) | ((g2 != r2) & ri).any(axis=1))[0][:8].tolist()
    fin = ~(rn | ri)
    d = np.where(fin, np.abs(np.where(fin, g2, 0.0) - np.where(fin, r2, 0.0)), 0.0)
    if atol is not None:
        tol = np.full(g2.shape[0], atol)
    else:
        tol = rtol * np.maximum(1.0, np.where(fin, np.abs(r2), 0.0).max(axis=1))
    bad = np.nonzero(d.max(axis=1) > tol)[0]
    if len(bad):
        return "sites %s off by %s (allowed %s)" % (bad[:8].tolist(), d.max(axis=1)[bad[:8]].tolist(), tol[bad[:8]].tolist())
    return None
