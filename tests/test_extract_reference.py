"""CPU: the arithmetic of the device feature extraction (ds_extract.h, run on the host by ds_extract_reference) against the host
extractor (deepsignal_amd/extract_features.py, itself pinned to the reference by tests/test_extract_features.py), bit for bit
after the float32 narrowing the engine's inputs get."""
import json
import os

import numpy as np
import pytest

from deepsignal_amd import extract_features as ef
from deepsignal_amd import synth
from deepsignal_amd.engine import ReadBatch, base_codes, extract_reference

import extract_cases as xc

GOLD = os.path.join(os.path.dirname(__file__), "golden", "extract_golden.json")


def _np_pairwise(x):
    """numpy's pairwise_sum as the issue states it (the model ds_extract.h implements)."""
    n = len(x)
    if n < 8:
        res = 0.0
        for v in x:
            res += v
        return res
    if n <= 128:
        r = list(x[:8])
        i = 8
        while i < n - (n % 8):
            for j in range(8):
                r[j] += x[i + j]
            i += 8
        res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]))
        for k in range(i, n):
            res += x[k]
        return res
    n2 = n // 2
    n2 -= n2 % 8
    return _np_pairwise(x[:n2]) + _np_pairwise(x[n2:])


def _np_sum_model(x):
    s = 0.0
    for b in range(0, len(x), 8192):
        s += _np_pairwise(x[b:b + 8192])
    return s


@pytest.mark.parametrize("n", list(range(1, 301, 7)) + [8191, 8192, 8193, 50000, 300000])
def test_summation_model_matches_numpy(n):
    x = np.random.default_rng(n).normal(3.0, 40.0, n)
    xs = [float(v) for v in x]
    m = _np_sum_model(xs) / n
    assert m == float(np.mean(x))
    d = [(v - m) * (v - m) for v in xs]
    assert np.sqrt(_np_sum_model(d) / n) == float(np.std(x))


@pytest.mark.parametrize("n", [1, 2, 3, 10, 11, 255, 256, 8193, 50000])
def test_around_is_rint_scaled(n):
    x = np.random.default_rng(n).normal(0, 3, n)
    assert np.array_equal(np.around(x, 6), np.rint(x * 1e6) / 1e6)


def _sites(bases, motif_seqs, kmer_len, methyloc=0):
    return [loc for loc, _, _ in ef.read_sites(bases, motif_seqs, methyloc, kmer_len, "+", "c", 0, None)]


def _host_features(raw, starts, lengths, bases, scaling, offset, motif_seqs, kmer_len, signal_len, norm):
    feats = ef.extract_read_features(raw, starts, lengths, bases, scaling, offset, "r", "t", "+", "c", 0, None, motif_seqs, 0,
                                     kmer_len, signal_len, 1, norm)
    return {"kmer": np.array([[ "ACGTN".index(b) for b in f[6]] for f in feats], np.int32).reshape(-1, kmer_len),
            "means": np.array([f[7] for f in feats], np.float32).reshape(-1, kmer_len),
            "stds": np.array([f[8] for f in feats], np.float32).reshape(-1, kmer_len),
            "sanums": np.array([f[9] for f in feats], np.float32).reshape(-1, kmer_len),
            "signals": np.array([np.asarray(f[10], np.float64) for f in feats], np.float32).reshape(-1, signal_len)}


def _same_bits(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint32) if a.dtype == np.float32 else a,
                                                 b.view(np.uint32) if b.dtype == np.float32 else b)


def _check_read(raw, starts, lengths, bases, scaling, offset, motif_seqs, kmer_len, signal_len, norm):
    locs = _sites(bases, motif_seqs, kmer_len)
    if not locs:
        return 0
    host = _host_features(raw, starts, lengths, bases, scaling, offset, motif_seqs, kmer_len, signal_len, norm)
    batch = ReadBatch([(raw, starts, lengths, base_codes(bases), scaling, offset)], [0] * len(locs), locs, norm=norm)
    dev = extract_reference(batch, kmer_len, signal_len)
    sub = np.array([lengths[loc] >= signal_len for loc in locs])      # subsample branch: checked separately
    for k in ("kmer", "means", "stds", "sanums"):
        assert _same_bits(dev[k], host[k]), k
    assert _same_bits(dev["signals"][~sub], host["signals"][~sub])
    return len(locs)


@pytest.fixture(scope="module")
def gold():
    with open(GOLD) as f:
        return json.load(f)


@pytest.mark.parametrize("idx", [0, 1, 2, 3])
def test_golden_cases_bit_identical(gold, idx):
    case = gold["cases"][idx]
    n = 0
    for name in gold["read_order"]:
        r = gold["reads"][name]
        bases = r["bases"]          # the site list depends on the bases only; the strand changes pos, not the features
        n += _check_read(np.asarray(r["signal"], np.int16), np.asarray(r["starts"], np.int64), np.asarray(r["lengths"], np.int64),
                         bases, r["range"] / r["digitisation"], r["offset"], case["motif_seqs"], case["kmer_len"],
                         case["signal_len"], case["normalize_method"])
    assert n > 0


@pytest.mark.parametrize("norm", ["mad", "zscore"])
@pytest.mark.parametrize("seed,nbases", [(1, 900), (2, 1201), (3, 3000), (4, 40)])
def test_synthetic_reads_bit_identical(norm, seed, nbases):
    raw, starts, lengths, bases, scaling, offset = synth.synthetic_read(nbases, seed)
    # sites at both read ends: force CG right at the first / last usable positions
    b = list(bases)
    b[8:10] = "CG"
    b[nbases - 10:nbases - 8] = "CG"
    bases = "".join(b)
    assert _check_read(raw, starts, lengths, bases, scaling, offset, ["CG"], 17, 360, norm) > 0
    if seed == 3:
        assert len(raw) > 8192      # z-score sums over more than one numpy block
    # a short window: zero-padded
    assert _check_read(raw, starts, lengths, bases, scaling, offset, ["CG"], 9, 100, norm) > 0


def test_odd_and_even_lengths_mad():
    for extra in (0, 1):
        raw, starts, lengths, bases, scaling, offset = synth.synthetic_read(500, 11 + extra)
        raw = raw[:len(raw) - ((len(raw) + extra) % 2)]      # one even, one odd sample count
        keep = starts + lengths <= len(raw)
        n = int(np.argmin(keep)) if not keep.all() else len(starts)
        assert _check_read(raw, starts[:n], lengths[:n], bases[:n], scaling, offset, ["CG"], 17, 360, "mad")


@pytest.mark.parametrize("norm_method", ["mad", "zscore"])
@pytest.mark.parametrize("n", list(range(2, 301, 3)) + [8191, 8192, 8193, 50000, 300000])
def test_read_statistics_match_normalize(n, norm_method):
    """The read statistics -- median / MAD by selection on the int16 histogram, mean / std in numpy's summation order --
    reproduce _normalize_signals bit for bit, also for reads with a wide value range (spread 20000: more histogram bins than
    the kernel keeps in LDS) and many ties (spread 3)."""
    rng = np.random.default_rng(n)
    for spread in (3, 300, 20000):
        raw = rng.integers(-spread, spread + 1, n).astype(np.int16)
        starts = np.array([0], np.int64)
        lengths = np.array([n], np.int64)
        norm = ef._normalize_signals(ef._rescale_signals(raw, 0.17, 12.0), norm_method)
        # one 1-mer site over the whole read; a window one sample longer than the read holds every normalised sample
        batch = ReadBatch([(raw, starts, lengths, base_codes("C"), 0.17, 12.0)], [0], [0], norm=norm_method)
        dev = extract_reference(batch, 1, n + 1)
        assert np.array_equal(dev["signals"][0, :n].view(np.uint32), norm.astype(np.float32).view(np.uint32))


def test_subsample_branch_is_ordered_and_seeded():
    raw, starts, lengths, bases, scaling, offset = synth.synthetic_read(300, 21, long_bases=20)
    locs = [i for i in range(8, 292) if lengths[i] >= 360]
    assert locs
    batch = ReadBatch([(raw, starts, lengths, base_codes(bases), scaling, offset)], [0] * len(locs), locs, seed=7)
    a = extract_reference(batch)
    b = extract_reference(ReadBatch([(raw, starts, lengths, base_codes(bases), scaling, offset)], [0] * len(locs), locs, seed=7))
    c = extract_reference(ReadBatch([(raw, starts, lengths, base_codes(bases), scaling, offset)], [0] * len(locs), locs, seed=8))
    assert np.array_equal(a["signals"], b["signals"]) and not np.array_equal(a["signals"], c["signals"])
    norm = ef._normalize_signals(ef._rescale_signals(raw, scaling, offset), "mad").astype(np.float32)
    for i, loc in enumerate(locs):
        mid = norm[starts[loc]:starts[loc] + lengths[loc]]
        # every window value is one of the middle base's samples, taken at strictly increasing indices
        idx, pos = [], 0
        for v in a["signals"][i]:
            while mid[pos] != v:
                pos += 1
            idx.append(pos)
            pos += 1
        assert len(idx) == 360 and all(np.diff(idx) > 0)


def _valid():
    raw, starts, lengths, bases, scaling, offset = synth.synthetic_read(100, 3)
    return [raw, starts, lengths, base_codes(bases), scaling, offset]


@pytest.mark.parametrize("what", ["loc_low", "loc_high", "past_read", "negative_start", "bad_code", "bad_read", "nsites0",
                                  "offsets"])
def test_invalid_inputs_rejected(what):
    r = _valid()
    site_read, site_loc = [0], [20]
    if what == "loc_low":
        site_loc = [7]
    elif what == "loc_high":
        site_loc = [100 - 8]
    elif what == "past_read":
        r[2] = r[2].copy(); r[2][-1] += len(r[0])
    elif what == "negative_start":
        r[1] = r[1].copy(); r[1][3] = -1
    elif what == "bad_code":
        r[3] = r[3].copy(); r[3][5] = 5
    elif what == "bad_read":
        site_read = [1]
    elif what == "nsites0":
        site_read, site_loc = [], []
    batch = ReadBatch([tuple(r)], site_read, site_loc)
    if what == "offsets":
        batch.base_off[1] -= 1          # base offsets that do not cover the bases given
        batch.raw_off[0] = 1
    with pytest.raises(RuntimeError, match="ds_reads"):
        extract_reference(batch)


# ---- the shared case table (tests/extract_cases.py): the inputs tests/test_gpu_extract.py runs the kernels on ------------
def test_case_table_covers_every_code_path():
    """Every case takes the paths it is listed for, and the table as a whole takes every path of ds_extract.hip that
    extract_cases.derive_paths distinguishes: the table may not shrink to cases that miss a branch."""
    union = set()
    for c in xc.CASES:
        got = c.derived()
        assert c.paths <= got, (c.name, sorted(c.paths - got))
        union |= got
    assert union == xc.ALL_PATHS, (sorted(xc.ALL_PATHS - union), sorted(union - xc.ALL_PATHS))


def _host_step(step):
    """The host extractor's features of a step's sites, in the step's site order, and the mask of SUB windows."""
    reads, site_read, site_loc, norm, T, S, _ = step
    per_read = {}
    for i, r in enumerate(reads):
        locs = sorted(int(loc) for rd, loc in zip(site_read, site_loc) if rd == i)
        if not locs:
            continue
        bases = "".join("ACGTN"[c] for c in r[3])
        assert _sites(bases, ["CG"], T) == locs
        with np.errstate(all="ignore"):
            per_read[i] = (locs, _host_features(r[0], r[1], r[2], bases, r[4], r[5], ["CG"], T, S, norm))
    rows = [(per_read[int(rd)][1], per_read[int(rd)][0].index(int(loc))) for rd, loc in zip(site_read, site_loc)]
    host = {k: np.stack([h[k][j] for h, j in rows]) for k in xc.KEYS}
    sub = np.array([reads[rd][2][loc] >= S for rd, loc in zip(site_read, site_loc)])
    return host, sub


@pytest.mark.parametrize("name,norm", xc.case_norm_params())
def test_case_table_bit_identical_to_host(name, norm):
    """ds_extract_reference == the numpy host extractor on every step of every case. Degenerate cases (scale == 0): NaNs at
    the same positions, everything else (+-inf included) bit for bit."""
    case = xc.BY_NAME[name]
    for step in case.steps(norm):
        reads, site_read, site_loc, _, T, S, seed = step
        host, sub = _host_step(step)
        dev = extract_reference(ReadBatch(reads, site_read, site_loc, norm=norm, seed=seed), T, S)
        for k in ("kmer", "means", "stds", "sanums"):
            assert xc.same_bits(dev[k], host[k], nan_positions=case.degenerate), k
        assert xc.same_bits(dev["signals"][~sub], host["signals"][~sub], nan_positions=case.degenerate)
        if case.degenerate and norm == "mad":      # what the host extractor yields for MAD == 0: NaN and +-inf, nothing finite
            assert not np.isfinite(host["means"]).any() and not np.isfinite(host["stds"]).any()
        elif not case.degenerate:
            assert all(np.isfinite(host[k]).all() for k in xc.KEYS)


@pytest.mark.parametrize("norm", ["mad", "zscore"])
def test_empty_read_does_not_change_its_neighbours(norm):
    (with_empty,), (without,) = xc.BY_NAME["mixed_batch"].steps(norm), xc.BY_NAME["mixed_batch_no_empty"].steps(norm)
    assert len(with_empty[0]) == len(without[0]) + 1 and len(with_empty[0][1][0]) == 0
    a = extract_reference(ReadBatch(*with_empty[:3], norm=norm, seed=with_empty[6]))
    b = extract_reference(ReadBatch(*without[:3], norm=norm, seed=without[6]))
    for k in xc.KEYS:
        assert xc.same_bits(a[k], b[k]), k
