"""GPU: fast5 feature extraction on the device (ds_extract / ds_submit_reads) against the CPU statement of the same arithmetic
(ds_extract_reference, itself held bit-identical to the host extractor by tests/test_extract_reference.py)."""
import json
import os

import numpy as np
import pytest

from deepsignal_amd import extract_features as ef
from deepsignal_amd import synth, weights
from deepsignal_amd.engine import Engine, ReadBatch, base_codes, extract_reference

import extract_cases as xc

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(__file__), "golden", "extract_golden.json")
KEYS = ("kmer", "means", "stds", "sanums", "signals")


def _bits(a):
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _reads(n, seed, long_bases=0, nbases=(400, 3000)):
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n):
        nb = int(rng.integers(*nbases))
        raw, starts, lengths, bases, scaling, offset = synth.synthetic_read(nb, seed * 1000 + i, long_bases=long_bases)
        out.append((raw, starts, lengths, base_codes(bases), scaling, offset, 100 + i))
    return out


def _all_sites(reads, kmer_len=17):
    nb = (kmer_len - 1) // 2
    sr, sl = [], []
    for i, r in enumerate(reads):
        codes = r[3]
        for loc in range(nb, len(codes) - nb):
            if codes[loc] == 1 and codes[loc + 1] == 2:
                sr.append(i)
                sl.append(loc)
    return np.array(sr, np.int32), np.array(sl, np.int32)


def _assert_same(a, b):
    for k in KEYS:
        assert a[k].shape == b[k].shape and np.array_equal(_bits(a[k]), _bits(b[k])), k


@pytest.fixture(scope="module")
def eng():
    e = Engine(device=0, max_batch=512)
    e.load_weights(weights.random_weights(seed=3, lstm_bias_std=0.1))
    yield e
    e.close()


@pytest.mark.parametrize("norm", ["mad", "zscore"])
def test_extract_matches_reference(eng, norm):
    reads = _reads(6, 1 if norm == "mad" else 2, long_bases=3)
    sr, sl = _all_sites(reads)
    for s in range(0, len(sr), 500):           # reads split across batches: each batch carries every read
        b = ReadBatch(reads, sr[s:s + 500], sl[s:s + 500], norm=norm, seed=5)
        _assert_same(eng.extract(b), extract_reference(b))


def test_extract_full_batch_and_short_windows():
    reads = _reads(3, 4, nbases=(8000, 9000))
    sr, sl = _all_sites(reads, 9)
    e = Engine(kmer_len=9, signal_len=100, device=0, max_batch=256)
    try:
        b = ReadBatch(reads, sr[:256], sl[:256], norm="zscore")
        assert b.nsites == 256
        _assert_same(e.extract(b), extract_reference(b, 9, 100))
    finally:
        e.close()


@pytest.mark.parametrize("norm", ["mad", "zscore"])
def test_extract_wide_range_reads(eng, norm):
    """Reads with spikes: raw values spanning more histogram bins than the statistics kernel keeps in LDS (global-memory
    path), next to an ordinary read (LDS path) in the same batch."""
    reads = _reads(3, 12)
    spiky = []
    for i, r in enumerate(reads):
        raw = r[0].copy()
        if i != 1:
            rng = np.random.default_rng(i)
            at = rng.choice(len(raw), 40, replace=False)
            raw[at] = rng.integers(-20000, 20000, 40).astype(np.int16)
            assert int(raw.max()) - int(raw.min()) + 1 > 8192
        spiky.append((raw,) + tuple(r[1:]))
    sr, sl = _all_sites(spiky)
    b = ReadBatch(spiky, sr[:512], sl[:512], norm=norm)
    assert len(set(b.site_read.tolist())) >= 2
    _assert_same(eng.extract(b), extract_reference(b))


def test_extract_golden_reads_match_host(eng):
    with open(GOLD) as f:
        gold = json.load(f)
    case = gold["cases"][0]
    reads, sr, sl = [], [], []
    for name in gold["read_order"]:
        r = gold["reads"][name]
        locs = [loc for loc, _, _ in ef.read_sites(r["bases"], case["motif_seqs"], 0, 17, "+", "c", 0, None)]
        if not locs:
            continue
        sr += [len(reads)] * len(locs)
        sl += locs
        reads.append((np.asarray(r["signal"], np.int16), np.asarray(r["starts"], np.int64), np.asarray(r["lengths"], np.int64),
                      base_codes(r["bases"]), r["range"] / r["digitisation"], r["offset"]))
    b = ReadBatch(reads, sr, sl)
    _assert_same(eng.extract(b), extract_reference(b))


@pytest.mark.parametrize("precision", ["fp32", "bf16x3"])
def test_submit_reads_matches_submit(precision):
    e = Engine(device=0, max_batch=512, precision=precision)
    try:
        e.load_weights(weights.random_weights(seed=3, lstm_bias_std=0.1))
        reads = _reads(5, 7)
        sr, sl = _all_sites(reads)
        batches = [ReadBatch(reads, sr[s:s + 512], sl[s:s + 512], seed=1) for s in range(0, len(sr), 512)]
        tickets = [e.submit_reads(b) for b in batches[:e.slots]]
        got = [e.wait(t) for t in tickets]
        for b, (act, pred) in zip(batches, got):
            f = extract_reference(b)
            act2, pred2 = e.wait(e.submit(f["kmer"], f["means"], f["stds"], f["sanums"], f["signals"]))
            assert np.array_equal(_bits(act), _bits(act2)) and np.array_equal(pred, pred2)
    finally:
        e.close()


def test_extract_kernel_times_are_reported(eng):
    reads = _reads(2, 9)
    sr, sl = _all_sites(reads)
    eng.set_profiling(1)
    try:
        eng.reset_stage_times()
        eng.extract(ReadBatch(reads, sr[:512], sl[:512]))
        stats = {k["name"]: k for k in eng.kernel_stats()}
        assert stats["extract_stats_kernel"]["launches"] == 1 and stats["extract_sites_kernel"]["total_ms"] > 0
    finally:
        eng.set_profiling(0)


def test_invalid_reads_are_refused_on_the_handle(eng):
    reads = _reads(1, 3)
    with pytest.raises(RuntimeError, match="ds_reads"):
        eng.extract(ReadBatch(reads, [0], [2]))
    with pytest.raises(RuntimeError, match="nsites"):
        eng.extract(ReadBatch(reads, [0] * 513, [20] * 513))


@pytest.mark.parametrize("style,norm", [("plain", "mad"), ("ont", "zscore")])
def test_call_mods_extract_on_gpu_rows_match_cpu(tmp_path, style, norm):
    """`deepsignal call_mods -i <fast5 dir> --extract_on gpu` writes the rows --extract_on cpu writes, byte for byte, except the
    probabilities of sites whose middle base took the subsample branch."""
    import shutil
    from deepsignal_amd import deepsignal as cli
    d = tmp_path / "f5"
    shutil.copytree(os.path.join(os.path.dirname(__file__), "golden", "fast5", style), str(d))
    wfile = str(tmp_path / "model.dsw")
    wts = weights.random_weights(seed=3, lstm_bias_std=0.1)
    weights.save_weights(wfile, wts)
    outs = {}
    for where in ("cpu", "gpu"):
        outs[where] = str(tmp_path / (where + ".tsv"))
        rc = cli.main(["call_mods", "-i", str(d), "-m", wfile, "-o", outs[where], "--normalize_method", norm, "--f5_batch_num", "2",
                       "--batch_size", "16", "--engine_batch", "64", "--is_gpu", "yes", "--extract_on", where])
        assert rc in (0, None)
    sub = set()      # sites whose middle base alone holds >= 360 samples: the one deliberate difference (probabilities only)
    for fp in ef.get_fast5s(str(d)):
        raw, starts, lengths, bases, _, _, info = ef._read_fast5(fp, "RawGenomeCorrected_000", "BaseCalled_template")
        for loc, pos, _ in ef.read_sites(bases, ["CG"], 0, 17, info[2], info[3], info[4], None):
            if lengths[loc] >= 360:
                sub.add((info[3], str(pos), info[2], info[0]))
    a, b = open(outs["cpu"]).read().splitlines(), open(outs["gpu"]).read().splitlines()
    assert len(a) == len(b) > 0
    # the oracle-driven harness on the same files (host features, C oracle forward): GPU-route rows within 1e-4
    from deepsignal_amd import call_modifications as cm
    from oracle import oracle

    class OracleEngine:
        class_num = 2

        def run(self, kmer, means, stds, sanums, signals):
            feats = {"kmer": np.asarray(kmer, np.int32), "means": np.asarray(means, np.float32),
                     "stds": np.asarray(stds, np.float32), "sanums": np.asarray(sanums, np.float32),
                     "signals": np.asarray(signals, np.float32)}
            return oracle.forward(wts, feats, "f32")

    out_oracle = str(tmp_path / "oracle.tsv")
    f5_args = (True, "RawGenomeCorrected_000", "BaseCalled_template", None, True, norm, "CG", 0, 1, 2, None)
    cm.call_mods(str(d), wfile, out_oracle, 17, 360, 16, 0.001, 2, 1, True, True, True, True, f5_args, engine=OracleEngine())
    ro = open(out_oracle).read().splitlines()
    assert len(ro) == len(b)
    for x, y in zip(ro, b):
        cx, cy = x.split("\t"), y.split("\t")
        assert cx[:6] == cy[:6] and cx[9] == cy[9]
        if (cx[0], cx[1], cx[2], cx[4]) not in sub:
            assert abs(float(cx[6]) - float(cy[6])) <= 1e-4 and abs(float(cx[7]) - float(cy[7])) <= 1e-4
    for ra, rb in zip(a, b):
        ca, cb = ra.split("\t"), rb.split("\t")
        if (ca[0], ca[1], ca[2], ca[4]) in sub:
            assert ca[:6] == cb[:6] and ca[9] == cb[9]
        else:
            assert ra == rb


# ---- the shared case table (tests/extract_cases.py; tests/test_extract_reference.py holds the checker to numpy on it) -------
@pytest.fixture(scope="module")
def geometry_engines():
    """One engine per (kmer_len, signal_len), kept for the module: ds_extract does not advance the slot, so consecutive cases
    of a geometry share slot 0, its pinned and device blocks and whatever the batch before left in them."""
    engines = {}
    yield lambda T, S: engines.setdefault((T, S), Engine(kmer_len=T, signal_len=S, device=0, max_batch=512))
    for e in engines.values():
        e.close()


def _batch(step):
    reads, site_read, site_loc, norm, _, _, seed = step
    return ReadBatch(reads, site_read, site_loc, norm=norm, seed=seed)


@pytest.mark.parametrize("name,norm", xc.case_norm_params())
def test_case_table_matches_reference(geometry_engines, name, norm):
    """The kernels == ds_extract_reference on every step of every case, in the case's order, on one slot. Degenerate cases
    (scale == 0): NaNs at the same positions (sign and payload not compared), everything else, +-inf included, bit for bit;
    that is the only relaxation of bit equality in this file."""
    case = xc.BY_NAME[name]
    e = geometry_engines(*case.geometry)
    for i, step in enumerate(case.steps(norm)):
        b = _batch(step)
        got, want = e.extract(b), extract_reference(b, *case.geometry)
        for k in KEYS:
            assert xc.same_bits(got[k], want[k], nan_positions=case.degenerate), (i, k)


@pytest.mark.parametrize("norm", ["mad", "zscore"])
def test_empty_read_does_not_change_its_neighbours(geometry_engines, norm):
    e = geometry_engines(17, 360)
    (with_empty,), (without,) = xc.BY_NAME["mixed_batch"].steps(norm), xc.BY_NAME["mixed_batch_no_empty"].steps(norm)
    _assert_same(e.extract(_batch(with_empty)), e.extract(_batch(without)))


def test_blocks_grow_and_are_reused_on_one_slot():
    """A fresh engine's slot allocates its blocks for a small batch, re-allocates them for one fifty times the size, and the
    small batch then runs in the large blocks."""
    case = xc.BY_NAME["block_growth"]
    e = Engine(device=0, max_batch=512)
    try:
        steps = case.steps("zscore")
        sizes = [len(s[0][0][0]) + sum(len(r[0]) for r in s[0][1:]) for s in steps]
        assert sizes[1] > 40 * sizes[0] and sizes[2] == sizes[0]
        for norm in case.norms:
            for step in case.steps(norm):
                b = _batch(step)
                _assert_same(e.extract(b), extract_reference(b))
    finally:
        e.close()


def _independence_reads():
    """Four reads with ~50 sites each: one of more than 16 numpy blocks, one with a wide raw range, one with long middle
    bases (SUB windows), one ordinary; explicit subsample keys, so a SUB window does not depend on the read's index."""
    rng = np.random.default_rng(2024)
    out = []
    for i, (nbases, long_bases) in enumerate([(15000, 0), (2500, 0), (1500, 12), (900, 0)]):
        raw, starts, lengths, _, scaling, offset = synth.synthetic_read(nbases, 600 + i, long_bases=long_bases)
        if i == 1:
            raw = raw.copy()
            raw[rng.choice(len(raw), 50, replace=False)] = rng.integers(-15000, 15000, 50).astype(np.int16)
        locs = np.sort(rng.choice(np.arange(8, nbases - 9, 2), 50, replace=False))
        if long_bases:
            sub = [int(v) for v in np.flatnonzero(lengths >= 360) if 8 <= v < nbases - 9][:6]
            locs = np.array(sorted(set(locs.tolist()) | set(sub) - {v + 1 for v in sub} - {v - 1 for v in sub}))
            locs = locs[np.concatenate([[True], np.diff(locs) >= 2])]
        out.append(((raw, starts, lengths, xc._codes(nbases, locs, rng), scaling, offset, 9000 + i), [int(v) for v in locs]))
    assert len(out[0][0][0]) > 16 * 8192 and int(out[1][0][0].max()) - int(out[1][0][0].min()) >= 8192
    assert any(out[2][0][2][loc] >= 360 for loc in out[2][1])
    return out


@pytest.mark.parametrize("norm", ["mad", "zscore"])
def test_site_bits_do_not_depend_on_the_batch(geometry_engines, norm):
    """The five feature rows of a site carry the same bits whatever batch the site travels in: (a) all reads in one batch,
    (b) reads in reversed order, (c) sites shuffled, (d) one read per batch, (e) an unrelated 1 M-sample read added."""
    e = geometry_engines(17, 360)
    rl = _independence_reads()
    rng = np.random.default_rng(5)

    def run(read_locs, order=None):
        reads, sr, sl = xc._one(read_locs)
        if order is not None:
            sr, sl = [sr[i] for i in order], [sl[i] for i in order]
        f = e.extract(ReadBatch(reads, sr, sl, norm=norm, seed=3))
        return {(reads[r][6], loc): tuple(f[k][i].view(np.uint32).tobytes() if f[k].dtype == np.float32 else f[k][i].tobytes()
                                          for k in KEYS) for i, (r, loc) in enumerate(zip(sr, sl))}

    a = run(rl)
    assert 180 <= len(a) <= 512
    b = run(rl[::-1])
    c = run(rl, order=rng.permutation(len(a)).tolist())
    d = {}
    for one in rl:
        d.update(run([one]))
    big = xc._spread_read(xc._signal(1000003, rng), 17, rng, 777)
    f = run([big] + rl)
    for other in (b, c, d, f):
        assert all(other[site] == rows for site, rows in a.items())
    assert len(f) == len(a) + len(big[1]) and len(b) == len(c) == len(d) == len(a)


@pytest.mark.parametrize("precision", ["fp32", "bf16x3"])
def test_submit_reads_long_reads_growing_blocks(precision):
    """ds_submit_reads on long reads == ds_submit of the checker's features. The batches ascend in size (20 k samples to
    1 M) and fill every slot, so each slot allocates its blocks while its neighbours' extraction and forward are in flight;
    a second round re-allocates every slot's blocks for a larger batch than it held. Tickets are waited newest first."""
    e = Engine(device=0, max_batch=512, precision=precision, slots=4)
    try:
        e.load_weights(weights.random_weights(seed=3, lstm_bias_std=0.1))
        assert e.slots == 4
        rng = np.random.default_rng(31)
        sizes = [20011, 8192 * 17 + 4000, 300007, 600001, 8192 * 33 + 129, 1050001, 8192 * 16 + 127, 700001]
        batches = []
        for i, n in enumerate(sorted(sizes)):
            reads, sr, sl = xc._one([xc._spread_read(xc._signal(n, rng), 17, rng, 50 + i, nsites=24),
                                     xc._synthetic(1200, 800 + i, 70 + i, 17, 100, long_bases=2)])
            batches.append(ReadBatch(reads, sr, sl, norm=("zscore", "mad")[i % 2], seed=1))
        for s in range(0, len(batches), e.slots):
            group = batches[s:s + e.slots]
            tickets = [e.submit_reads(b) for b in group]
            got = [e.wait(t) for t in tickets[::-1]][::-1]
            for b, (act, pred) in zip(group, got):
                f = extract_reference(b)
                act2, pred2 = e.wait(e.submit(f["kmer"], f["means"], f["stds"], f["sanums"], f["signals"]))
                assert np.array_equal(_bits(act), _bits(act2)) and np.array_equal(pred, pred2)
    finally:
        e.close()
