"""Shared inputs of the feature-row tests (tests/test_extract_rows_reference.py on the CPU, tests/test_gpu_extract_rows.py on the
GPU): the directed table of values for the number rule, and the host extractor's rows of a step of tests/extract_cases.py."""
import numpy as np

from deepsignal_amd import extract_features as ef
from deepsignal_amd import synth
from deepsignal_amd.engine import ReadBatch, base_codes, pack_info

LABEL = 1


def directed_values():
    """+-0, values that round to +-0, every K in [-300, 300) as K / 1e6 (the exponent forms), fraction edges, large values,
    NaN of both signs, +-inf, seeded normal draws at three scales."""
    rng = np.random.default_rng(20240611)
    parts = [[0.0, -0.0, 4e-7, -4e-7], [k / 1e6 for k in range(-300, 300)],
             [0.0001, 0.999999, 0.9999995, 1.0, 2.5, -3.0, 123456.789012, 65536 * 3.1, 1e8 + 0.5e-6],
             [np.nan, -np.nan, np.copysign(np.nan, -1.0), np.inf, -np.inf]]
    parts += [rng.normal(0.0, scale, 20000) for scale in (1e-5, 1.0, 300.0)]
    return np.concatenate([np.asarray(p, np.float64) for p in parts])


def numpy_text(values):
    with np.errstate(all="ignore"):
        return ",".join(str(np.around(np.float64(v), 6)) for v in values).encode()


def host_rows(step):
    """The host extractor's row text of every site of a step, in the step's site order (read i is named r<i>), and the mask of
    the sites whose window is an ordered subsample (SUB)."""
    reads, site_read, site_loc, norm, T, S, _ = step
    per_read = {}
    for i in sorted(set(int(r) for r in site_read)):
        r = reads[i]
        bases = "".join("ACGTN"[c] for c in r[3])
        with np.errstate(all="ignore"):
            feats = ef.extract_read_features(r[0], r[1], r[2], bases, r[4], r[5], "r%d" % i, "t", "+", "chr%d" % (i % 3), 1000 * i,
                                             None, ["CG"], 0, T, S, LABEL, norm)
            locs = [loc for loc, _, _ in ef.read_sites(bases, ["CG"], 0, T, "+", "c", 0, None)]
            per_read[i] = dict(zip(locs, (ef._features_to_str(f) for f in feats)))
    rows = [per_read[int(rd)][int(loc)] for rd, loc in zip(site_read, site_loc)]
    sub = np.array([reads[rd][2][loc] >= S for rd, loc in zip(site_read, site_loc)])
    return rows, sub


def step_inputs(step, rows):
    """(ReadBatch, info blob, info offsets) of a step; the leading columns are those of the host rows."""
    reads, site_read, site_loc, norm, _, _, seed = step
    info, info_off = pack_info(["\t".join(r.split("\t")[:6]).encode() for r in rows])
    return ReadBatch(reads, site_read, site_loc, norm=norm, seed=seed), info, info_off


def split_rows(text, row_off):
    assert row_off[0] == 0 and np.all(np.diff(row_off) > 0) and row_off[-1] == len(text)
    rows = [text[a:b] for a, b in zip(row_off[:-1], row_off[1:])]
    assert all(r.endswith(b"\n") and r.count(b"\n") == 1 for r in rows)
    return [r[:-1].decode() for r in rows]


def two_read_batch(T, norm, nsites=70):
    """(ReadBatch, info blob, info offsets): `nsites` CG sites of two synthetic reads, half from each, at k-mer length T, and the
    six leading columns of their rows. Shared by the output-extent tests (CPU and GPU)."""
    reads = []
    for i in range(2):
        raw, starts, lengths, bases, scaling, offset = synth.synthetic_read(700 + 90 * i, 40 + i, long_bases=i)
        reads.append((raw, starts, lengths, base_codes(bases), scaling, offset, 500 + i))
    sr, sl = [], []
    for i, r in enumerate(reads):
        codes = r[3]
        for loc in range(T // 2, len(codes) - T // 2):
            if codes[loc] == 1 and codes[loc + 1] == 2:
                sr.append(i)
                sl.append(loc)
    half = nsites // 2
    assert sr.count(0) >= half and sr.count(1) >= nsites - half
    sr, sl = np.array(sr[:half] + sr[half - nsites:], np.int32), np.array(sl[:half] + sl[half - nsites:], np.int32)
    rows = [("chr%d\t%d\t+\t%d\tread%d\tt" % (r, loc, 5 * loc, r)).encode() for r, loc in zip(sr.tolist(), sl.tolist())]
    return (ReadBatch(reads, sr, sl, norm=norm, seed=3),) + pack_info(rows)
