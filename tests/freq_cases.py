"""Shared by the frequency tests (CPU and GPU): synthetic call_mods result files, and the CPU checker ds_freq_reference put
behind the interface calculate_mods_frequency_gpu drives, so the Python half of `--on gpu` runs without a GPU."""
import struct

import numpy as np

from deepsignal_amd import engine as eng

from table_backend import RememberedBatches

KMER = "ACGTACGTCGACGTACG"


def bits(x: float) -> bytes:
    return struct.pack("<d", x)


def call_row(chrom, pos, p0, p1, label=None, strand="+", pis=None, read="read0", kmer=KMER) -> str:
    """One result row; p0 / p1 are written as given when they are text, else as str(np.float32)."""
    t0 = p0 if isinstance(p0, str) else str(np.float32(p0))
    t1 = p1 if isinstance(p1, str) else str(np.float32(p1))
    if pis is None:
        pis = 1000 - pos if isinstance(pos, int) else 7
    if label is None and not (isinstance(p0, str) or isinstance(p1, str)):
        label = int(float(t1) > float(t0))
    return "\t".join([chrom, str(pos), strand, str(pis), read, "t", t0, t1, str(1 if label is None else label), kmer])


def random_rows(seed: int, nrows: int, nsites: int, nchrom: int):
    """nrows rows over at most nsites sites of nchrom chromosomes, scattered; probabilities as call_mods prints them
    (str(np.float32) of p and of 1 - p, now and then a tiny one in exponent form)."""
    rng = np.random.default_rng(seed)
    sites = [("chr%d" % rng.integers(1, nchrom + 1), int(rng.integers(0, 5000))) for _ in range(nsites)]
    rows = []
    for r in range(nrows):
        chrom, pos = sites[int(rng.integers(0, nsites))]
        p = np.float32(rng.random()) if rng.random() > 0.05 else np.float32(10.0 ** -rng.uniform(4, 9))
        rows.append(call_row(chrom, pos, np.float32(1) - p, p, read="read%d" % r))
    return rows


def stats_tuple(stats):
    """SiteStats dict -> comparable list in dict order: key, text fields, the sums' bits, the counts."""
    return [(k, s.strand, s.pos_in_strand, s.kmer, bits(s.prob_0), bits(s.prob_1), s.met, s.unmet, s.coverage)
            for k, s in stats.items()]


class ReferenceBackend(RememberedBatches):
    """freq_begin .. freq_end of Engine on top of ds_freq_reference: the batches are remembered and the checker makes its one
    pass in row order over all of them when the result is asked for."""

    def freq_begin(self, total_rows, batch_rows, prob_cf=0.0):
        self.begun(total_rows, batch_rows)
        self.cf = prob_cf

    def freq_parse(self, text, begin, end, chrom, flags):
        chunk, b, e = self.remember(text, begin, end, chrom=np.array(chrom, np.int32), flags=np.array(flags, np.uint8))
        return eng.freq_reference(chunk, b, e, chrom, flags, self.cf)["status"]

    def freq_accumulate(self, rows=(), chrom=(), pos=(), p0=(), p1=(), met=()):
        self.give({int(r): (int(c), int(q), float(a), float(b), int(m)) for r, c, q, a, b, m in zip(rows, chrom, pos, p0, p1, met)})

    def freq_result(self):
        text, begin, end, (chrom, flags), given, row = self.joined("chrom", "flags")
        out = eng.freq_reference(text, begin, end, chrom, flags, self.cf, given)
        assert not (out["status"] != eng.TEXT_ROW_OK).any(), "a host row got no values"
        return {"first_row": out["first_row"], "chrom": out["chrom"], "pos": out["pos"], "sum0": out["sum0"], "sum1": out["sum1"],
                "met": out["met"], "unmet": out["unmet"], "rows": row, "used": out["used"]}

    freq_times, freq_end = RememberedBatches.times, RememberedBatches.close
