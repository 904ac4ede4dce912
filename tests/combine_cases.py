"""Shared by the combine_strands tests (CPU and GPU): synthetic genomes and tables, Python's own answer for the motif bitmap, and
the CPU checkers ds_motif_reference / ds_combine_reference put behind the interface combine_strands_gpu drives, so the Python half
of `--on gpu` runs without a GPU."""
import json
import os

import numpy as np

from deepsignal_amd import combine_strands as cs
from deepsignal_amd import engine as eng

from table_backend import RememberedBatches

GOLD = os.path.join(os.path.dirname(__file__), "golden", "combine_golden.json")
KMER = "ACGTACGTCGACGTACG"


def load_gold():
    with open(GOLD) as f:
        return json.load(f)


def write_bytes(path, data: bytes) -> str:
    with open(str(path), "wb") as f:
        f.write(data)
    return str(path)


def write_case(tmp_path, gold, case):
    """A golden case's FASTA and input on disk -> (input path, FASTA path)."""
    fa = write_bytes(tmp_path / "genome.fa", gold["fasta"].encode())
    inp = write_bytes(tmp_path / case["input_name"], ("\n".join(case["input_rows"]) + "\n").encode())
    return inp, fa


def fasta_text(records, width, newline="\n", final_newline=True) -> bytes:
    """records: (name, sequence) pairs -> FASTA bytes with lines of `width` bases."""
    out = []
    for name, seq in records:
        out.append(">" + name)
        out += [seq[i:i + width] for i in range(0, len(seq), width)]
    text = newline.join(out) + (newline if final_newline else "")
    return text.encode()


def random_seq(rng, n) -> str:
    s = rng.choice(list("ACGTacgtN"), n, p=[0.1, 0.28, 0.28, 0.1, 0.03, 0.08, 0.08, 0.03, 0.02])
    return "".join(s)


def random_fasta(seed: int, nbases: int):
    """(FASTA bytes, {name: upper-cased sequence}) of about nbases bases over a few records, line widths and line ends mixed."""
    rng = np.random.default_rng(seed)
    nrec = int(rng.integers(1, 6))
    cuts = np.sort(rng.integers(1, max(nbases, 2), nrec - 1)) if nrec > 1 else np.array([], np.int64)
    lens = np.diff(np.concatenate([[0], cuts, [nbases]]))
    text, genome = b"", {}
    for k, n in enumerate(lens.tolist()):
        seq = random_seq(rng, max(int(n), 1))
        name = "ctg%d" % k
        genome[name] = seq.upper()
        text += fasta_text([(name + (" note" if k % 2 else ""), seq)], int(rng.choice([1, 7, 60, 100])), "\r\n" if k % 3 == 1 else "\n")
        if rng.random() < 0.3:
            text += b"\n"
    return (text.rstrip(b"\r\n") if seed % 2 else text), genome


def table_row(name, pos, strand, p0="1.250", p1="2.750", met=1, unmet=3, cov=4, kmer=KMER, pis=7) -> str:
    return "\t".join([name, str(pos), strand, str(pis), str(p0), str(p1), str(met), str(unmet), str(cov), "0.2500", kmer])


def bed_row(name, pos, strand, cov=4, pct=25) -> str:
    return "\t".join([name, str(pos), str(pos + 1) if isinstance(pos, int) else "0", ".", str(cov), strand, str(pos), "0", "0,0,0", str(cov),
                      str(pct)])


def random_table(seed: int, genome: dict, nrows: int, bed: bool = False):
    """nrows rows scattered over the CGs of `genome` (both strands), now and then a position that is no CG, an unknown name, a
    coverage of 0; the doubles as a frequency table prints them (%.3f), which sum differently in another order."""
    rng = np.random.default_rng(seed)
    names = list(genome)
    sites = [(n, i) for n in names for i in range(len(genome[n]) - 1) if genome[n][i:i + 2] == "CG"] or [(names[0], 0)]
    rows = []
    for r in range(nrows):
        u = rng.random()
        if u < 0.06:
            name = names[int(rng.integers(0, len(names)))]
            pos, strand = int(rng.integers(-1, len(genome[name]) + 2)), "+-"[int(rng.integers(0, 2))]
        elif u < 0.08:
            name, pos, strand = "chrUn", int(rng.integers(0, 50)), "+"
        else:
            name, pos = sites[int(rng.integers(0, len(sites)))]
            strand = "+-"[int(rng.integers(0, 2))]
            pos += strand == "-"
        cov = 0 if rng.random() < 0.05 else int(rng.integers(1, 60))
        met = int(rng.integers(0, cov + 1))
        if bed:
            rows.append(bed_row(name, pos, strand, cov, "%.1f" % rng.uniform(0, 100) if rng.random() < 0.5 else int(rng.integers(0, 101))))
        else:
            p1 = rng.uniform(0, cov) if cov else 0.0
            rows.append(table_row(name, pos, strand, "%.3f" % (cov - p1), "%.3f" % p1, met, cov - met, cov, KMER[r % 5:] + "ACGT"[:r % 4 + 1],
                                  pis=1000 - pos))
    return rows


def python_bitmap(seqs) -> np.ndarray:
    """Python's answer: the records' upper-cased sequences back to back, bit i set iff a CG begins at base i of a record."""
    nbits = sum(len(s) for s in seqs)
    bits = np.zeros(((nbits + 31) // 32) * 32, np.uint8)
    base = 0
    for s in seqs:
        i = s.find("CG")
        while i >= 0:
            bits[base + i] = 1
            i = s.find("CG", i + 1)
        base += len(s)
    return np.packbits(bits.reshape(-1, 32)[:, ::-1], axis=1).view(">u4").astype(np.uint32).ravel()


class CheckerBackend(RememberedBatches):
    """combine_begin .. combine_end of Engine on top of ds_motif_reference and ds_combine_reference: the chunks go into a host
    bitmap as they come, the batches are remembered, and the checker makes its one pass in row order over all of them when the
    result is asked for."""

    def combine_begin(self, form, rec_len, total_rows, batch_rows):
        self.begun(total_rows, batch_rows)
        self.form, self.rec_len = form, np.array(rec_len, np.int64)
        self.nbits = int(self.rec_len.sum())
        self.bitmap = np.zeros((self.nbits + 31) // 32, np.uint32)

    def combine_genome(self, text, seg_begin, seg_end, seg_bit, seg_carry):
        assert not self.batches, "the genome comes first"
        assert int(seg_end[-1]) - int(seg_begin[0]) <= eng.COMBINE_MAX_CHUNK
        eng.motif_reference(text, seg_begin, seg_end, seg_bit, seg_carry, self.nbits, self.bitmap)

    def combine_bitmap(self):
        return self.bitmap.copy()

    def combine_parse(self, text, begin, end, chrom, flags):
        chunk, b, e = self.remember(text, begin, end, chrom=np.array(chrom, np.int32), flags=np.array(flags, np.uint8))
        return eng.combine_reference(self.form, chunk, b, e, chrom, flags, self.rec_len, self.bitmap, sites=False)["status"]

    def combine_accumulate(self, rows=(), given=()):
        self.give({int(r): v for r, v in zip(rows, given)})

    def combine_result(self):
        text, begin, end, (chrom, flags), given, row = self.joined("chrom", "flags")
        out = eng.combine_reference(self.form, text, begin, end, chrom, flags, self.rec_len, self.bitmap, given)
        assert not (out["status"] == eng.TEXT_ROW_HOST).any(), "a host row got no values"
        res = {k: out[k] for k in ("chrom", "pos", "sum0", "sum1", "met", "unmet", "cov", "last_plus")}
        res["rows"] = row
        return res

    combine_times, combine_end = RememberedBatches.times, RememberedBatches.close


def run_route(tmp_path, capsys, inp, fa, on, contig="", **kw):
    """One route on (inp, fa) -> (output bytes, stdout). on: "cpu", or "gpu" with the keywords of combine_strands_gpu."""
    out = str(tmp_path / ("out_%s%s" % (on, os.path.splitext(inp)[1])))
    capsys.readouterr()
    rows = cs.combine_strands_cpu(inp, fa, contig) if on == "cpu" else cs.combine_strands_gpu(inp, fa, contig, **kw)
    cs.write_rows(rows, out)
    return open(out, "rb").read(), capsys.readouterr().out
