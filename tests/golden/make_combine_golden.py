"""Golden vectors for scope row f5 by RUNNING the reference script
(/root/reference/scripts/combine_two_strands_frequency.py — stdlib only, runs under any Python):
    python tests/golden/make_combine_golden.py
Commits a synthetic FASTA, four inputs (table, table with --contig, bedMethyl, a table of several concatenated runs) and for each
the reference's output lines and captured stdout."""
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference/scripts/combine_two_strands_frequency.py"
KMER = "ACGTACGTCGACGTACG"
rng = np.random.default_rng(11)


def seq(n):
    """n random bases, CG-rich, mixed case."""
    s = "".join(rng.choice(list("ACGT"), n, p=[0.15, 0.35, 0.35, 0.15]))
    return "".join(c.lower() if rng.random() < 0.3 else c for c in s)


def wrap(s, width, nl):
    return nl.join(s[i:i + width] for i in range(0, len(s), width)) + nl


# chr1: CRLF lines of 20 with a description after the name, a blank line inside, and a CG across a line break
s1 = seq(95)
s1 = s1[:19] + "cG" + s1[21:]                     # bases 19 | 20: the C ends a line, the G opens the next
# chrD comes twice: the later record replaces the earlier one. chr2 ends in C and the record after it opens with G.
sd_old, sd_new = seq(30), seq(41)
s2 = seq(63) + "C"
s3 = "G" + seq(52)
fasta = (">chr1 first contig, description after the name\r\n" + wrap(s1[:40], 20, "\r\n") + "\r\n" + wrap(s1[40:], 20, "\r\n")
         + ">chrD\n" + wrap(sd_old, 7, "\n")
         + ">empty\n"
         + ">chr2\n" + wrap(s2, 60, "\n")
         + ">chr3\n" + wrap(s3, 1, "\n")
         + ">chrD again\n" + "\n" + wrap(sd_new, 13, "\n")).rstrip("\n")      # no final newline
genome = {"chr1": s1.upper(), "chrD": sd_new.upper(), "chr2": s2.upper(), "chr3": s3.upper()}
assert genome["chr1"][19:21] == "CG" and genome["chr2"][-1] == "C" and genome["chr3"][0] == "G" and not fasta.endswith("\n")


def table_rows(seed, bed=False):
    r = np.random.default_rng(seed)
    rows = []

    def row(name, pos, strand):
        cov = int(r.integers(0, 30)) if r.random() > 0.08 else 0
        met = int(r.integers(0, cov + 1))
        p1 = float(r.uniform(0, cov)) if cov else 0.0
        if bed:
            pct = str(int(round(met / cov * 100, 0))) if cov else "0"
            return "\t".join([name, str(pos), str(pos + 1), ".", str(cov), strand, str(pos), str(pos + 1), "0,0,0", str(cov), pct])
        return "\t".join([name, str(pos), strand, str(1000 - pos), "%.3f" % (cov - p1), "%.3f" % p1, str(met), str(cov - met), str(cov),
                          "%.4f" % (met / cov if cov else 0.0), KMER[int(r.integers(0, 5)):] + "ACGT"])

    for name, s in genome.items():
        for i in range(len(s) - 1):
            if s[i:i + 2] == "CG":
                u = r.random()
                if u < 0.75:
                    rows.append(row(name, i, "+"))
                if u > 0.15:
                    rows.append(row(name, i + 1, "-"))       # u > 0.75: a site with '-' rows only
            elif r.random() < 0.06:
                rows.append(row(name, i, "+-"[int(r.integers(0, 2))]))
        rows.append(row(name, 0, "-"))                       # key -1
        rows.append(row(name, len(s) - 1, "+"))
        rows.append(row(name, len(s), "-"))
        rows.append(row(name, len(s), "+"))
    rows.append(row("chrUn", 5, "+"))
    rows.append(row("empty", 0, "+"))
    rows.append(row("chr1", 1 << 40, "-"))
    order = r.permutation(len(rows))
    return [rows[i] for i in order]


inputs = [("table", "freq.tsv", table_rows(1), ""), ("table --contig", "freq.tsv", table_rows(2), "chrD"),
          ("bed", "freq.BED", table_rows(3, bed=True), ""),
          ("concatenated runs", "freq.txt", table_rows(4) + table_rows(5) + table_rows(6), "")]
cases = []
with tempfile.TemporaryDirectory() as d:
    fa = os.path.join(d, "genome.fa")
    with open(fa, "w", newline="") as f:
        f.write(fasta)
    for name, fname, rows, contig in inputs:
        inp = os.path.join(d, fname)
        with open(inp, "w") as f:
            f.write("\n".join(rows) + "\n")
        argv = [sys.executable, "-B", REF, "--frequency_fp", inp, "-r", fa] + (["--contig", contig] if contig else [])
        stdout = subprocess.run(argv, check=True, stdout=subprocess.PIPE, cwd=os.path.dirname(REF),
                                env=dict(os.environ, PYTHONDONTWRITEBYTECODE="1")).stdout.decode()
        base, ext = os.path.splitext(inp)
        out = base + ".fb_combined" + ext
        cases.append({"name": name, "input_name": fname, "input_rows": rows, "contig": contig, "output": open(out).read().splitlines(),
                      "stdout": stdout})
        os.remove(out)
with open(os.path.join(HERE, "combine_golden.json"), "w") as f:
    json.dump({"generator": "tests/golden/make_combine_golden.py (reference script run here)", "fasta": fasta, "cases": cases}, f)
print("wrote combine_golden.json", [(c["name"], len(c["input_rows"]), len(c["output"]), c["stdout"].count("\n")) for c in cases])
