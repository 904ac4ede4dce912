"""Generated training files for the `denoise` tests (TEST INFRASTRUCTURE): 12-column feature rows (extract_features.py:289-303)
with short k-mers and windows. The read name says what the row is: pos_good / pos_bad (label 1) and neg (label 0), with a
running number that makes every row unique."""
import numpy as np

KMERS = ["ACGTA", "CCGTT", "GCGAA", "TCGCC", "AAGTC"]      # the last one occurs among the negatives only


def _row(i, name, kmer, label, rng, seq_len, sig_len, shift):
    means = rng.normal(shift, 1.0, seq_len)
    stds = rng.uniform(0.05, 0.5, seq_len)
    lens = rng.integers(3, 30, seq_len)
    sig = rng.normal(shift, 1.0, sig_len)
    cols = ["chr1", str(1000 + i), "+", str(1000 + i), "%s_%d" % (name, i), "t", kmer,
            ",".join("%.6f" % v for v in means), ",".join("%.6f" % v for v in stds), ",".join(str(int(v)) for v in lens),
            ",".join("%.6f" % v for v in sig), str(label)]
    return "\t".join(cols) + "\n"


def write_training_file(path, n_good=70, n_bad=30, n_neg=100, seed=1, seq_len=5, sig_len=16):
    """Rows in a seeded random order. Positive k-mers are drawn 4 : 3 : 2 : 1 over KMERS[:4]; the negatives hold all five."""
    rng = np.random.default_rng(seed)
    kinds = ["pos_good"] * n_good + ["pos_bad"] * n_bad + ["neg"] * n_neg
    rng.shuffle(kinds)
    rows = []
    for i, kind in enumerate(kinds):
        if kind == "neg":
            kmer = KMERS[int(rng.integers(0, 5))]
        else:
            kmer = KMERS[int(rng.choice(4, p=[0.4, 0.3, 0.2, 0.1]))]
        rows.append(_row(i, kind, kmer, 0 if kind == "neg" else 1, rng, seq_len, sig_len, 0.0 if kind != "pos_good" else 1.5))
    with open(path, "w") as f:
        f.writelines(rows)
    return rows


def name_of(line):
    return line.split("\t")[4]


def kmer_of(line):
    return line.split("\t")[6]


def label_of(line):
    return int(line.strip().split("\t")[-1])
