"""Golden vectors for scope row f6 by RUNNING the reference script
(/root/reference/scripts/evaluate_mods_call.py -- needs numpy and scikit-learn):
    python tests/golden/make_evaluate_golden.py
Commits data only: per case the two input files' text, the reference's output lines and its captured stdout. The subsampled case
(more than 100,000 rows per file) commits the seed its rows are generated from (tests/evaluate_cases.py subsample_texts) in the place
of the rows; the script is run for it through a wrapper written here that seeds `random` first, so that our --seed picks its rows."""
import json
import os
import random
import subprocess
import sys
import tempfile
from fractions import Fraction

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from evaluate_cases import SUBSAMPLE_SEED, call_row, scored_rows, subsample_texts  # noqa: E402
from deepsignal_amd import evaluate_mods_call as ev  # noqa: E402

REF = "/root/reference/scripts/evaluate_mods_call.py"
# The script is always run through this wrapper of the generator's own: it seeds `random` when asked to, and it gives the script the
# scikit-learn it was written for. Those releases raised ValueError from roc_auc_score when y_true holds one class, which the script
# catches ("for only one kind of label": auroc = 0); newer ones warn (UndefinedMetricWarning) and return nan, which the script would
# print as "nan". The wrapper turns that one warning back into the ValueError; nothing of the script is changed.
WRAPPER = ("import os, random, runpy, sys, warnings\n"
           "from sklearn.exceptions import UndefinedMetricWarning\n"
           "def one_class(message, category, *a, **k):\n"
           "    if issubclass(category, UndefinedMetricWarning):\n"
           "        raise ValueError(str(message))\n"
           "warnings.showwarning = one_class\n"
           "warnings.simplefilter('always', UndefinedMetricWarning)\n"
           "if sys.argv[1] != 'none':\n"
           "    random.seed(int(sys.argv[1]))\n"
           "del sys.argv[:2]\n"
           "sys.path.insert(0, os.path.dirname(sys.argv[0]))\n"
           "runpy.run_path(sys.argv[0], run_name='__main__')\n")


def text(rows, newline="\n", final=True):
    return newline.join(rows) + (newline if final and rows else "")


def balanced():
    """~500 + 700 rows at two places (ties across the classes), |p1 - p0| on several cut-offs as decimals, labels 0 / 1 / 2, mixed
    tab and space runs, leading blanks."""
    r = np.random.default_rng(21)
    un, me = scored_rows(31, 480, 0.36), scored_rows(32, 680, 0.64)
    for rows, n in ((un, 20), (me, 20)):
        for k in range(n):
            # differences 0.05, 0.075, 0.1, 0.15, 0.3, 0.6 and their negatives, as the decimals a result file holds
            d = [0.05, 0.075, 0.1, 0.15, 0.3, 0.6][k % 6] * (1 if k % 4 else -1)
            p1 = "%.4f" % (0.5 + d / 2)
            rows.append(call_row(r, p1, p0_text="%.4f" % (0.5 - d / 2)))
    for rows in (un, me):
        for i in range(0, len(rows), 9):
            f = rows[i].split("\t")
            f[8] = "2"
            rows[i] = "\t".join(f)
        for i in range(3, len(rows), 11):
            rows[i] = rows[i].replace("\t", " \t ", 2).replace("\t", "  ", 1)
        for i in range(5, len(rows), 13):
            rows[i] = " \t" + rows[i] + "\textra column"
    return text(un), text(me, final=False)


def separated(inverted):
    lo, hi = ["%.2f" % v for v in np.linspace(0.02, 0.45, 30)], ["%.2f" % v for v in np.linspace(0.55, 0.99, 36)]
    r = np.random.default_rng(5)
    un, me = (hi, lo) if inverted else (lo, hi)
    return text([call_row(r, v) for v in un]), text([call_row(r, v) for v in me])


def with_nan():
    r = np.random.default_rng(6)
    un, me = scored_rows(41, 30, 0.4), scored_rows(42, 30, 0.6)
    me[7] = call_row(r, "nan", label=1, p0_text="0.5")
    return text(un), text(me)


cases_in = [("balanced, with ties", balanced()), ("one class: no unmethylated call", ("", text(scored_rows(51, 40, 0.6)))),
            ("one class: no methylated call", (text(scored_rows(52, 35, 0.4)), "")), ("perfect separation", separated(False)),
            ("inverted separation", separated(True)), ("nan as prob_1", with_nan())]


def not_a_decimal_half(un, me, picks=None):
    """The exact AUROC of a tested set is not k + 1/2 thousandths: where it is, %.3f of the script's trapezoid may round either way."""
    parts = [[ev.row_values(line.split())[1] for line in t.splitlines()] for t in (un, me)]
    if picks is not None:
        parts = [[p[i] for i in idx] for p, idx in zip(parts, picks)]
    p1 = np.array(parts[0] + parts[1])
    truth = np.array([False] * len(parts[0]) + [True] * len(parts[1]))
    if not np.isfinite(p1).all() or truth.all() or not truth.any():
        return True
    u2, p, n = ev.exact_auc_parts(p1, truth)
    return (Fraction(u2, 2 * p * n) * 1000) % 1 != Fraction(1, 2)


def run_reference(d, un, me, seed=None):
    paths = []
    for name, t in (("un.tsv", un), ("me.tsv", me)):
        paths.append(os.path.join(d, name))
        with open(paths[-1], "w", newline="") as f:
            f.write(t)
    out = os.path.join(d, "result.tsv")
    wrapper = os.path.join(d, "run_reference.py")
    with open(wrapper, "w") as f:
        f.write(WRAPPER)
    argv = [sys.executable, "-B", wrapper, "none" if seed is None else str(seed), REF, "--unmethylated", paths[0], "--methylated", paths[1], "--result_file", out]
    stdout = subprocess.run(argv, check=True, stdout=subprocess.PIPE, cwd=os.path.dirname(REF),
                            env=dict(os.environ, PYTHONDONTWRITEBYTECODE="1")).stdout.decode()
    with open(out) as f:
        return f.read().splitlines(), stdout


cases = []
with tempfile.TemporaryDirectory() as d:
    for name, (un, me) in cases_in:
        assert not_a_decimal_half(un, me), name
        output, stdout = run_reference(d, un, me)
        cases.append({"name": name, "unmethylated": un, "methylated": me, "output": output, "stdout": stdout})
    un, me = subsample_texts(61)
    picks = ev.sample_rows(len(un.splitlines()), len(me.splitlines()), ev.NUM_SITES, random.Random(SUBSAMPLE_SEED))
    assert not_a_decimal_half(un, me) and not_a_decimal_half(un, me, picks)
    output, stdout = run_reference(d, un, me, seed=SUBSAMPLE_SEED)
    cases.append({"name": "subsampled", "rows_seed": 61, "seed": SUBSAMPLE_SEED, "output": output, "stdout": stdout})
with open(os.path.join(HERE, "evaluate_golden.json"), "w") as f:
    json.dump({"generator": "tests/golden/make_evaluate_golden.py (reference script run here)", "cases": cases}, f)
print("wrote evaluate_golden.json", [(c["name"], len(c["output"]), c["stdout"].count("\n")) for c in cases])
