"""Call accuracy and AUROC from two labelled call_mods result files -- scope row f6, the step that judges a set of calls. Same
algorithm, output and stdout as the reference script (scripts/evaluate_mods_call.py): one file of calls from an unmethylated
sample, one from a fully methylated sample; per prob_cf cut-off of numpy.arange(0, 0.70, 0.025) a row with the confusion matrix,
eight rates, the AUROC and how many calls stand at that cut-off and how many of those are right, for a sample of `num_sites` calls
per file and, at cut-off 0, for all of them.

What is computed differently, with the same result: every row is read once, not 29 times; the sample is a shuffled index list (it
draws the numbers random.shuffle draws for the script's record list); and the AUROC needs no scikit-learn: over the distinct values
of prob_1 in ascending order, U2 = sum pos_i * (2 * sum_{j<i} neg_j + neg_i) and auc = U2 / (2 P N) -- the trapezoid area under the
ROC curve in integers, one division at the end (DESIGN.md f6 names the one place where its third decimal can differ).

`--on cpu` (evaluate_cpu) parses with Python's own split(), int() and float(). `--on gpu` (evaluate_gpu) leaves the host to find
the rows (ds_eval_locate); the device parses them, counts, and keeps the distinct scores in the site table (csrc/ds_eval.hip).
Rows in a form the device does not parse go through the expressions of the cpu route right here. File and stdout are byte-identical
to `--on cpu`."""
from __future__ import annotations

import argparse
import io
import math
import os
import random
import sys
from typing import Callable, List, Optional, Sequence, Tuple

import numpy

if __package__ in (None, ""):                       # run as a script: the package is the directory above
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import deepsignal_amd  # noqa: F401
    __package__ = "deepsignal_amd"

from . import table_route as tr
from .table_route import _CpuRoute

NUM_SITES = 100000                                  # the script's num_sites[0]
PROB_CFS = numpy.arange(0, 0.70, 0.025)             # the script's own doubles: 0.075 is not the literal
HEADER = ("tested_type\tprob_cf\ttrue_positive\tfalse_positive\ttrue_negative\tfalse_negative\t"
          "accuracy\trecall\tspecificity\tprecision\t"
          "fallout\tmiss_rate\tFDR\tNPV\tauc\ttotal_num\tcalled_num\tcalled_ratio\tcalled_accuracy\n")
MSG_TOTAL = "there are {} basemod candidates totally"


def row_values(f: List[str]) -> Tuple[float, float, int]:
    """The fields of one row through ModRecord's expressions in ModRecord's order -> (prob_0, prob_1, label); raises what the
    script raises on a malformed row (a blank line: IndexError). Shared by the cpu route and the gpu route's host rows."""
    f[0]
    int(f[1])
    f[2]
    int(f[3])
    f[4]
    f[5]
    prob_0, prob_1, label = float(f[6]), float(f[7]), int(f[8])
    f[9]
    return prob_0, prob_1, label


def read_calls(path: str):
    """(prob_0 float64[n], prob_1 float64[n], called bool[n]) of a result file; called = a non-zero label."""
    p0: List[float] = []
    p1: List[float] = []
    lab: List[bool] = []
    with open(path) as rf:
        for line in rf:
            a, b, c = row_values(line.rstrip().split())
            p0.append(a)
            p1.append(b)
            lab.append(c != 0)
    return numpy.array(p0, numpy.float64), numpy.array(p1, numpy.float64), numpy.array(lab, numpy.bool_)


def sample_rows(n_unmeth: int, n_meth: int, num_sites: int, rng) -> List[numpy.ndarray]:
    """The rows of each file that are in the _N sample, as index arrays [unmethylated, methylated]. The script shuffles each
    file's record list, unmethylated first, and takes the first num_sites; a shuffled index list draws the same numbers. When
    neither file has more than num_sites rows the sample is everything and no number is drawn."""
    if n_unmeth <= num_sites and n_meth <= num_sites:
        return [numpy.arange(n_unmeth, dtype=numpy.int64), numpy.arange(n_meth, dtype=numpy.int64)]
    picks = []
    for n in (n_unmeth, n_meth):
        idx = list(range(n))
        rng.shuffle(idx)
        picks.append(numpy.array(idx[:num_sites], numpy.int64))
    return picks


def exact_auc_parts(scores: numpy.ndarray, truth: numpy.ndarray) -> Tuple[int, int, int]:
    """(U2, P, N) of finite scores: over the distinct values ascending (-0.0 is 0.0), U2 = sum pos_i * (2 * below_i + neg_i)."""
    s = numpy.asarray(scores, numpy.float64) + 0.0
    truth = numpy.asarray(truth, numpy.bool_)
    uniq, inv = numpy.unique(s, return_inverse=True)
    inv = inv.reshape(-1)
    pos = numpy.bincount(inv[truth], minlength=uniq.size).astype(numpy.int64)
    neg = numpy.bincount(inv[~truth], minlength=uniq.size).astype(numpy.int64)
    below = numpy.cumsum(neg) - neg
    return int((pos * (2 * below + neg)).sum()), int(pos.sum()), int(neg.sum())


def auc_value(u2: int, p: int, n: int, finite: bool = True) -> float:
    """U2 / (2 P N): integers, one correctly rounded division. 0 where sklearn raises the ValueError the script catches: one class
    only, or a score that is NaN or infinite."""
    if not finite or p == 0 or n == 0:
        return 0
    return int(u2) / (2 * int(p) * int(n))


def exact_auc(scores, truth) -> float:
    scores = numpy.asarray(scores, numpy.float64)
    if scores.size and not bool(numpy.isfinite(scores).all()):
        return 0
    return auc_value(*exact_auc_parts(scores, truth))


def format_stats(tp: int, fp: int, tn: int, fn: int, total: int, called: int, correct: int, auroc: float) -> str:
    """The tail of a result row: the script's rates and its 17 %-formats; prints the script's `tp fp tn fn` line first. An empty
    tested set ends in the script's ZeroDivisionError."""
    print(tp, fp, tn, fn)
    precision, recall, specificity, accuracy = 0, 0, 0, 0
    fall_out, miss_rate, fdr, npv = 0, 0, 0, 0
    called_accuracy = 0
    if total > 0:
        accuracy = float(tp + tn) / total
        if tp + fp > 0:
            precision = float(tp) / (tp + fp)
            fdr = float(fp) / (tp + fp)
        if tp + fn > 0:
            recall = float(tp) / (tp + fn)
            miss_rate = float(fn) / (tp + fn)
        if tn + fp > 0:
            specificity = float(tn) / (tn + fp)
            fall_out = float(fp) / (fp + tn)
        if tn + fn > 0:
            npv = float(tn) / (tn + fn)
        if called > 0:
            called_accuracy = float(correct) / called
    else:
        auroc = 0
    return "%d\t%d\t%d\t%d\t%.3f\t%.3f\t%.3f\t%.3f\t%.3f\t%.3f\t%.3f\t%.3f\t%.3f\t%d" \
           "\t%d\t%.3f\t%.3f" % (tp, fp, tn, fn,
                                 accuracy, recall, specificity, precision,
                                 fall_out, miss_rate, fdr, npv, auroc, total,
                                 called, float(called) / total,
                                 called_accuracy)


class SetStats:
    """What one tested set comes to: the confusion matrix, per cut-off called / correct, and the AUROC."""

    def __init__(self, tp, fp, tn, fn, called: Sequence[int], correct: Sequence[int], auroc: float):
        self.tp, self.fp, self.tn, self.fn = int(tp), int(fp), int(tn), int(fn)
        self.called, self.correct, self.auroc = [int(v) for v in called], [int(v) for v in correct], auroc

    @property
    def total(self) -> int:
        return self.tp + self.fp + self.tn + self.fn

    def row(self, k: int) -> str:
        return format_stats(self.tp, self.fp, self.tn, self.fn, self.total, self.called[k], self.correct[k], self.auroc)


def set_stats(p0, p1, called, truth) -> SetStats:
    """SetStats of rows given as arrays, the script's comparisons in float64: called_k = |p1 - p0| >= cf_k, correct_k =
    (p1 - p0 >= cf_k) == truth among those."""
    truth = numpy.asarray(truth, numpy.bool_)
    tp = int((called & truth).sum())
    fp = int((called & ~truth).sum())
    tn = int((~called & ~truth).sum())
    fn = int((~called & truth).sum())
    with numpy.errstate(invalid="ignore"):
        d = p1 - p0
        ad = numpy.abs(d)
        n_called, n_correct = [], []
        for cf in PROB_CFS:
            stands = ad >= cf
            n_called.append(int(stands.sum()))
            n_correct.append(int((stands & ((d >= cf) == truth)).sum()))
    return SetStats(tp, fp, tn, fn, n_called, n_correct, exact_auc(p1, truth))


def write_result(result_file: str, num_sites: int, sample: Callable[[], SetStats], everything: Callable[[], SetStats]) -> None:
    """The script's table: 28 `_N` rows and the all_sites row at cut-off 0. The sets are asked for when their rows are due."""
    with open(os.path.abspath(result_file), "w") as wf:
        wf.write(HEADER)
        st = sample()
        for k, cf in enumerate(PROB_CFS):
            wf.write("\t".join(["_" + str(num_sites), "%.3f" % cf, st.row(k)]) + "\n")
        st = everything()
        wf.write("\t".join(["all_sites", "%.3f" % 0.0, st.row(0)]) + "\n")


# ---- the cpu route ----------------------------------------------------------------------------------------------------------
def evaluate_cpu(unmethylated: str, methylated: str, result_file: str, num_sites: int = NUM_SITES, rng=random) -> None:
    files = []
    for path in (unmethylated, methylated):
        files.append(read_calls(path))
        print(MSG_TOTAL.format(files[-1][0].size))
    picks = sample_rows(files[0][0].size, files[1][0].size, num_sites, rng)

    def gather(chosen) -> SetStats:
        cols = [[c if idx is None else c[idx] for c in f] for f, idx in zip(files, chosen)]
        truth = numpy.concatenate([numpy.zeros(cols[0][0].size, numpy.bool_), numpy.ones(cols[1][0].size, numpy.bool_)])
        return set_stats(*(numpy.concatenate([cols[0][k], cols[1][k]]) for k in range(3)), truth)

    write_result(result_file, num_sites, lambda: gather(picks), lambda: gather([None, None]))


# ---- the gpu route ----------------------------------------------------------------------------------------------------------
def _python_fields(raw: bytes) -> List[str]:
    """A row's bytes -> the script's fields: decoded by the text layer open(path) uses, then line.rstrip().split(). (A bare
    carriage return would make two lines of it; ds_eval_locate sends a file that holds one to the cpu route whole.)"""
    return "".join(io.TextIOWrapper(io.BytesIO(raw + b"\n"))).rstrip().split()


class _Calls(tr.RowFile):
    """One input file of the gpu route: its bytes, the row spans and the per-row flags."""

    def __init__(self, path: str, eng):
        tr.RowFile.__init__(self, path)
        begin, end, flags, file_flags = eng.eval_locate(self.data)
        if file_flags & eng.EVAL_BARE_CR:
            raise _CpuRoute("%s holds a bare carriage return, which ends a line in Python's text mode" % path)
        self.set_rows(begin, end, flags)


def evaluate_gpu(unmethylated: str, methylated: str, result_file: str, num_sites: int = NUM_SITES, rng=random, device: int = 0,
                 batch_rows: int = 1 << 20, info: Optional[dict] = None, make_engine=None) -> None:
    """evaluate_cpu on the GPU: the same file and the same stdout. Raises what the cpu route raises on a malformed row, after the
    same stdout. _CpuRoute, before anything is printed or drawn from `rng`: the input cannot be taken as it is; the message says
    why. `info`, when given, receives host_rows, rows and the device times. make_engine: what provides eval_begin .. eval_end
    (default: an Engine on `device`; the tests put the CPU checker behind it)."""
    from . import engine as eng
    tr.check_batch_rows(batch_rows)
    files = [_Calls(path, eng) for path in (unmethylated, methylated)]
    total = files[0].n + files[1].n
    if total > eng.FREQ_MAX_ROWS:
        raise _CpuRoute("more than 2^30 rows")
    host_rows, times = 0, {}
    sets: List[Optional[SetStats]] = [None, None]
    if total:
        with tr.small_engine(make_engine, device) as e:
            with tr.fits("the score table of %d rows does not fit the device" % total):
                e.eval_begin(total, min(batch_rows, total), PROB_CFS)
            picks = sample_rows(files[0].n, files[1].n, num_sites, rng)
            finite = [True, True]                     # per set: no NaN or infinite prob_1 among the rows read here
            set_bits = (eng.EVAL_SET_SAMPLE, eng.EVAL_SET_ALL)
            for f, pick, truth in zip(files, picks, (0, eng.EVAL_TRUTH)):
                # a row's byte: in the _N sample, in all_sites, from --methylated
                mask = numpy.full(f.n, eng.EVAL_SET_ALL | truth, numpy.uint8)
                mask[pick] |= eng.EVAL_SET_SAMPLE

                def host_row(row: int, _status: int):
                    prob_0, prob_1, label = row_values(_python_fields(f.row_bytes(row)))
                    if not math.isfinite(prob_1):
                        for k, bit in enumerate(set_bits):
                            if mask[row] & bit:
                                finite[k] = False
                    return prob_0, prob_1, int(label != 0)

                host_rows += tr.walk(f.n, batch_rows, lambda s, t: e.eval_parse(f.data, f.begin[s:t], f.end[s:t], f.flags[s:t]), host_row,
                                     lambda s, t, rows, values: e.eval_accumulate(mask[s:t], rows, *tr.columns(values, 3)))
                print(MSG_TOTAL.format(f.n))
            res, times = tr.finish(e, "eval")
        tr.check_rows(res, total)
        ncf = len(PROB_CFS)
        for k in range(2):
            c = res["counts"][k]
            if finite[k] and (res["p"][k], res["n"][k]) != (c[0] + c[3], c[1] + c[2]):
                raise RuntimeError("gpu route: the score table holds %d + %d rows of set %d, the counters %d + %d"
                                   % (res["p"][k], res["n"][k], k, c[0] + c[3], c[1] + c[2]))
            sets[k] = SetStats(c[0], c[1], c[2], c[3], c[4:4 + ncf], c[4 + ncf:4 + 2 * ncf],
                               auc_value(res["u2"][k], c[0] + c[3], c[1] + c[2], finite[k]))
    else:
        for f in files:
            print(MSG_TOTAL.format(f.n))
    if info is not None:
        info.update(host_rows=host_rows, rows=total, **times)
    print("--on gpu: %d of %d rows read by Python" % (host_rows, total), file=sys.stderr)
    empty = SetStats(0, 0, 0, 0, [0] * len(PROB_CFS), [0] * len(PROB_CFS), 0)
    write_result(result_file, num_sites, lambda: sets[0] or empty, lambda: sets[1] or empty)


def evaluate(unmethylated: str, methylated: str, result_file: str, on: str = "cpu", device: int = 0, num_sites: int = NUM_SITES,
             seed: Optional[int] = None, info: Optional[dict] = None) -> None:
    """Evaluate the two call files and write the table. seed: the sample comes from a random.Random(seed) of its own; None: from
    the global `random`, as in the script."""
    def rng():
        return random if seed is None else random.Random(seed)
    if on == "gpu":
        try:
            return evaluate_gpu(unmethylated, methylated, result_file, num_sites, rng(), device, info=info)
        except _CpuRoute as exc:
            print("--on gpu: {}; running the cpu route..".format(exc), file=sys.stderr)
    evaluate_cpu(unmethylated, methylated, result_file, num_sites, rng())


def add_arguments(ap) -> None:
    ap.add_argument("--unmethylated", type=str, required=True, help="call_mods results of an unmethylated sample")
    ap.add_argument("--methylated", type=str, required=True, help="call_mods results of a fully methylated sample")
    ap.add_argument("--result_file", type=str, required=True, help="a file path to save the evaluation result")
    ap.add_argument("--on", default="cpu", choices=["cpu", "gpu"],
                    help="gpu: rows parsed, counted and their scores ranked on the GPU (the host only finds the rows); same output "
                         "bytes")
    ap.add_argument("--device", type=int, default=None, help="GPU ordinal of --on gpu (default 0)")
    ap.add_argument("--num_sites", type=int, default=NUM_SITES, help="calls sampled from each file for the _N rows (default 100000)")
    ap.add_argument("--seed", type=int, default=None, help="seed of the sample (default: the global random state, as the script)")


def check_arguments(ap, a) -> None:
    if a.device is not None and a.on != "gpu":
        ap.error("--device needs --on gpu")
    if a.device is not None and a.device < 0:
        ap.error("--device must be >= 0")
    if a.num_sites < 0:
        ap.error("--num_sites must be >= 0")


def run(a) -> int:
    evaluate(a.unmethylated, a.methylated, a.result_file, a.on, a.device or 0, a.num_sites, a.seed)
    return 0


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description="Calculate call accuracy stats of nn results for cpgs")
    add_arguments(ap)
    a = ap.parse_args(argv)
    check_arguments(ap, a)
    return run(a)


if __name__ == "__main__":
    sys.exit(main())
