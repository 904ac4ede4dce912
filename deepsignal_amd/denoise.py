"""`deepsignal denoise`: clean the positive samples of a training file by cross-ranking -- the reference's denoise module
(denoise.py:187-345) restated, with the models trained and the rows scored on the GPU (Engine.train_step, csrc/ds_train.hip).

Per iteration the current training file is split at random into two halves `rounds` times; a fresh RNN-only model
(--is_cnn no --is_base no --is_rnn yes) is trained on one half and scores the other, then the reverse, so every row gets
`rounds` scores from models that never saw it. A positive row is kept iff the mean of its scores exceeds --score_cf; as many
negatives as kept positives are drawn from the label-0 rows so that their k-mer distribution follows the kept positives'
(process_utils.py:377-478), both are shuffled into `<name>.denoise<i><ext>`, and the loop ends when more than 99 % of the
positives were kept.

What is done differently, with the same result: the halves are read by the native TSV reader (no `.bin` conversion); the batch
metrics are computed here (no scikit-learn; a zero denominator gives 0, as sklearn's default does with a warning); the scratch
lists of the clean / re-balance step stay in memory instead of `<name>.pos.cf*` / `<name>.neg_all.r*` files. TensorFlow's random
draws (initialisation, dropout, shuffle) are not reproduced: the distributions are. With --seed every draw derives from it and two
runs write identical files.

The training-and-scoring part is a callable `scorer(train_file, score_file, tag) -> float32 scores of score_file's rows`;
`denoise()` takes it as an argument, so the file workflow runs without a GPU under a stand-in (tests/test_denoise_host.py)."""
from __future__ import annotations

import argparse
import math
import os
import random
import sys
import time
from typing import Callable, Dict, List, Optional, Sequence, Tuple

import numpy as np

if __package__ in (None, ""):                       # run as a script: the package is the directory above
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import deepsignal_amd  # noqa: F401
    __package__ = "deepsignal_amd"

from .utils.process_utils import display_args, str2bool

Scorer = Callable[[str, str, str], np.ndarray]
RNN_ONLY_MESSAGE = ("this release trains the RNN-only model: --is_cnn no --is_base no --is_rnn yes --layer_num 3 --class_num 2 "
                    "(the signal model's backward and the embedding gradient are not implemented)")


# ---- file helpers (process_utils.py:236-279, 320-352, 377-478 restated) --------------------------------------------------------
def _read_lines(path: str) -> List[str]:
    with open(path, "r") as f:
        return f.readlines()


def _label(line: str) -> int:
    return int(line.strip().split("\t")[-1])


def _kmer(line: str) -> str:
    return line.strip().split("\t")[6]


def write_negatives(train_file: str) -> str:
    """`<name>.neg_all<ext>`: the label-0 rows, in file order."""
    fname, fext = os.path.splitext(train_file)
    out = fname + ".neg_all" + fext
    with open(out, "w") as wf:
        for line in _read_lines(train_file):
            if _label(line) == 0:
                wf.write(line)
    return out


def split_rows(lines: Sequence[str], file1: str, file2: str, half_num: int, rng: random.Random) -> Tuple[List[int], List[int]]:
    """half_num rows chosen at random go to file1, the rest to file2, both in file order; returns every row's index per file."""
    chosen = set(rng.sample(range(len(lines)), min(half_num, len(lines))))
    idx1, idx2 = [], []
    with open(file1, "w") as w1, open(file2, "w") as w2:
        for i, line in enumerate(lines):
            if i in chosen:
                w1.write(line)
                idx1.append(i)
            else:
                w2.write(line)
                idx2.append(i)
    return idx1, idx2


def select_negatives(pos_lines: Sequence[str], neg_lines: Sequence[str], rng: random.Random) -> List[int]:
    """Indices into neg_lines, ascending: per k-mer (column 7) of the positives ceil(total * ratio) negatives of that k-mer, all of
    them if fewer exist; what is still missing is spread over the negatives' k-mers that no positive has."""
    total = len(pos_lines)
    count: Dict[str, int] = {}
    for line in pos_lines:
        count[_kmer(line)] = count.get(_kmer(line), 0) + 1
    by_kmer: Dict[str, List[int]] = {}
    for i, line in enumerate(neg_lines):
        by_kmer.setdefault(_kmer(line), []).append(i)
    selected: List[int] = []
    others: List[str] = []
    short = 0
    for kmer, rows in by_kmer.items():
        if kmer not in count:
            others.append(kmer)
            continue
        want = int(math.ceil(total * (float(count[kmer]) / total)))
        if len(rows) <= want:
            selected += rows
            short += want - len(rows)
        else:
            selected += rng.sample(rows, want)
    print("for {} common kmers, fill {} samples, {} samples that can't filled".format(len(by_kmer) - len(others), len(selected), short))
    unfilled = total - len(selected)
    print("totalline: {}, need to fill: {}".format(total, unfilled))
    if others:
        each = max(0, int(math.ceil(float(unfilled) / len(others))))
        got = 0
        for kmer in others:
            rows = by_kmer[kmer]
            take = rows if len(rows) <= each else rng.sample(rows, each)
            selected += take
            got += len(take)
        print("extract {} samples from {} diff kmers".format(got, len(others)))
    return sorted(selected)


def write_shuffled(lines: Sequence[str], path: str, rng: random.Random) -> None:
    rows = [line.strip() for line in lines]
    rng.shuffle(rows)
    with open(path, "w") as wf:
        for row in rows:
            wf.write(row + "\n")


# ---- metrics of a batch, by hand ---------------------------------------------------------------------------------------------
def batch_metrics(labels: np.ndarray, pred: np.ndarray) -> Tuple[float, float, float]:
    """(accuracy, precision, recall) of the positive class; a zero denominator gives 0."""
    labels, pred = np.asarray(labels), np.asarray(pred)
    tp = int(np.sum((labels == 1) & (pred == 1)))
    fp = int(np.sum((labels == 0) & (pred == 1)))
    fn = int(np.sum((labels == 1) & (pred == 0)))
    accuracy = float(np.mean(labels == pred)) if len(labels) else 0.0
    return accuracy, (tp / (tp + fp) if tp + fp else 0.0), (tp / (tp + fn) if tp + fn else 0.0)


def windowed_shuffle(n: int, buffer_size: int, rng: np.random.Generator) -> np.ndarray:
    """The order tf.data's shuffle(buffer_size) yields n elements in: a buffer of the next buffer_size elements, one drawn at
    random and replaced by the following element, until both run out."""
    order = np.empty(n, np.int64)
    buf = list(range(min(max(1, buffer_size), n)))
    nxt = len(buf)
    for k in range(n):
        j = int(rng.integers(len(buf)))
        order[k] = buf[j]
        if nxt < n:
            buf[j] = nxt
            nxt += 1
        else:
            buf[j] = buf[-1]
            buf.pop()
    return order


def read_features(path: str, kmer_len: int, signal_len: int) -> Dict[str, np.ndarray]:
    """means / stds / sanums float32[n, kmer_len] and labels int32[n] of a feature file, through the native TSV reader."""
    from .fastio import FeatureReader
    reader = FeatureReader(path, kmer_len, signal_len)
    parts: Dict[str, List[np.ndarray]] = {"means": [], "stds": [], "sanums": [], "labels": []}
    try:
        for item in reader.items(200):
            parts["means"].append(item.means)
            parts["stds"].append(item.stds)
            parts["sanums"].append(item.lens)
            parts["labels"].append(item.labels)
    finally:
        reader.close()
    if not parts["labels"]:
        return {"means": np.zeros((0, kmer_len), np.float32), "stds": np.zeros((0, kmer_len), np.float32),
                "sanums": np.zeros((0, kmer_len), np.float32), "labels": np.zeros((0,), np.int32)}
    return {k: np.concatenate(v) for k, v in parts.items()}


class GpuScorer:
    """Trains a fresh RNN-only model on one file and scores another: one engine handle per run, re-initialised per model
    (denoise.py:33-184 restated)."""

    def __init__(self, args, rng: random.Random):
        from .engine import Engine
        self.args, self.rng = args, rng
        self.engine = Engine(kmer_len=args.seq_len, signal_len=args.cent_signals_len, class_num=2, device=args.device or 0,
                             max_batch=args.batch_size, is_cnn=False, is_rnn=True, is_base=False)
        self.loaded = False

    def close(self) -> None:
        self.engine.close()

    def __call__(self, train_file: str, score_file: str, tag: str) -> np.ndarray:
        from . import weights
        a, eng = self.args, self.engine
        train = read_features(train_file, a.seq_len, a.cent_signals_len)
        init = weights.random_weights(seed=self.rng.getrandbits(32), kmer_len=a.seq_len, signal_len=a.cent_signals_len,
                                      is_cnn=False, is_rnn=True, is_base=False)        # glorot-uniform kernels, zero LSTM bias
        mask_seed = self.rng.getrandbits(63)
        order_rng = np.random.default_rng(self.rng.getrandbits(64))
        if not self.loaded:
            eng.load_weights(init)
            self.loaded = True
            eng.train_begin(keep_prob=a.keep_prob, pos_weight=a.pos_weight, seed=mask_seed)
        else:
            eng.train_begin(keep_prob=a.keep_prob, pos_weight=a.pos_weight, seed=mask_seed, weights=init)
        n = len(train["labels"])
        for epoch in range(a.epoch_num):
            start = time.time()
            lr = a.lr if epoch < 2 else a.lr * a.decay_rate
            order = windowed_shuffle(n, a.batch_size * 3, order_rng)
            accus = []
            for it, b in enumerate(range(0, n, a.batch_size), start=1):
                rows = order[b:b + a.batch_size]
                labels = train["labels"][rows]
                loss, pred = eng.train_step(train["means"][rows], train["stds"][rows], train["sanums"][rows], labels, lr)
                if it % a.step_interval == 0:
                    accu, prec, reca = batch_metrics(labels, pred)
                    accus.append(accu)
                    print("Epoch [{}/{}], Step {}, Loss: {:.4f}, Accuracy: {:.4f}, Precision: {:.4f}, Recall: {:.4f}, Time: {:.2f}s"
                          .format(epoch + 1, a.epoch_num, it, loss, accu, prec, reca, time.time() - start))
                    sys.stdout.flush()
                    start = time.time()
            # (the mean of no accuracies is NaN and compares false, as np.mean([]) does in the reference)
            if (sum(accus) / len(accus) if accus else float("nan")) >= 0.95:
                break
        # score the other file with the inference forward on the trained parameters
        eng.train_sync_weights()
        valid = read_features(score_file, a.seq_len, a.cent_signals_len)
        m = len(valid["labels"])
        scores = np.empty(m, np.float32)
        zeros_k = np.zeros((a.batch_size, a.seq_len), np.int32)
        zeros_s = np.zeros((a.batch_size, a.cent_signals_len), np.float32)
        stats = []
        for b in range(0, m, a.batch_size):
            e = min(m, b + a.batch_size)
            act, pred = eng.run(zeros_k[:e - b], valid["means"][b:e], valid["stds"][b:e], valid["sanums"][b:e], zeros_s[:e - b])
            scores[b:e] = act[:, 1]
            stats.append(batch_metrics(valid["labels"][b:e], pred))
        if stats:
            print("===Test, Total Accuracy: {:.4f}, Precision: {:.4f}, Recall: {:.4f}".format(*np.mean(np.array(stats), axis=0)))
        sys.stdout.flush()
        return scores


# ---- the workflow (denoise.py:187-345) ---------------------------------------------------------------------------------------
def cross_rank(train_file: str, iterstr: str, args, scorer: Scorer, rng: random.Random) -> np.ndarray:
    """float32 scores [rounds, rows]: per round every row is scored once, by the model trained on the half it is not in."""
    print("\n##########Train Cross Rank##########")
    lines = _read_lines(train_file)
    total = len(lines)
    if total < 2:
        raise ValueError("%s: a training file needs at least two rows" % train_file)
    fname, fext = os.path.splitext(train_file)
    file1, file2 = fname + ".half1" + fext, fname + ".half2" + fext
    scores = np.empty((args.rounds, total), np.float32)
    for r in range(args.rounds):
        print("##########Train Cross Rank, Iter {}, Round {}##########".format(iterstr, r + 1))
        idx1, idx2 = split_rows(lines, file1, file2, total // 2, rng)
        try:
            print("##########Train Cross Rank, Iter {}, Round {}, part1##########".format(iterstr, r + 1))
            s2 = np.asarray(scorer(file1, file2, iterstr + str(r) + "1"), np.float32)
            print("##########Train Cross Rank, Iter {}, Round {}, part2##########".format(iterstr, r + 1))
            s1 = np.asarray(scorer(file2, file1, iterstr + str(r) + "2"), np.float32)
        finally:
            os.remove(file1)
            os.remove(file2)
        if s1.shape != (len(idx1),) or s2.shape != (len(idx2),):
            raise ValueError("the scorer returned %d / %d scores for halves of %d / %d rows" % (len(s1), len(s2), len(idx1), len(idx2)))
        scores[r, idx1] = s1
        scores[r, idx2] = s2
    print("##########Train Cross Rank, finished!##########")
    sys.stdout.flush()
    return scores


def score_stats(scores: np.ndarray) -> Tuple[np.ndarray, np.ndarray]:
    """Per row the mean of its scores (float32 sum in round order, then one division, as sum(probs) / len(probs) of float32
    scores) and their population standard deviation."""
    s = np.zeros(scores.shape[1], np.float32)
    for r in range(scores.shape[0]):
        s = (s + scores[r]).astype(np.float32)
    return s.astype(np.float64) / scores.shape[0], np.std(scores, axis=0).astype(np.float64)


def denoise(args, scorer: Optional[Scorer] = None) -> str:
    """Runs the workflow and returns the final file's path. `scorer`: see the module docstring (default: the GPU)."""
    total_start = time.time()
    rng = random.Random(args.seed) if args.seed is not None else random.Random()
    own = None
    if scorer is None:
        own = scorer = GpuScorer(args, rng)
    scores_out = open(args.scores_file, "w") if getattr(args, "scores_file", None) else None
    neg_file = write_negatives(args.train_file)
    train_file = args.train_file
    try:
        neg_lines = _read_lines(neg_file)
        for it in range(args.iterations):
            print("\n###### cross rank to clean samples, Iter: {} ######".format(it + 1))
            scores = cross_rank(train_file, str(it + 1), args, scorer, rng)
            mean, std = score_stats(scores)
            print("\n######clean the samples######")
            lines = _read_lines(train_file)
            labels = [_label(line) for line in lines]
            if scores_out:
                for i, lab in enumerate(labels):
                    scores_out.write("%d\t%d\t%d\t%r\t%r\n" % (it + 1, i, lab, float(mean[i]), float(std[i])))
                scores_out.flush()
            pos = [i for i, lab in enumerate(labels) if lab == 1]
            print("There are {} positive, {} negative samples in total;".format(len(pos), len(labels) - len(pos)))
            if not pos:
                raise ValueError("%s holds no positive sample" % train_file)
            kept = [lines[i] for i in pos if mean[i] > args.score_cf]
            left_ratio = float(len(kept)) / len(pos)
            print("{} ({}) high quality positive samples left, {} high quality negative samples left".format(len(kept), left_ratio, 0))
            print("######clean the samples, finished!######")
            if train_file != args.train_file:
                os.remove(train_file)
            print("\n#####concat denoised file#####")
            chosen = select_negatives(kept, neg_lines, rng) if kept else []
            fname, fext = os.path.splitext(args.train_file)
            train_file = fname + ".denoise" + str(it + 1) + fext
            write_shuffled(kept + [neg_lines[i] for i in chosen], train_file, rng)
            print("#####concat denoised file, finished!#####")
            sys.stdout.flush()
            if left_ratio > 0.99:
                break
            if len(kept) + len(chosen) < 2:
                print("###### fewer than two samples left: nothing to cross rank, stopping here")
                break
    finally:
        os.remove(neg_file)
        if scores_out:
            scores_out.close()
        if own is not None:
            own.close()
    print("###### training totally costs {:.2f} seconds".format(time.time() - total_start))
    print("###### denoised file for training: {}".format(train_file))
    return train_file


# ---- command line (deepsignal.py:389-418: the reference's flags and defaults) --------------------------------------------------
def add_arguments(ap) -> None:
    g = ap.add_argument_group("INPUT")
    g.add_argument("--train_file", type=str, required=True)
    g = ap.add_argument_group("TRAIN")
    g.add_argument("--model_prefix", type=str, default="model", required=False)
    g.add_argument("--is_cnn", type=str, default="no", required=False)
    g.add_argument("--is_base", type=str, default="no", required=False)
    g.add_argument("--is_rnn", type=str, default="yes", required=False)
    g.add_argument("--seq_len", type=int, default=17, required=False)
    g.add_argument("--cent_signals_len", type=int, default=360, required=False)
    g.add_argument("--layer_num", type=int, default=3, required=False)
    g.add_argument("--class_num", type=int, default=2, required=False)
    g.add_argument("--batch_size", type=int, default=512, required=False)
    g.add_argument("--lr", type=float, default=0.001, required=False, help="learning rate")
    g.add_argument("--decay_rate", type=float, default=0.1, required=False)
    g.add_argument("--keep_prob", action="store", default=0.5, type=float, required=False, help="keep prob, default 0.5")
    g.add_argument("--pos_weight", type=float, default=1.0, required=False)
    g.add_argument("--iterations", type=int, default=6, required=False)
    g.add_argument("--epoch_num", type=int, default=5, required=False)
    g.add_argument("--step_interval", type=int, default=100, required=False)
    g.add_argument("--rounds", type=int, default=5, required=False)
    g.add_argument("--score_cf", type=float, default=0.5, required=False, help="score cutoff")
    g = ap.add_argument_group("RUN")
    g.add_argument("--seed", type=int, default=None,
                   help="every random choice (split, shuffle, initialisation, dropout masks, negative selection) derives from it; "
                        "default: unseeded, as the reference")
    g.add_argument("--device", type=int, default=None, help="GPU ordinal (default 0)")
    g.add_argument("--scores_file", type=str, default=None,
                   help="per iteration one row per training-file row: iteration, row index, label, mean and population standard "
                        "deviation of its cross-rank scores")


def check_arguments(ap, a) -> None:
    try:
        variant = (str2bool(a.is_cnn), str2bool(a.is_base), str2bool(a.is_rnn))
    except Exception:
        ap.error("--is_cnn / --is_base / --is_rnn take yes or no")
    if variant != (False, False, True) or a.layer_num != 3 or a.class_num != 2:
        ap.error(RNN_ONLY_MESSAGE)
    if a.device is not None and a.device < 0:
        ap.error("--device must be >= 0")
    if not (0.0 < a.keep_prob <= 1.0):
        ap.error("--keep_prob must lie in (0, 1]")
    if not a.pos_weight > 0.0:
        ap.error("--pos_weight must be positive")
    for name in ("batch_size", "iterations", "epoch_num", "step_interval", "rounds"):
        if getattr(a, name) < 1:
            ap.error("--%s must be at least 1" % name)
    if a.seq_len < 1 or a.seq_len % 2 == 0:
        ap.error("--seq_len must be odd")


def run(a) -> int:
    display_args(a)
    denoise(a)
    return 0


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description="denoise training samples by deep-learning, filter false positive samples")
    add_arguments(ap)
    a = ap.parse_args(argv)
    check_arguments(ap, a)
    return run(a)


if __name__ == "__main__":
    sys.exit(main())
