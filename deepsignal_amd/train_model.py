"""`deepsignal train`: fit a model on a training file, validate it on a second one, and save the best parameters as TensorFlow
checkpoints -- the reference's train module (train_model.py:24-285) restated statement for statement, with the steps and the
validation passes on the GPU (Engine.train_step / Engine.train_eval, csrc/ds_train.hip; Engine.train_step_signal /
Engine.train_eval_signal, csrc/ds_train_signal.hip).

What is trained: the variants with one sub-model. `--is_cnn no --is_rnn yes` with `--is_base yes` (embedding + BiLSTM, the
reference's "RNN-only" model) or `--is_base no` (what `denoise` trains); and `--is_cnn yes --is_rnn no`, the signal model alone
feeding the joint layers (`--is_base` is ignored, as in the reference). `--is_cnn yes --is_rnn yes` is the reference's default and
a usage error here: joined to the BiLSTM the signal model has no backward in this release.

The loop is the reference's: per epoch the learning rate (epochs 0 and 1: --learning_rate, later ones times --decay_rate), a
shuffle through a window of 3 x batch_size rows (tf.data's shuffle), per batch accuracy / recall / precision; every
--display_step iterations a line in train.txt, a pass over the validation file in file order (training = False, keep_prob 1), a
line in valid.txt, the save rule, the `epoch: ...` line, and both sets of running metrics start over. The save rule with its
quirk: a display saves iff its mean validation accuracy exceeds the best of THIS epoch so far and that new epoch best exceeds
`test_accu_best` -- which only moves at the end of an epoch, so within an epoch every new epoch best above the previous epochs'
best is saved over the same `epoch_<id>` prefix. Training stops after an epoch that did not improve the best once
epoch_id >= min_epoch_num - 1.

What is done differently. The training file is read ONCE and held in memory (the reference streams it through tf.data every
epoch): about 4 x (4 x kmer_len + cent_signals_len) bytes a row (1.7 KB at the defaults), so a few million rows are fine and the reference's "up to 20m" samples are out of
scope. The batch metrics are computed here (no scikit-learn; a zero denominator gives 0). TensorFlow's random draws
(initialisation, dropout, shuffle) are not reproduced, their distributions are; with --seed every draw derives from it and two
runs write identical files. A save writes `bn_<k>.sn_<s>.epoch_<id>.ckpt` (.index + .data-00000-of-00001) with the variant's
tensors under the reference graph's names and `modelglobal_step`, and the `checkpoint` state file; like tf.train.Saver's default
it keeps the five most recent prefixes. The BiLSTM variants' checkpoints are for this project's `call_mods -m <prefix> --is_cnn no
[--is_base no]`; the reference's own graph always creates the signal model's variables, which they do not hold. A save of the
signal-only variant holds all of its tensors, the batch norms' moving statistics included, so `call_mods -m <prefix> --is_rnn no`
reads it; the zero-debias helper variables that TensorFlow keeps beside each moving mean (`.../biased`, `.../local_step`) are NOT
written: a TensorFlow run that resumed from such a checkpoint would have to start them over.

The device part is an object with begin / step / eval / weights (GpuDevice); `train()` takes it as an argument, so the workflow
runs without a GPU under a stand-in (tests/test_train_host.py)."""
from __future__ import annotations

import argparse
import os
import random
import re
import sys
import time
from typing import Dict, List, Optional, Tuple

import numpy as np

if __package__ in (None, ""):                       # run as a script: the package is the directory above
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import deepsignal_amd  # noqa: F401
    __package__ = "deepsignal_amd"

from .denoise import batch_metrics, windowed_shuffle
from .utils.process_utils import display_args, str2bool

Rows = Dict[str, np.ndarray]      # kmer int32[n, T], means / stds / sanums float32[n, T], signals float32[n, S], labels int32[n]
MAX_TO_KEEP = 5                   # tf.train.Saver's default
SCOPE_NOTE = ("The training file is read once and held in memory: a few million rows, not the 20m the reference streams. "
              "Trains --is_cnn no --is_rnn yes with --is_base yes or no, and --is_cnn yes --is_rnn no (the signal model alone); "
              "joined to the BiLSTM the signal model's backward is not implemented.")


def read_rows(path: str, kmer_len: int, signal_len: int) -> Rows:
    """A feature file through the native TSV reader, as denoise.read_features reads it, plus the k-mer codes and the signals."""
    from .fastio import FeatureReader
    reader = FeatureReader(path, kmer_len, signal_len)
    parts: Dict[str, List[np.ndarray]] = {"kmer": [], "means": [], "stds": [], "sanums": [], "signals": [], "labels": []}
    try:
        for item in reader.items(200):
            parts["kmer"].append(item.kmer)
            parts["means"].append(item.means)
            parts["stds"].append(item.stds)
            parts["sanums"].append(item.lens)
            parts["signals"].append(item.signals)
            parts["labels"].append(item.labels)
    finally:
        reader.close()
    if not parts["labels"]:
        raise ValueError("%s holds no feature row" % path)
    return {k: np.concatenate(v) for k, v in parts.items()}


def take(rows: Rows, idx) -> Rows:
    return {k: v[idx] for k, v in rows.items()}


class GpuDevice:
    """The model on one engine handle: begin (fresh parameters), step, eval (training = False), weights (for a save). The variant
    follows the flags: the signal model alone (--is_cnn yes --is_rnn no), or a BiLSTM variant."""

    def __init__(self, args):
        from .engine import Engine
        self.args = args
        self.signal_only = str2bool(args.is_cnn) and not str2bool(args.is_rnn)
        self.is_base = str2bool(args.is_base) and not self.signal_only
        self.engine = Engine(kmer_len=args.kmer_len, signal_len=args.cent_signals_len, class_num=2, device=args.device or 0,
                             max_batch=args.batch_size, is_cnn=self.signal_only, is_rnn=not self.signal_only, is_base=self.is_base)

    def begin(self, init_seed: int, mask_seed: int) -> None:
        from . import weights
        a = self.args       # glorot-uniform kernels, zero LSTM bias, truncated-normal embedding: the reference's initialisers
        if self.signal_only:      # ... and batch_norm's: gamma 1, beta 0, moving mean 0, moving variance 1
            init = weights.random_weights(seed=init_seed, kmer_len=a.kmer_len, signal_len=a.cent_signals_len, is_cnn=True, is_rnn=False,
                                          randomize_bn=False)
        else:
            init = weights.random_weights(seed=init_seed, kmer_len=a.kmer_len, signal_len=a.cent_signals_len, is_cnn=False, is_rnn=True,
                                          is_base=self.is_base)
        self.engine.load_weights(init)
        self.engine.train_begin(keep_prob=a.keep_prob, pos_weight=a.pos_weight, seed=mask_seed, base=True)

    def step(self, rows: Rows, lr: float) -> Tuple[float, np.ndarray]:
        if self.signal_only:
            return self.engine.train_step_signal(rows["signals"], rows["labels"], lr)
        return self.engine.train_step(rows["means"], rows["stds"], rows["sanums"], rows["labels"], lr, kmer=rows["kmer"])

    def eval(self, rows: Rows) -> Tuple[float, np.ndarray]:
        if self.signal_only:
            loss, pred, _ = self.engine.train_eval_signal(rows["signals"], rows["labels"])
        else:
            loss, pred, _ = self.engine.train_eval(rows["means"], rows["stds"], rows["sanums"], rows["labels"], kmer=rows["kmer"])
        return loss, pred

    def weights(self) -> Dict[str, np.ndarray]:
        return self.engine.train_tensors()      # the signal-only variant: the moving statistics too

    def close(self) -> None:
        self.engine.close()


# ---- saving (saver.save of train_model.py:242-243) -----------------------------------------------------------------------------
class Saver:
    """tf.train.Saver().save into one directory: the checkpoint, then the `checkpoint` state file naming the latest prefix and
    the (at most MAX_TO_KEEP) prefixes kept, oldest first; a prefix that falls out of that list is deleted."""

    def __init__(self, model_dir: str):
        self.model_dir = model_dir
        self.kept: List[str] = []

    def save(self, name: str, tensors: Dict[str, np.ndarray], global_step: int) -> str:
        from . import tf_checkpoint
        prefix = os.path.join(self.model_dir, name)
        out = dict(tensors)
        out["modelglobal_step"] = np.array(global_step, np.int32)
        tf_checkpoint.write_checkpoint(prefix, out)
        if name in self.kept:
            self.kept.remove(name)
        self.kept.append(name)
        while len(self.kept) > MAX_TO_KEEP:
            old = os.path.join(self.model_dir, self.kept.pop(0))
            for path in (old + ".index", tf_checkpoint.shard_path(old, 0, 1)):
                if os.path.exists(path):
                    os.remove(path)
        with open(os.path.join(self.model_dir, "checkpoint"), "w") as f:
            f.write('model_checkpoint_path: "%s"\n' % name)
            for k in self.kept:
                f.write('all_model_checkpoint_paths: "%s"\n' % k)
        return prefix


def _mean(values) -> float:
    return float(np.mean(values))


# ---- the workflow (train_model.py:24-285) ----------------------------------------------------------------------------------------
def train(args, device=None) -> List[str]:
    """Runs the workflow; returns the prefix of every save in order. `device`: see the module docstring (default: the GPU)."""
    train_start = time.time()
    kmer_len, cent_signals_len, batch_size = args.kmer_len, args.cent_signals_len, args.batch_size
    model_dir = os.path.abspath(args.model_dir)
    log_dir = os.path.abspath(args.log_dir) if args.log_dir is not None else None

    model_regex = re.compile(r"bn_" + str(kmer_len) + r"\.sn_" + str(cent_signals_len) + r"\.epoch_\d+\.ckpt*")
    model_prefix = "bn_" + str(kmer_len) + ".sn_" + str(cent_signals_len) + ".epoch_"
    model_suffix = ".ckpt"
    if os.path.exists(model_dir):
        count = 0
        for mfile in os.listdir(model_dir):
            if model_regex.match(mfile) or mfile == "checkpoint":
                os.remove(model_dir + "/" + mfile)
                count += 1
        if count >= 1:
            print("the previous model ({} files) in model_directory deleted...".format(count))
    else:
        os.mkdir(model_dir)

    train_log_txt, valid_log_txt = "train.txt", "valid.txt"
    if log_dir is not None:
        if os.path.exists(log_dir):
            count = 0
            for name in (train_log_txt, valid_log_txt):
                if os.path.exists(log_dir + "/" + name):
                    os.remove(log_dir + "/" + name)
                    count += 1
            if count >= 1:
                print("the previous log file ({} files) in log_directory deleted...".format(count))
        else:
            os.mkdir(log_dir)

    train_rows = read_rows(os.path.abspath(args.train_file), kmer_len, cent_signals_len)
    valid_rows = read_rows(os.path.abspath(args.valid_file), kmer_len, cent_signals_len)
    n_train, n_valid = len(train_rows["labels"]), len(valid_rows["labels"])

    rng = random.Random(args.seed) if args.seed is not None else random.Random()
    init_seed, mask_seed = rng.getrandbits(32), rng.getrandbits(63)
    order_rng = np.random.default_rng(rng.getrandbits(64))
    own = None
    if device is None:
        own = device = GpuDevice(args)
    saver = Saver(model_dir)
    saved: List[str] = []
    try:
        device.begin(init_seed, mask_seed)
        global_step = 0
        test_accu_best = 0.0
        for epoch_id in range(args.max_epoch_num):
            start = time.time()
            if epoch_id == 0 or epoch_id == 1:
                epoch_learning_rate = args.learning_rate
            else:
                epoch_learning_rate = args.learning_rate * args.decay_rate

            train_accuracy_total, train_recall_total, train_precision_total, train_loss_total = [], [], [], []
            test_accu_best_ep = 0.0
            test_accuracy_total, test_recall_total, test_precision_total, test_loss_total = [], [], [], []
            iter_id = 0

            order = windowed_shuffle(n_train, batch_size * 3, order_rng)
            for b in range(0, n_train, batch_size):
                batch = take(train_rows, order[b:b + batch_size])
                train_loss, train_prediction = device.step(batch, epoch_learning_rate)
                global_step += 1
                accu_batch, precision_batch, recall_batch = batch_metrics(batch["labels"], train_prediction)
                train_loss_total.append(train_loss)
                train_accuracy_total.append(accu_batch)
                train_recall_total.append(recall_batch)
                train_precision_total.append(precision_batch)

                iter_id += 1
                if iter_id % args.display_step == 0:
                    if log_dir is not None:
                        with open(log_dir + "/" + train_log_txt, "a") as train_log:
                            train_log.write("epoch:%d, iterid:%d, loss:%.3f, accuracy:%.3f, recall:%.3f, precision:%.3f\n" %
                                            (epoch_id, iter_id, _mean(train_loss_total), _mean(train_accuracy_total),
                                             _mean(train_recall_total), _mean(train_precision_total)))

                    for v in range(0, n_valid, batch_size):
                        vbatch = take(valid_rows, slice(v, v + batch_size))
                        test_loss, test_prediction = device.eval(vbatch)
                        accu_batch, precision_batch, recall_batch = batch_metrics(vbatch["labels"], test_prediction)
                        test_loss_total.append(test_loss)
                        test_accuracy_total.append(accu_batch)
                        test_recall_total.append(recall_batch)
                        test_precision_total.append(precision_batch)

                    if log_dir is not None:
                        with open(log_dir + "/" + valid_log_txt, "a") as valid_log:
                            valid_log.write("epoch:%d, iterid:%d, loss:%.3f, accuracy:%.3f, recall:%.3f, precision:%.3f\n" %
                                            (epoch_id, iter_id, _mean(test_loss_total), _mean(test_accuracy_total),
                                             _mean(test_recall_total), _mean(test_precision_total)))

                    if _mean(test_accuracy_total) > test_accu_best_ep:
                        test_accu_best_ep = _mean(test_accuracy_total)
                        if test_accu_best_ep > test_accu_best:
                            saved.append(saver.save(model_prefix + str(epoch_id) + model_suffix, device.weights(), global_step))

                    end = time.time()
                    line = "epoch: %d, iterid: %d\n train_loss: %.3f, valid_loss: %.3f, train_accuracy: %.3f, " \
                           "valid_accuracy: %.3f, curr_epoch_best_accuracy: %.3f, " \
                           "time_cost: %.2fs" % (epoch_id, iter_id, _mean(train_loss_total), _mean(test_loss_total),
                                                 _mean(train_accuracy_total), _mean(test_accuracy_total), test_accu_best_ep, end - start)
                    sys.stdout.write(line + "\n")
                    sys.stdout.flush()

                    train_accuracy_total, train_recall_total, train_precision_total, train_loss_total = [], [], [], []
                    test_accuracy_total, test_recall_total, test_precision_total, test_loss_total = [], [], [], []
                    start = time.time()

            improved = test_accu_best_ep > test_accu_best
            if improved:
                test_accu_best = test_accu_best_ep
            sys.stdout.write("================ epoch %d best accuracy: %.3f, best accuracy: %.3f\n" % (epoch_id, test_accu_best_ep, test_accu_best))
            sys.stdout.flush()
            if not improved and epoch_id >= args.min_epoch_num - 1:
                break
    finally:
        if own is not None:
            own.close()
    sys.stdout.write("training finished, costs %.1f seconds..\n" % (time.time() - train_start))
    return saved


# ---- command line (train_model.py:288-346: the reference's flags and defaults) -------------------------------------------------
def add_arguments(ap) -> None:
    g = ap.add_argument_group("INPUT")
    g.add_argument("--train_file", action="store", type=str, required=True,
                   help="file contains samples for training, from extract_features.py. The file should contain shuffled positive "
                        "and negative samples. It is read once and held in memory, signals included: 4 x (4 x kmer_len + "
                        "cent_signals_len) bytes a row, 1.7 KB at the defaults (a few million rows; not the reference's 20m).")
    g.add_argument("--valid_file", action="store", type=str, required=True,
                   help="file contains samples for testing, from extract_features.py. For CpG, 10k (~5k positive and ~5k negative) "
                        "samples are sufficient.")
    g.add_argument("--is_binary", action="store", type=str, required=False, default="no", choices=["yes", "no"],
                   help="are the train_file and valid_file in binary format or not? default no. (yes is not implemented)")
    g = ap.add_argument_group("OUTPUT")
    g.add_argument("--model_dir", "-o", action="store", type=str, required=True, help="directory for saving the trained model")
    g.add_argument("--log_dir", "-g", action="store", type=str, required=False, default=None, help="directory for saving the training log")
    g = ap.add_argument_group("TRAIN")
    g.add_argument("--is_cnn", type=str, default="yes", required=False,
                   help="using inception module of deepsignal or not. yes trains with --is_rnn no (the signal model alone); with the "
                        "default --is_rnn yes it is not implemented (joined to the BiLSTM the signal model has no backward)")
    g.add_argument("--is_base", type=str, default="yes", required=False, help="using base features in BiLSTM module or not")
    g.add_argument("--is_rnn", type=str, default="yes", required=False, help="using BiLSTM module of deepsignal or not")
    g.add_argument("--kmer_len", "-x", action="store", default=17, type=int, required=False, help="base num of the kmer, default 17")
    g.add_argument("--cent_signals_len", "-y", action="store", default=360, type=int, required=False,
                   help="the number of central signals of the kmer to be used, default 360")
    g.add_argument("--batch_size", "-b", default=512, type=int, required=False, action="store", help="batch size, default 512")
    g.add_argument("--learning_rate", "-l", default=0.001, type=float, required=False, action="store", help="init learning rate, default 0.001")
    g.add_argument("--decay_rate", "-d", default=0.1, type=float, required=False, action="store", help="decay rate, default 0.1")
    g.add_argument("--class_num", "-c", action="store", default=2, type=int, required=False, help="class num, default 2")
    g.add_argument("--keep_prob", action="store", default=0.5, type=float, required=False, help="keep prob, default 0.5")
    g.add_argument("--max_epoch_num", action="store", default=10, type=int, required=False, help="max epoch num, default 10")
    g.add_argument("--min_epoch_num", action="store", default=5, type=int, required=False, help="min epoch num, default 5")
    g.add_argument("--display_step", action="store", default=100, type=int, required=False, help="display step, default 100")
    g.add_argument("--pos_weight", action="store", default=1.0, type=float, required=False,
                   help="pos_weight in loss function: tf.nn.weighted_cross_entropy_with_logits, for imbalanced training samples, "
                        "default 1. If |pos samples| : |neg samples| = 1:3, set pos_weight to 3.")
    g = ap.add_argument_group("RUN")
    g.add_argument("--seed", type=int, default=None,
                   help="every random choice (initialisation, dropout masks, shuffle) derives from it; default: unseeded, as the reference")
    g.add_argument("--device", type=int, default=None, help="GPU ordinal (default 0)")


def check_arguments(ap, a) -> None:
    try:
        is_cnn, is_base, is_rnn = str2bool(a.is_cnn), str2bool(a.is_base), str2bool(a.is_rnn)
    except Exception:
        ap.error("--is_cnn / --is_base / --is_rnn take yes or no")
    del is_base         # both values are trained (ignored without the BiLSTM)
    if is_cnn and is_rnn:
        ap.error("--is_cnn yes --is_rnn yes (the default) is not implemented: joined to the BiLSTM the signal model has no backward in "
                 "this release; pass --is_rnn no to train it alone, or --is_cnn no for the BiLSTM variants")
    if not is_rnn and not is_cnn:
        ap.error("--is_rnn no is not implemented: without the signal model the BiLSTM is all there is to train")
    if a.class_num != 2:
        ap.error("--class_num other than 2 is not implemented: the training step has the two-class loss only")
    if str2bool(a.is_binary):
        ap.error("--is_binary yes is not implemented: binary feature files are not read; pass the text feature files")
    if a.device is not None and a.device < 0:
        ap.error("--device must be >= 0")
    if not (0.0 < a.keep_prob <= 1.0):
        ap.error("--keep_prob must lie in (0, 1]")
    if not a.pos_weight > 0.0:
        ap.error("--pos_weight must be positive")
    for name in ("batch_size", "display_step", "max_epoch_num"):
        if getattr(a, name) < 1:
            ap.error("--%s must be at least 1" % name)
    if a.kmer_len < 1 or a.kmer_len % 2 == 0:
        ap.error("--kmer_len must be odd")


def run(a) -> int:
    display_args(a)
    train(a)
    return 0


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description="train a model, need two independent datasets for training and validating. " + SCOPE_NOTE)
    add_arguments(ap)
    a = ap.parse_args(argv)
    check_arguments(ap, a)
    return run(a)


if __name__ == "__main__":
    sys.exit(main())
