"""GPU: `deepsignal train` end to end on generated files, both trained variants: a checkpoint is written, `call_mods -m <it>
--is_cnn no` calls the validation file as ds_train_eval does on the saved parameters (wherever the float64 statement's logit gap
exceeds the gradient test's loss bar), and the validation loss falls."""
import os
import re

import numpy as np
import pytest
import torch

import denoise_cases as dc
import train_statement as ts
import train_statement_base as tsb

pytestmark = pytest.mark.gpu

T, S = 17, 16


def _write(path, n, seed):
    """Rows whose label a (mean, k-mer) rule decides: label 1 has its means shifted up and a C in the centre of the k-mer,
    label 0 has them shifted down and a T there."""
    rng = np.random.default_rng(seed)
    rows = []
    for i in range(n):
        label = int(rng.integers(0, 2))
        kmer = "".join("ACGT"[b] for b in rng.integers(0, 4, T))
        kmer = kmer[:T // 2] + ("C" if label else "T") + kmer[T // 2 + 1:]
        rows.append(dc._row(i, "r", kmer, label, rng, T, S, 1.0 if label else -0.5))
    with open(path, "w") as f:
        f.writelines(rows)


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    d = tmp_path_factory.mktemp("train_cli")
    _write(d / "train.tsv", 600, 1)
    _write(d / "valid.tsv", 200, 2)
    return d


@pytest.mark.parametrize("is_base", ["yes", "no"])
def test_train_saves_what_call_mods_then_calls_with(files, is_base, capsys):
    from deepsignal_amd import deepsignal, tf_checkpoint, train_model
    from deepsignal_amd.engine import Engine
    model, log = files / ("model_" + is_base), files / ("log_" + is_base)
    rc = deepsignal.main(["train", "--train_file", str(files / "train.tsv"), "--valid_file", str(files / "valid.tsv"), "-o", str(model),
                          "-g", str(log), "--is_cnn", "no", "--is_base", is_base, "-x", str(T), "-y", str(S), "--batch_size", "64",
                          "--display_step", "2", "--max_epoch_num", "2", "--min_epoch_num", "1", "--seed", "3"])
    out = capsys.readouterr().out
    assert not rc and "training finished" in out
    state = open(model / "checkpoint").read()
    name = re.match(r'model_checkpoint_path: "(bn_17\.sn_16\.epoch_\d\.ckpt)"\n', state).group(1)
    prefix = str(model / name)
    assert tf_checkpoint.is_checkpoint(prefix) and os.path.exists(prefix + ".data-00000-of-00001")
    variant = dict(is_cnn=False, is_rnn=True, is_base=is_base == "yes")
    saved = tf_checkpoint.checkpoint_to_weights(prefix, kmer_len=T, signal_len=S, **variant)
    assert ("modelembedding" in saved) == variant["is_base"]
    steps = int(tf_checkpoint.load_checkpoint(prefix, ["modelglobal_step"])["modelglobal_step"])
    assert 2 <= steps <= 20 and steps % 2 == 0

    # the validation loss of the last display is below that of the first
    losses = [float(re.search(r"loss:(-?\d+\.\d+)", line).group(1)) for line in open(log / "valid.txt")]
    assert len(losses) == 10 and len(open(log / "train.txt").readlines()) == 10
    print("validation losses", losses)
    assert losses[-1] < losses[0]

    # call_mods with the checkpoint against ds_train_eval on the saved parameters
    calls = files / ("calls_%s.tsv" % is_base)
    deepsignal.main(["call_mods", "-i", str(files / "valid.tsv"), "-m", prefix, "-o", str(calls), "--is_cnn", "no", "--is_base", is_base,
                     "-x", str(T), "-y", str(S), "--batch_size", "64"])
    capsys.readouterr()
    called = np.array([int(line.split("\t")[8]) for line in open(calls)], np.int32)
    rows = train_model.read_rows(str(files / "valid.tsv"), T, S)
    assert called.shape == rows["labels"].shape
    eng = Engine(kmer_len=T, signal_len=S, max_batch=256, **variant)
    try:
        eng.load_weights(saved)
        eng.train_begin(base=True)
        loss, pred, logits = eng.train_eval(rows["means"], rows["stds"], rows["sanums"], rows["labels"], kmer=rows["kmer"])
    finally:
        eng.close()
    statement = tsb if variant["is_base"] else ts
    l64, g64, _ = statement.step(saved, rows, rows["labels"], None, 1.0, 1.0, torch.float64)
    l32, _, _ = statement.step(saved, rows, rows["labels"], None, 1.0, 1.0, torch.float32)
    loss_bar = 4 * max(abs(l32 - l64), 2.0 ** -22 * abs(l64))
    assert abs(loss - l64) <= loss_bar
    decided = np.abs(g64[:, 1] - g64[:, 0]) > loss_bar
    print("is_base %s: %d of %d rows decided, accuracy of the calls %.3f" % (is_base, int(decided.sum()), len(called), float(np.mean(called == rows["labels"]))))
    assert decided.sum() > len(called) // 2          # the comparison is not an empty one
    assert (called[decided] == pred[decided]).all() and (pred[decided] == ts.pred_of(g64, 1.0)[decided]).all()
