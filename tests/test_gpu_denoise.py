"""GPU: `deepsignal denoise` end to end on a generated file of 96 rows: models trained by ds_train_step, rows scored by the
inference forward after ds_train_sync_weights. Whether a model has learnt anything in 12 steps is not asserted; what the files
must be whatever the scores are is."""
import os

import pytest

import denoise_cases as dc
from deepsignal_amd import deepsignal

pytestmark = pytest.mark.gpu

FLAGS = ["--seq_len", "5", "--cent_signals_len", "16", "--batch_size", "16", "--rounds", "1", "--epoch_num", "2", "--step_interval", "2",
         "--seed", "3"]


def _run(d, iterations):
    d.mkdir()
    rows = dc.write_training_file(str(d / "train.tsv"), n_good=30, n_bad=18, n_neg=48, seed=2)
    rc = deepsignal.main(["denoise", "--train_file", str(d / "train.tsv"), "--iterations", str(iterations), "--scores_file", str(d / "scores.tsv")] + FLAGS)
    assert rc == 0
    return rows


def _table(path):
    return [(int(t[0]), int(t[1]), int(t[2]), float(t[3]), float(t[4])) for t in (l.split("\t") for l in open(path))]


def test_denoise_command_line(tmp_path, capsys):
    rows = _run(tmp_path / "a", 2)
    out = capsys.readouterr().out
    assert "Epoch [1/2], Step 2, Loss:" in out and "===Test, Total Accuracy:" in out
    names = sorted(os.listdir(tmp_path / "a"))
    finals = [n for n in names if n.startswith("train.denoise")]
    assert len(finals) == 1 and sorted(names) == sorted(["scores.tsv", "train.tsv"] + finals)      # halves, .neg_all, earlier iterations: gone
    final = tmp_path / "a" / finals[0]
    assert out.strip().splitlines()[-1] == "###### denoised file for training: " + str(final)
    got = open(final).readlines()
    assert set(got) <= set(rows) and len(set(got)) == len(got)                  # every output row is an input row
    table = _table(tmp_path / "a" / "scores.tsv")
    first = [t for t in table if t[0] == 1]
    assert [t[1] for t in first] == list(range(96)) and [t[2] for t in first] == [dc.label_of(r) for r in rows]
    assert all(0.0 < t[3] < 1.0 and t[4] == 0.0 for t in table)                  # one round: the mean is the score itself
    last = max(t[0] for t in table)
    assert finals[0] == "train.denoise%d.tsv" % last
    kept_last = sum(1 for t in table if t[0] == last and t[2] == 1 and t[3] > 0.5)
    pos = [r for r in got if dc.label_of(r) == 1]
    neg = [r for r in got if dc.label_of(r) == 0]
    assert len(pos) == kept_last
    assert len(neg) <= len(pos) + 5 and (len(neg) > 0) == (len(pos) > 0)         # equal in number, up to the ceil of the k-mer rule (five k-mers)
    if last == 2:     # iteration 2 scored the rows of train.denoise1: as many positives as iteration 1 kept
        assert sum(1 for t in table if t[0] == 2 and t[2] == 1) == sum(1 for t in first if t[2] == 1 and t[3] > 0.5)

    # the same seed writes the same bytes
    _run(tmp_path / "b", 2)
    assert open(tmp_path / "b" / finals[0], "rb").read() == open(final, "rb").read()
    assert open(tmp_path / "b" / "scores.tsv", "rb").read() == open(tmp_path / "a" / "scores.tsv", "rb").read()

    # one iteration with that seed is the first iteration of the run above: the positives of train.denoise1 are exactly the rows
    # whose mean in the scores file exceeds score_cf
    _run(tmp_path / "c", 1)
    capsys.readouterr()
    one = _table(tmp_path / "c" / "scores.tsv")
    assert one == first
    d1 = open(tmp_path / "c" / "train.denoise1.tsv").readlines()
    want = sorted(dc.name_of(rows[t[1]]) for t in one if t[2] == 1 and t[3] > 0.5)
    assert sorted(dc.name_of(r) for r in d1 if dc.label_of(r) == 1) == want
    assert set(d1) <= set(rows) and len(set(d1)) == len(d1)
    assert sorted(os.listdir(tmp_path / "c")) == ["scores.tsv", "train.denoise1.tsv", "train.tsv"]
