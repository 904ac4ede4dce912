"""CPU: the workflow of `deepsignal train` (deepsignal_amd/train_model.py) under a stand-in device with scripted validation
accuracies: the save rule with its quirk, the stop epoch, the text of train.txt / valid.txt and of the printed lines, the cleaning
of the output directories, seeding, the parser with its defaults and refusals, and the checkpoint round trip."""
import os
import re

import numpy as np
import pytest

import denoise_cases as dc
from deepsignal_amd import deepsignal, spec, tf_checkpoint, weights
from deepsignal_amd import train_model as tm
from deepsignal_amd.denoise import batch_metrics

K, S = 5, 16
LOG_FORMAT = "epoch:%d, iterid:%d, loss:%.3f, accuracy:%.3f, recall:%.3f, precision:%.3f\n"


def _write(path, n, seed):
    rng = np.random.default_rng(seed)
    rows = []
    for i in range(n):
        label = int(rng.integers(0, 2))
        rows.append(dc._row(i, "r", dc.KMERS[int(rng.integers(0, 4))], label, rng, K, S, 1.0 if label else -0.2))
    with open(path, "w") as f:
        f.writelines(rows)
    return rows


@pytest.fixture()
def files(tmp_path):
    _write(tmp_path / "train.tsv", 40, 1)
    _write(tmp_path / "valid.tsv", 10, 2)
    return tmp_path


def _args(d, *extra):
    argv = ["train", "--train_file", str(d / "train.tsv"), "--valid_file", str(d / "valid.tsv"), "-o", str(d / "model"), "-g", str(d / "log"),
            "--is_cnn", "no", "-x", str(K), "-y", str(S), "-b", "10", "--display_step", "2", "--max_epoch_num", "6", "--min_epoch_num", "3",
            "--seed", "5"] + list(extra)
    parser = deepsignal.build_parser(False)
    a = parser.parse_args(argv)
    tm.check_arguments(parser.train_parser, a)
    return a


class StandIn:
    """A device whose k-th validation pass has accuracy script[k] (the first round((1 - a) n) predictions are wrong); a step
    predicts mean[0] > 0.4 and reports a falling loss. Everything it is asked is recorded."""

    def __init__(self, script):
        self.script, self.steps, self.evals, self.begun = list(script), [], [], []

    def begin(self, init_seed, mask_seed):
        self.begun.append((init_seed, mask_seed))

    def step(self, rows, lr):
        pred = (rows["means"][:, 0] > 0.4).astype(np.int32)
        loss = 0.9 - 0.01 * len(self.steps)
        self.steps.append((rows["labels"].copy(), pred, loss, lr, rows["kmer"].copy()))
        return loss, pred

    def eval(self, rows):
        accu = self.script[len(self.evals)]
        pred = rows["labels"].copy()
        wrong = int(round((1 - accu) * len(pred)))
        pred[:wrong] = 1 - pred[:wrong]
        self.evals.append((rows["labels"].copy(), pred, 0.7 - 0.05 * len(self.evals)))
        return self.evals[-1][2], pred

    def weights(self):
        return {"w": np.array([len(self.steps), len(self.evals)], np.float32)}


#         epoch 0: both displays beat the epoch best and the overall best (0 until the epoch ends): two saves over one prefix
#         epoch 1: 0.4 then 0.5 beat the epoch best, not the overall 0.6: no save; no improvement, before min_epoch_num: goes on
#         epoch 2: 0.7 and 0.8: two saves; epoch 3: 0.8 does not exceed 0.8, 0.7 does not beat the epoch best: none, and it stops
SCRIPT = [0.5, 0.6, 0.4, 0.5, 0.7, 0.8, 0.8, 0.7]
SAVES = [(0, 2, 1), (0, 4, 2), (2, 10, 5), (2, 12, 6)]       # epoch, steps taken, validation passes done


def test_save_rule_stop_epoch_logs_and_printed_lines(files, capsys):
    dev = StandIn(SCRIPT)
    a = _args(files)
    saved = tm.train(a, dev)
    out = capsys.readouterr().out
    model = files / "model"
    assert [os.path.basename(p) for p in saved] == ["bn_5.sn_16.epoch_%d.ckpt" % e for e, _, _ in SAVES]
    assert len(dev.steps) == 16 and len(dev.evals) == 8 and len(dev.begun) == 1        # four epochs of four steps: stopped after epoch 3
    assert sorted(os.listdir(model)) == ["bn_5.sn_16.epoch_%d.ckpt.%s" % (e, x) for e in (0, 2) for x in ("data-00000-of-00001", "index")] + ["checkpoint"]
    for epoch, (steps, evals) in ((0, (4, 2)), (2, (12, 6))):        # the later save of an epoch stands
        got = tf_checkpoint.load_checkpoint(str(model / ("bn_5.sn_16.epoch_%d.ckpt" % epoch)))
        assert got["w"].tolist() == [steps, evals] and got["modelglobal_step"].dtype == np.int32 and int(got["modelglobal_step"]) == steps
    assert open(model / "checkpoint").read() == ('model_checkpoint_path: "bn_5.sn_16.epoch_2.ckpt"\n'
                                                 'all_model_checkpoint_paths: "bn_5.sn_16.epoch_0.ckpt"\n'
                                                 'all_model_checkpoint_paths: "bn_5.sn_16.epoch_2.ckpt"\n')
    # learning rate: epochs 0 and 1 as given, then times decay_rate
    assert [s[3] for s in dev.steps] == [0.001] * 8 + [0.001 * 0.1] * 8
    # every epoch is a permutation of the file, and the stand-in saw the codes of the k-mer column
    labels = tm.read_rows(str(files / "train.tsv"), K, S)["labels"]
    for e in range(4):
        assert sorted(np.concatenate([s[0] for s in dev.steps[4 * e:4 * e + 4]]).tolist()) == sorted(labels.tolist())
    assert dev.steps[0][4].shape == (10, K) and set(np.unique(dev.steps[0][4]).tolist()) <= {0, 1, 2, 3}

    # the logs and the printed lines, from what the stand-in recorded and the reference's formats
    train_txt, valid_txt, printed = [], [], []
    best_ep = {}
    best = 0.0
    for d in range(8):
        epoch, iterid = d // 2, 2 * (d % 2) + 2
        m = [batch_metrics(l, p) for l, p, _, _, _ in dev.steps[2 * d:2 * d + 2]]
        tl, ta = np.mean([s[2] for s in dev.steps[2 * d:2 * d + 2]]), np.mean([x[0] for x in m])
        train_txt.append(LOG_FORMAT % (epoch, iterid, tl, ta, np.mean([x[2] for x in m]), np.mean([x[1] for x in m])))
        va, vp, vr = batch_metrics(dev.evals[d][0], dev.evals[d][1])
        assert abs(va - SCRIPT[d]) < 1e-12
        valid_txt.append(LOG_FORMAT % (epoch, iterid, dev.evals[d][2], va, vr, vp))
        best_ep[epoch] = max(best_ep.get(epoch, 0.0), va)
        printed.append("epoch: %d, iterid: %d\n train_loss: %.3f, valid_loss: %.3f, train_accuracy: %.3f, valid_accuracy: %.3f, "
                       "curr_epoch_best_accuracy: %.3f, time_cost: Xs\n" % (epoch, iterid, tl, dev.evals[d][2], ta, va, best_ep[epoch]))
        if d % 2 == 1:
            best = max(best, best_ep[epoch])
            printed.append("================ epoch %d best accuracy: %.3f, best accuracy: %.3f\n" % (epoch, best_ep[epoch], best))
    assert open(files / "log" / "train.txt").read() == "".join(train_txt)
    assert open(files / "log" / "valid.txt").read() == "".join(valid_txt)
    out = re.sub(r"time_cost: \d+\.\d\ds", "time_cost: Xs", out)
    assert out.startswith("".join(printed)), out
    assert re.fullmatch(r"training finished, costs \d+\.\d seconds\.\.\n", out[len("".join(printed)):])


def test_min_epoch_num_and_max_epoch_num_bound_the_run(files, capsys):
    # never improving after epoch 0: runs on to epoch min_epoch_num - 1 = 2 and stops there
    dev = StandIn([0.6, 0.6] + [0.5] * 20)
    saved = tm.train(_args(files), dev)
    assert len(dev.steps) == 12 and [os.path.basename(p) for p in saved] == ["bn_5.sn_16.epoch_0.ckpt"]
    # always improving: max_epoch_num ends it, and only the five most recent prefixes are kept
    dev = StandIn([0.1 * (1 + k // 2) for k in range(12)])
    saved = tm.train(_args(files, "--max_epoch_num", "6"), dev)
    capsys.readouterr()
    assert len(dev.steps) == 24 and len(saved) == 6
    names = sorted(n for n in os.listdir(files / "model") if n.endswith(".index"))
    assert names == ["bn_5.sn_16.epoch_%d.ckpt.index" % e for e in range(1, 6)]
    assert open(files / "model" / "checkpoint").read().splitlines()[0] == 'model_checkpoint_path: "bn_5.sn_16.epoch_5.ckpt"'


def test_an_existing_model_dir_and_log_dir_are_cleaned(files, capsys):
    model, log = files / "model", files / "log"
    model.mkdir()
    log.mkdir()
    for name in ("bn_5.sn_16.epoch_7.ckpt.index", "bn_5.sn_16.epoch_7.ckpt.data-00000-of-00001", "checkpoint", "notes.txt", "bn_17.sn_360.epoch_1.ckpt.index"):
        (model / name).write_text("old")
    (log / "train.txt").write_text("old\n")
    (log / "other.txt").write_text("old\n")
    tm.train(_args(files), StandIn([0.5] * 20))
    out = capsys.readouterr().out
    assert "the previous model (3 files) in model_directory deleted..." in out
    assert "the previous log file (1 files) in log_directory deleted..." in out
    left = set(os.listdir(model))
    assert "bn_5.sn_16.epoch_7.ckpt.index" not in left and "bn_5.sn_16.epoch_7.ckpt.data-00000-of-00001" not in left
    assert {"notes.txt", "bn_17.sn_360.epoch_1.ckpt.index", "checkpoint", "bn_5.sn_16.epoch_0.ckpt.index"} <= left
    assert (model / "notes.txt").read_text() == "old" and (model / "checkpoint").read_text() != "old"
    assert "old" not in (log / "train.txt").read_text() and (log / "other.txt").read_text() == "old\n"


def test_seed_decides_every_byte(files, capsys):
    def run(seed, sub):
        dev = StandIn(SCRIPT)
        a = _args(files, "--seed", str(seed), "-o", str(files / sub), "-g", str(files / (sub + "_log")))
        tm.train(a, dev)
        capsys.readouterr()
        got = {}
        for d in (files / sub, files / (sub + "_log")):
            for name in sorted(os.listdir(d)):
                got[name] = open(d / name, "rb").read()
        return got, dev
    a, dev_a = run(5, "a")
    b, dev_b = run(5, "b")
    c, dev_c = run(6, "c")
    assert a == b and dev_a.begun == dev_b.begun
    assert dev_c.begun != dev_a.begun and c["train.txt"] != a["train.txt"]


def test_parser_defaults_are_the_references():
    parser = deepsignal.build_parser(False)
    a = parser.parse_args(["train", "--train_file", "t", "--valid_file", "v", "--model_dir", "m"])
    want = dict(is_binary="no", log_dir=None, is_cnn="yes", is_base="yes", is_rnn="yes", kmer_len=17, cent_signals_len=360, batch_size=512,
                learning_rate=0.001, decay_rate=0.1, class_num=2, keep_prob=0.5, max_epoch_num=10, min_epoch_num=5, display_step=100,
                pos_weight=1.0, seed=None, device=None)
    for k, v in want.items():
        assert getattr(a, k) == v, k
    b = parser.parse_args(["train", "--train_file", "t", "--valid_file", "v", "-o", "m", "-g", "l", "-x", "9", "-y", "20", "-b", "4", "-l", "0.5",
                           "-d", "0.3", "-c", "2"])
    assert (b.model_dir, b.log_dir, b.kmer_len, b.cent_signals_len, b.batch_size, b.learning_rate, b.decay_rate, b.class_num) == \
        ("m", "l", 9, 20, 4, 0.5, 0.3, 2)
    assert "held in memory" in parser.train_parser.format_help() and "20m" in parser.train_parser.format_help()


@pytest.mark.parametrize("flags,message", [([], "--is_cnn no"),
                                           (["--is_cnn", "yes"], "signal model has no backward"),
                                           (["--is_cnn", "no", "--is_rnn", "no"], "--is_rnn no is not implemented"),
                                           (["--is_cnn", "no", "--class_num", "3"], "--class_num other than 2 is not implemented"),
                                           (["--is_cnn", "no", "--is_binary", "yes"], "--is_binary yes is not implemented")])
def test_what_is_not_trained_is_a_usage_error(flags, message, capsys):
    with pytest.raises(SystemExit) as e:
        deepsignal.main(["train", "--train_file", "t", "--valid_file", "v", "-o", "m"] + flags)
    assert e.value.code == 2
    assert message in capsys.readouterr().err


@pytest.mark.parametrize("is_base", [True, False])
def test_a_saved_checkpoint_reads_back_as_the_variants_weights(tmp_path, is_base):
    w = weights.random_weights(seed=3, kmer_len=K, signal_len=S, is_cnn=False, is_rnn=True, is_base=is_base)
    prefix = tm.Saver(str(tmp_path)).save("bn_5.sn_16.epoch_0.ckpt", w, 123)
    back = tf_checkpoint.checkpoint_to_weights(prefix, kmer_len=K, signal_len=S, is_cnn=False, is_rnn=True, is_base=is_base)
    assert list(back) == [n for n, _ in spec.tensor_table(K, S, 2, is_cnn=False, is_rnn=True, is_base=is_base)]
    assert ("modelembedding" in back) == is_base
    for name, arr in w.items():
        assert back[name].dtype == np.float32 and back[name].tobytes() == arr.tobytes(), name
    assert int(tf_checkpoint.load_checkpoint(prefix, ["modelglobal_step"])["modelglobal_step"]) == 123
    assert tf_checkpoint.is_checkpoint(prefix)
