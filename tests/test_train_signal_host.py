"""CPU: what `deepsignal train --is_cnn yes --is_rnn no` adds on the host: the workflow under a stand-in device that reads the
signals, the new and the kept usage errors, the checkpoint round trip of the signal-only variant (moving statistics included), the
mask checker that takes the stream's width, and the new entries of the C ABI."""
import os
import re

import numpy as np
import pytest

import __graft_entry__ as g
import denoise_cases as dc
from deepsignal_amd import deepsignal, spec, tf_checkpoint, weights
from deepsignal_amd import train_model as tm

K, S = 5, 40
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("ds_train_begin_signal", "ds_train_step_signal", "ds_train_eval_signal", "ds_train_get_tap", "ds_train_mask_reference_wide")


def _write(path, n, seed):
    rng = np.random.default_rng(seed)
    rows = [dc._row(i, "r", dc.KMERS[int(rng.integers(0, 4))], label, rng, K, S, 1.0 if label else -0.2)
            for i, label in enumerate(rng.integers(0, 2, n).tolist())]
    with open(path, "w") as f:
        f.writelines(rows)


class StandIn:
    """Predicts from the signals alone (their mean > 0.4) and records what it was given."""

    def __init__(self):
        self.steps, self.evals, self.begun = [], [], []

    def begin(self, init_seed, mask_seed):
        self.begun.append((init_seed, mask_seed))

    def step(self, rows, lr):
        self.steps.append((rows["signals"].copy(), rows["labels"].copy(), lr))
        return 0.9 - 0.01 * len(self.steps), (rows["signals"].mean(axis=1) > 0.4).astype(np.int32)

    def eval(self, rows):
        self.evals.append(rows["signals"].shape)
        return 0.7 - 0.01 * len(self.evals), (rows["signals"].mean(axis=1) > 0.4).astype(np.int32)

    def weights(self):
        return weights.random_weights(seed=len(self.steps), kmer_len=K, signal_len=S, is_cnn=True, is_rnn=False, randomize_bn=True)


def test_workflow_reads_the_signals_and_saves_the_variant(tmp_path):
    _write(tmp_path / "train.tsv", 40, 1)
    _write(tmp_path / "valid.tsv", 10, 2)
    parser = deepsignal.build_parser(False)
    a = parser.parse_args(["train", "--train_file", str(tmp_path / "train.tsv"), "--valid_file", str(tmp_path / "valid.tsv"), "-o",
                           str(tmp_path / "model"), "-g", str(tmp_path / "log"), "--is_cnn", "yes", "--is_rnn", "no", "-x", str(K), "-y", str(S),
                           "-b", "10", "--display_step", "2", "--max_epoch_num", "2", "--min_epoch_num", "1", "--seed", "5"])
    tm.check_arguments(parser.train_parser, a)          # --is_base yes (the default) is ignored, as in the reference
    dev = StandIn()
    saved = tm.train(a, dev)
    rows = tm.read_rows(str(tmp_path / "train.tsv"), K, S)
    assert rows["signals"].shape == (40, S) and rows["signals"].dtype == np.float32 and rows["kmer"].shape == (40, K)
    assert len(dev.steps) >= 4 and all(sig.shape == (10, S) for sig, _, _ in dev.steps) and dev.evals[0] == (10, S)
    # an epoch's batches are a permutation of the file's rows, signals and labels moved together
    epoch = np.concatenate([sig for sig, _, _ in dev.steps[:4]])
    assert sorted(map(bytes, epoch)) == sorted(map(bytes, rows["signals"]))
    by_signal = {bytes(s): int(l) for s, l in zip(rows["signals"], rows["labels"])}
    assert all(by_signal[bytes(s)] == int(l) for sig, lab, _ in dev.steps[:4] for s, l in zip(sig, lab))
    assert saved and os.path.basename(saved[0]) == "bn_5.sn_40.epoch_0.ckpt"
    back = tf_checkpoint.checkpoint_to_weights(saved[-1], kmer_len=K, signal_len=S, is_cnn=True, is_rnn=False)
    assert list(back) == [n for n, _ in spec.tensor_table(K, S, 2, is_cnn=True, is_rnn=False)]
    names = set(tf_checkpoint.load_checkpoint(saved[-1]))
    assert not [n for n in names if n.endswith(("/biased", "/local_step"))]         # the zero-debias helpers are not written


@pytest.mark.parametrize("flags,message", [([], "--is_cnn no"),
                                           ([], "signal model has no backward"),
                                           ([], "--is_rnn no to train it alone"),
                                           (["--is_cnn", "yes", "--is_rnn", "yes"], "signal model has no backward"),
                                           (["--is_cnn", "no", "--is_rnn", "no"], "--is_rnn no is not implemented"),
                                           (["--is_cnn", "yes", "--is_rnn", "no", "--class_num", "3"], "--class_num other than 2 is not implemented"),
                                           (["--is_cnn", "yes", "--is_rnn", "no", "--is_binary", "yes"], "--is_binary yes is not implemented")])
def test_usage_errors_new_and_kept(flags, message, capsys):
    with pytest.raises(SystemExit) as e:
        deepsignal.main(["train", "--train_file", "t", "--valid_file", "v", "-o", "m"] + flags)
    assert e.value.code == 2
    assert message in capsys.readouterr().err


def test_signal_only_flags_pass_the_checks_and_help_gives_the_memory():
    parser = deepsignal.build_parser(False)
    for extra in ([], ["--is_base", "no"]):
        a = parser.parse_args(["train", "--train_file", "t", "--valid_file", "v", "-o", "m", "--is_cnn", "yes", "--is_rnn", "no"] + extra)
        tm.check_arguments(parser.train_parser, a)
    text = re.sub(r"\s+", " ", parser.train_parser.format_help())
    assert "4 x (4 x kmer_len + cent_signals_len) bytes a row" in text and "1.7 KB" in text
    assert 4 * (4 * 17 + 360) == 1712


def test_a_saved_checkpoint_reads_back_as_the_variants_weights(tmp_path):
    w = weights.random_weights(seed=3, kmer_len=K, signal_len=S, is_cnn=True, is_rnn=False, randomize_bn=True)
    prefix = tm.Saver(str(tmp_path)).save("bn_5.sn_40.epoch_0.ckpt", w, 77)
    back = tf_checkpoint.checkpoint_to_weights(prefix, kmer_len=K, signal_len=S, is_cnn=True, is_rnn=False)
    assert list(back) == [n for n, _ in spec.tensor_table(K, S, 2, is_cnn=True, is_rnn=False)] and len(back) == 113 * 5 + 2
    assert sum(n.endswith(("/moving_mean", "/moving_variance")) for n in back) == 226
    for name, arr in w.items():
        assert back[name].dtype == np.float32 and back[name].tobytes() == arr.tobytes(), name
    assert int(tf_checkpoint.load_checkpoint(prefix, ["modelglobal_step"])["modelglobal_step"]) == 77


def test_initial_batch_norm_is_the_references():
    w = weights.random_weights(seed=1, signal_len=S, is_cnn=True, is_rnn=False, randomize_bn=False)
    for name, arr in w.items():
        leaf = name.rsplit("/", 1)[-1]
        if leaf in ("gamma", "moving_variance"):
            assert (arr == 1).all(), name
        if leaf in ("beta", "moving_mean"):
            assert (arr == 0).all(), name


@pytest.fixture(scope="module")
def engine():
    g.build()
    from deepsignal_amd import engine
    return engine


def test_wide_mask_checker(engine):
    wide, narrow = engine.train_mask_reference_wide, engine.train_mask_reference
    J = spec.net_dims(17, 360, 2, True, False).joint
    a = wide(3, 0, "fc1", 8, J, 0.5)
    assert J == 5520 and a.shape == (8, J) and a.dtype == np.uint8 and set(np.unique(a)) == {0, 1}
    assert (wide(3, 0, "fc1", 8, J, 0.5) == a).all()
    # the function ds_train_mask_reference runs: the first 512 units of a row are that checker's row, and fc2 is fc2
    assert (a[:, :512] == narrow(3, 0, "fc1", 8, 17, 0.5)).all()
    assert (wide(3, 0, "fc2", 8, 2, 0.5) == narrow(3, 0, "fc2", 8, 17, 0.5)).all()
    assert (wide(3, 0, "fc1", 3, 700, 0.5) == a[:3, :700]).all()                       # a row's mask depends on neither n nor the width
    for other in (wide(4, 0, "fc1", 8, J, 0.5), wide(3, 1, "fc1", 8, J, 0.5)):
        assert abs((other == a).mean() - 0.5) < 0.02                                   # 6 sigma of 44,160 fair draws is 0.014
    assert abs(a.mean() - 0.5) <= 6 * np.sqrt(0.25 / a.size) and abs((a[0] == a[1]).mean() - 0.5) < 0.05
    assert wide(9, 5, "fc1", 4, 65535, 1.0).all()
    for args in ((1, 0, "fw_l0", 4, 256, 0.5), (1, 0, "fc1", 4, 65536, 0.5), (1, 0, "fc1", 4, 0, 0.5), (1, 0, "fc1", 4, 100, 0.0)):
        with pytest.raises(ValueError):
            wide(*args)


def test_new_entries_are_declared_and_exported(engine):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "deepsignal_hip.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(ds_[a-z_0-9]+)\s*\(", text))
    lib = engine.load_library()
    for name in NEW_SYMBOLS:
        assert name in declared and name in engine.EXPORTED_SYMBOLS and hasattr(lib, name), name
    assert b"0.5" in lib.ds_version() and b"0.4 (" not in lib.ds_version()
    assert engine.signal_tap_names()[:4] == ["stem1", "stem2", "stem3", "m1.b1"] and len(engine.signal_tap_names()) == 3 + 11 * 11 + 2
    assert len(engine.signal_trainable_names()) == 341 and len(engine.signal_tensor_names()) == 567
