"""GPU: `call_mods --freq_file` -- freq_values_kernel against the CPU checker built from the same routine, bit for bit; the streaming
table (growth by rehash, pushes in row order) against calculate_mods_frequency on the text of the same rows; and the command line
against `call_freq --on cpu` on the result file it writes, byte for byte."""
import os

import numpy as np
import pytest

from deepsignal_amd import call_modification_frequency as cmf
from deepsignal_amd import engine as eng
from deepsignal_amd import synth
from deepsignal_amd import weights as W

from callfreq_cases import (HOST, OK, act_for, assert_values, cpu_table, edge_q, make_batch, outside_act, random_q, random_rows,
                            stream_table)
from freq_cases import stats_tuple

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def engine():
    e = eng.Engine(device=0, max_batch=64, slots=1)
    yield e
    e.close()


def test_values_kernel_equals_the_checker(engine):
    edge, outside = act_for(edge_q()), outside_act()
    act = np.concatenate([edge, outside, act_for(random_q(4096 - len(edge) - len(outside), 15))])
    assert act.shape == (4096, 2)
    r0, r1, rs = eng.freq_values_reference(act)
    p0, p1, status = engine.freq_values(act)
    assert status.tolist() == rs.tolist() and (status == HOST).any() and (status == OK).sum() > 4000
    assert p0.tobytes() == r0.tobytes() and p1.tobytes() == r1.tobytes()
    assert_values(act, p0, p1, status)                               # and both are Python's
    wide = np.concatenate([act, np.ones((4096, 1), np.float32)], axis=1)          # class_num 3
    q0, q1, qs = engine.freq_values(wide)
    assert qs.tolist() == rs.tolist() and q0.tobytes() == r0.tobytes() and q1.tobytes() == r1.tobytes()


ROWS, SITES = 3000, 700


@pytest.fixture(scope="module")
def rows():
    infos, act, pred, kmer = random_rows(41, ROWS, SITES)
    # a site seen twice inside one push and again in every later one
    for r in (5, 6, 300, 600, 900, 2999):
        infos[r] = infos[5].rsplit("\t", 2)[0] + "\tdup%d\tt" % r
    return infos, act, pred, kmer


def batches_of(rows, size):
    infos, act, pred, kmer = rows
    return [make_batch(infos[s:s + size], act[s:s + size], pred[s:s + size], kmer[s:s + size]) for s in range(0, len(infos), size)]


@pytest.mark.parametrize("prob_cf", [0.0, 0.3])
def test_stream_with_growth(rows, tmp_path, capsys, prob_cf):
    batches = batches_of(rows, 257)
    want, want_bytes = cpu_table(tmp_path, batches, prob_cf)
    cpu_out = capsys.readouterr().out
    assert len(want) > 600
    # 64 slots at first: 2 * (sites + 257) > slots doubles the table before the first insert and on through the run
    got, got_bytes, info = stream_table(tmp_path, batches, prob_cf, device=0, batch_rows=257, initial_slots=64)
    out = capsys.readouterr().out
    assert stats_tuple(got) == stats_tuple(want)                     # keys in the same order, sums bit for bit, counts
    assert got_bytes == want_bytes and out.splitlines()[-1] == cpu_out.splitlines()[-1]
    assert info["growths"] >= 5 and info["rows"] == ROWS and info["host_rows"] == 0 and info["batches"] == len(batches)
    # one push larger than the table it meets
    got, got_bytes, info = stream_table(tmp_path, batches_of(rows, ROWS), prob_cf, device=0, batch_rows=4096, initial_slots=64)
    assert stats_tuple(got) == stats_tuple(want) and info["growths"] == 7 and info["batches"] == 1      # 64 -> 8,192 slots in one rehash
    # no growth at all: the same table
    got, got_bytes, info = stream_table(tmp_path, batches, prob_cf, device=0, batch_rows=257, initial_slots=1 << 14)
    assert stats_tuple(got) == stats_tuple(want) and got_bytes == want_bytes and info["growths"] == 0


def test_push_reports_status_and_opened_rows(engine):
    act = np.array([[0.2, 0.8], [0.5, 0.5], [0.0, 0.0], [0.3, 0.7], [0.1, 0.9], [0.4, 0.6], [0.25, 0.75]], np.float32)
    chrom = np.array([0, 1, 0, 1, 0, -1, 0], np.int32)
    pos = np.array([7, 9, 7, 9, 7, 3, 1 << 40], np.int64)
    engine.freq_begin_stream(1, 16, 0.3)
    try:
        status = engine.freq_push(chrom, pos, act, np.array([1, 0, 1, 1, 1, 1, 1], np.int32))
        assert status.tolist() == [OK, OK, HOST, OK, OK, HOST, HOST]        # NaN, a flagged row, a position outside the key
        with pytest.raises(RuntimeError):                            # the push is open until its host rows have their values
            engine.freq_push(chrom, pos, act, np.zeros(7, np.int32))
        opened = engine.freq_accumulate([2, 5, 6], [0, 2, 2], [7, 3, 3], [float("nan"), 0.4, 0.5], [0.5, 0.6, 0.5], [1, 1, 1])
        # row 1 is below the threshold: its site opens with row 3; row 5 is below it too, so (2, 3) never opens
        assert opened.tolist() == [1, 0, 0, 1, 0, 0, 0]
        res = engine.freq_result()
    finally:
        engine.freq_end()
    order = np.argsort(res["first_row"])
    assert res["first_row"][order].tolist() == [0, 3] and res["rows"] == 7 and res["used"] == 4
    assert res["met"][order].tolist() == [3, 1] and np.isnan(res["sum0"][order][0])
    t = engine.freq_stream_times()
    assert t["growths"] >= 1 and t["values_ms"] > 0


# ---- the command line ----------------------------------------------------------------------------------------------------------
NCALLS, NPOS = 600, 40


@pytest.fixture(scope="module")
def cli(balanced_weights, tmp_path_factory):
    from deepsignal_amd.deepsignal import main
    from deepsignal_amd.utils.process_utils import code2base_dna
    d = tmp_path_factory.mktemp("call_mods_freq")
    feats = synth.synthetic_features(NCALLS, seed=77)
    tsv, dsw = str(d / "features.tsv"), str(d / "model.dsw")
    with open(tsv, "w") as f:
        for i in range(NCALLS):
            k = i % NPOS
            cols = ["chr%d" % (1 + k % 3), str(1000 + 7 * k), "+-"[k % 2], str(5000 - k), "read_%03d" % (i // NPOS), "t",
                    "".join(code2base_dna[int(c)] for c in feats["kmer"][i]),
                    ",".join("%s" % np.float32(x) for x in feats["means"][i]), ",".join("%s" % np.float32(x) for x in feats["stds"][i]),
                    ",".join(str(int(x)) for x in feats["sanums"][i]), ",".join("%s" % np.float32(x) for x in feats["signals"][i]), "1"]
            f.write("\t".join(cols) + "\n")
    W.save_weights(dsw, balanced_weights)
    base = ["call_mods", "-i", tsv, "-m", dsw, "--engine_batch", "512"]
    plain = str(d / "plain.tsv")
    assert main(base + ["-o", plain]) == 0
    return d, base, open(plain, "rb").read()


def call_freq_cpu(d, calls, tag, argv):
    out = str(d / (tag + ".want"))
    assert cmf.main(["-i", calls, "-o", out, "--on", "cpu"] + argv) == 0
    return open(out, "rb").read()


@pytest.mark.parametrize("tag,flags,freq_flags", [("table", [], []), ("bed", ["--freq_bed"], ["--bed"]), ("sort", ["--freq_sort"], ["--sort"]),
                                                  ("cf", ["--freq_prob_cf", "0.2"], ["--prob_cf", "0.2"])])
def test_cli_table_next_to_the_result_file(cli, capsys, tag, flags, freq_flags):
    from deepsignal_amd.deepsignal import main
    d, base, plain = cli
    calls, freq = str(d / (tag + ".calls.tsv")), str(d / (tag + ".freq.tsv"))
    assert main(base + ["-o", calls, "--freq_file", freq] + flags) == 0
    out = capsys.readouterr().out
    assert open(calls, "rb").read() == plain and plain.count(b"\n") == NCALLS        # the result file is what it was
    want = call_freq_cpu(d, calls, tag, freq_flags)
    assert open(freq, "rb").read() == want and (want.count(b"\n") == NPOS if tag != "cf" else 0 < want.count(b"\n") <= NPOS)
    assert capsys.readouterr().out.splitlines()[-1] in out.splitlines()             # the "calls used" line
    # the table alone: the same bytes, and no result file
    alone = str(d / (tag + ".alone.tsv"))
    before = set(os.listdir(str(d)))
    assert main(base + ["--freq_file", alone] + flags) == 0
    assert open(alone, "rb").read() == want
    assert set(os.listdir(str(d))) - before == {os.path.basename(alone)}


def test_cli_parse_on_gpu_and_freq_device(cli):
    from deepsignal_amd.deepsignal import main
    d, base, plain = cli
    calls, freq = str(d / "text.calls.tsv"), str(d / "text.freq.tsv")
    assert main(base + ["-o", calls, "--freq_file", freq, "--parse_on", "gpu", "--freq_device", "0"]) == 0
    assert open(calls, "rb").read() == plain
    assert open(freq, "rb").read() == call_freq_cpu(d, calls, "text", [])


def test_cli_aggregates_the_merged_results_of_a_recheck(cli, capsys):
    from deepsignal_amd.deepsignal import main
    d, base, plain = cli
    calls, freq = str(d / "recheck.calls.tsv"), str(d / "recheck.freq.tsv")
    assert main(base + ["-o", calls, "--freq_file", freq, "--precision", "bf16_all", "--recheck_margin", "0.1"]) == 0
    out = capsys.readouterr().out
    assert "recheck: %d sites" % NCALLS in out
    assert open(freq, "rb").read() == call_freq_cpu(d, calls, "recheck", [])


def test_cli_fast5_directory_with_extraction_on_the_gpu(tmp_path, small_weights):
    """The fast5 route with --extract_on gpu: the rows reach the stream from the tickets of ds_submit_reads, in file order."""
    import shutil
    from deepsignal_amd.deepsignal import main
    d = tmp_path / "f5"
    shutil.copytree(os.path.join(os.path.dirname(__file__), "golden", "fast5", "plain"), str(d))
    dsw = str(tmp_path / "model.dsw")
    W.save_weights(dsw, small_weights)
    base = ["call_mods", "-i", str(d), "-m", dsw, "--f5_batch_num", "2", "--batch_size", "16", "--engine_batch", "64", "--extract_on", "gpu"]
    calls, freq, alone = (str(tmp_path / x) for x in ("calls.tsv", "freq.tsv", "alone.tsv"))
    assert main(base + ["-o", calls, "--freq_file", freq]) == 0
    want = call_freq_cpu(tmp_path, calls, "fast5", [])
    assert open(freq, "rb").read() == want and want
    assert main(base + ["--freq_file", alone]) == 0
    assert open(alone, "rb").read() == want


def test_fast5_reads_straddling_engine_batches(tmp_path, small_weights):
    """--extract_on gpu with an engine of 7 sites per forward: the file batch's reads (9 .. 17 sites each) straddle batches and need
    more tickets than the engine has slots; rows and table are those of an engine that takes the file batch in one forward."""
    from deepsignal_amd import call_modifications as cm
    d = os.path.join(os.path.dirname(__file__), "golden", "fast5", "plain")
    dsw = str(tmp_path / "model.dsw")
    W.save_weights(dsw, small_weights)
    f5_args = (True, "RawGenomeCorrected_000", "BaseCalled_template", None, True, "mad", "CG", 0, 1, 5, None)
    out = {}
    for cap in (7, 4096):
        calls, freq = str(tmp_path / ("calls%d.tsv" % cap)), str(tmp_path / ("freq%d.tsv" % cap))
        n = cm.call_mods(d, dsw, calls, 17, 360, 16, 0.001, 2, 1, True, True, True, True, f5_args, engine_batch=cap, extract_on="gpu",
                         freq_file=freq)
        out[cap] = (n, open(calls, "rb").read(), open(freq, "rb").read())
    assert out[7] == out[4096] and out[7][0] == out[7][1].count(b"\n") == 68 and out[7][2]
