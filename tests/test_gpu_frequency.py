"""GPU: `call_freq --on gpu` -- the device kernels (csrc/ds_freq.hip) against the CPU checker built from the same routines, bit for
bit, and the command line against the cpu route, byte for byte."""
import gzip
import json
import os

import numpy as np
import pytest

from deepsignal_amd import call_modification_frequency as cmf
from deepsignal_amd import deepsignal
from deepsignal_amd import engine as eng

from freq_cases import bits, call_row, random_rows, stats_tuple

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(__file__), "golden", "frequency_golden.json")


@pytest.fixture(scope="module")
def gold():
    with open(GOLD) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def engine():
    e = eng.Engine(device=0, max_batch=64, slots=1)
    yield e
    e.close()


def write_rows(path, rows, newline="\n"):
    with open(str(path), "wb") as f:
        f.write((newline.join(rows) + newline).encode())
    return str(path)


def device_sites(engine, text, batch_rows, prob_cf=0.0, total=None):
    """The rows of `text` through freq_parse / freq_accumulate in batches -> the sites ordered by first row, and the checker's."""
    begin, end, chrom, flags, names = eng.freq_locate(text)
    n = len(begin)
    engine.freq_begin(n if total is None else total, batch_rows, prob_cf)
    try:
        for s in range(0, n, batch_rows):
            t = min(n, s + batch_rows)
            status = engine.freq_parse(text, begin[s:t], end[s:t], chrom[s:t], flags[s:t])
            assert (status == eng.TEXT_ROW_OK).all()
            engine.freq_accumulate()
        got = engine.freq_result()
    finally:
        engine.freq_end()
    ref = eng.freq_reference(text, begin, end, chrom, flags, prob_cf)
    order = np.argsort(got["first_row"], kind="stable")
    return {k: (v[order] if isinstance(v, np.ndarray) else v) for k, v in got.items()}, ref


def assert_sites_equal(got, ref):
    assert got["first_row"].tolist() == ref["first_row"].tolist()          # the unsorted output order
    assert got["chrom"].tolist() == ref["chrom"].tolist() and got["pos"].tolist() == ref["pos"].tolist()
    assert got["sum0"].tobytes() == ref["sum0"].tobytes() and got["sum1"].tobytes() == ref["sum1"].tobytes()
    assert got["met"].tolist() == ref["met"].tolist() and got["unmet"].tolist() == ref["unmet"].tolist()
    assert got["used"] == ref["used"] and got["rows"] == len(ref["status"])


def both_routes(tmp_path, argv, capsys, via=cmf.main):
    out_c, out_g = str(tmp_path / "cpu.out"), str(tmp_path / "gpu.out")
    assert via(argv + ["-o", out_c]) == 0
    cpu_stdout = capsys.readouterr().out
    assert via(argv + ["-o", out_g, "--on", "gpu"]) == 0
    gpu_stdout = capsys.readouterr().out
    return open(out_c, "rb").read(), open(out_g, "rb").read(), cpu_stdout, gpu_stdout


@pytest.mark.parametrize("idx", [0, 1, 2, 3])
def test_golden_cases_on_the_gpu(gold, idx, tmp_path, capsys):
    case = gold["cases"][idx]
    inp = write_rows(tmp_path / "calls.tsv", gold["input_rows"])
    cpu, gpu, cpu_stdout, gpu_stdout = both_routes(tmp_path, ["-i", inp] + case["flags"], capsys)
    assert gpu.decode().splitlines() == case["output"]
    assert gpu == cpu and gpu_stdout == cpu_stdout


@pytest.mark.parametrize("nrows", [1, 63, 64, 65, 1000])
def test_row_counts_and_batch_sizes(engine, nrows):
    text = ("\n".join(random_rows(10 + nrows, nrows, min(nrows, 40), 3)) + "\n").encode()
    for batch in (256, 1024):                  # 1,000 rows: four batches with every site in several of them, and one batch
        got, ref = device_sites(engine, text, batch, prob_cf=0.1)
        assert_sites_equal(got, ref)


def test_sums_follow_the_row_order(engine):
    rng = np.random.default_rng(5)
    p = np.float32(10.0 ** rng.uniform(-7, 0, 3000))
    vals = [float(str(x)) for x in p]
    fwd = rev = 0.0
    for v in vals:
        fwd += v
    for v in reversed(vals):
        rev += v
    assert bits(fwd) != bits(rev)              # otherwise the input proves nothing
    rows = [call_row("chr1", 77, str(x), "0.0", label=1) for x in p]
    text = ("\n".join(rows) + "\n").encode()
    for batch in (256, 4096):
        got, ref = device_sites(engine, text, batch)
        assert_sites_equal(got, ref)
        assert len(got["sum0"]) == 1 and bits(float(got["sum0"][0])) == bits(fwd)
        assert got["met"].tolist() == [3000]


def test_run_heads_on_workgroup_edges(engine):
    """Three sites of 256 rows each, interleaved in file order: whatever order the hash gives the sites, their runs begin on sorted
    lanes 0, 256 and 512, the first lanes of three workgroups, with 256 pad keys behind (768 rows sort as 1,024 keys). Then in
    batches of 256, where every run goes on from the sums the batch before it stored."""
    rng = np.random.default_rng(11)
    p = np.float32(10.0 ** rng.uniform(-7, 0, 768))
    differs = False
    for site in range(3):
        vals = [float(str(x)) for x in p[site::3]]
        fwd = rev = 0.0
        for v in vals:
            fwd += v
        for v in reversed(vals):
            rev += v
        differs = differs or bits(fwd) != bits(rev)
    assert differs                             # otherwise the input proves nothing
    rows = [call_row("chr1", 100 + i % 3, str(x), "0.0", label=i % 2) for i, x in enumerate(p)]
    text = ("\n".join(rows) + "\n").encode()
    for batch in (768, 256):
        got, ref = device_sites(engine, text, batch)
        assert_sites_equal(got, ref)
        assert got["first_row"].tolist() == [0, 1, 2] and (got["met"] + got["unmet"]).tolist() == [256] * 3


def test_table_at_its_load_cap(engine):
    pos = [0, (1 << 40) - 1] + list(range(1, 2047))
    rows = [call_row("chr%d" % (i % 3), q, 0.25, 0.75, pis=1) for i, q in enumerate(pos)]
    text = ("\n".join(rows) + "\n").encode()
    got, ref = device_sites(engine, text, 512)          # 2,048 distinct sites in 4,096 slots
    assert len(got["first_row"]) == 2048 and got["first_row"].tolist() == list(range(2048))
    assert_sites_equal(got, ref)
    assert got["pos"][:2].tolist() == [0, (1 << 40) - 1]
    with pytest.raises(RuntimeError):                   # the host refuses rows the table was not sized for
        device_sites(engine, text, 512, total=2047)


def test_positions_outside_the_key(tmp_path, capsys):
    rows = [call_row("chr1", 5, 0.25, 0.75), call_row("chr1", 1 << 40, 0.25, 0.75), call_row("chr1", -2, 0.3, 0.7),
            call_row("chr1", 1 << 40, 0.125, 0.875), call_row("chr1", 5, 0.5, 0.5), call_row("chr1", -2, 0.4, 0.6)]
    inp = write_rows(tmp_path / "calls.tsv", rows)
    cpu, gpu, cpu_stdout, gpu_stdout = both_routes(tmp_path, ["-i", inp], capsys)
    assert gpu == cpu and str(1 << 40).encode() in gpu and b"\t-2\t" in gpu
    assert "4 row(s) parsed on the host" in gpu_stdout and gpu_stdout.splitlines()[-1] == cpu_stdout.splitlines()[-1]


def test_threshold_edges(tmp_path, capsys):
    # |p0 - p1| in double just below, at and just above 0.4: by one unit in the last place (17 digits: rows for the host parser)
    # and by one unit of the 15th digit (rows the device parses), plus differences that round onto and next to 0.4
    below, above = float(np.nextafter(0.4, 0.0)), float(np.nextafter(0.4, 1.0))
    cases = [("0.5", "0.1"), ("0.4", "0.0"), ("0.4", "0"), (repr(above), "0.0"), (repr(below), "0.0"), ("0.400000000000001", "0"),
             ("0.399999999999999", "0"), ("0.7", "0.3"), ("0.3", "0.7"), ("0.6", "0.2"), ("0.9", "0.5"), ("0.45", "0.05"),
             ("0.05", "0.45"), ("0.1", "0.5")]
    diffs = [abs(float(a) - float(b)) for a, b in cases]
    assert below in diffs and above in diffs and 0.4 in diffs
    rows = [call_row("chr1", 100 + i, a, b, label=1) for i, (a, b) in enumerate(cases)]
    inp = write_rows(tmp_path / "calls.tsv", rows)
    cpu, gpu, cpu_stdout, gpu_stdout = both_routes(tmp_path, ["-i", inp, "--prob_cf", "0.4"], capsys)
    assert gpu == cpu and gpu_stdout.splitlines()[-1] == cpu_stdout.splitlines()[-1]
    assert gpu.count(b"\n") == sum(not d < 0.4 for d in diffs) and 0 < gpu.count(b"\n") < len(cases)


HOST_FORMS = [("nan", "0.5"), ("inf", "0.5"), ("1e-30", "0.75"), ("+0.5", "0.25")]


def test_host_rows_in_the_middle_of_a_run(tmp_path, capsys):
    rows = []
    for i in range(40):
        rows.append(call_row("chr1", 9, np.float32(0.01 * i), np.float32(1 - 0.01 * i)))
        rows.append(call_row("chr2", 9 + i % 3, 0.2, 0.8))
    planted = [call_row("chr1", 9, a, b, label=1) for a, b in HOST_FORMS] + [" " + call_row("chr1", 9, 0.3, 0.7),
                                                                              call_row("chr1", 9, 0.6, 0.4) + "\r"]
    for k, r in enumerate(planted):
        rows.insert(7 + 11 * k, r)
    inp = write_rows(tmp_path / "calls.tsv", rows)
    cpu = cmf.calculate_mods_frequency([inp], 0.0)
    info = {}
    gpu = cmf.calculate_mods_frequency_gpu([inp], 0.0, batch_rows=16, info=info)
    assert stats_tuple(gpu) == stats_tuple(cpu)
    assert info["host_rows"] == len(planted)
    capsys.readouterr()
    c, g, cpu_stdout, gpu_stdout = both_routes(tmp_path, ["-i", inp], capsys)
    assert g == c and "%d row(s) parsed on the host" % len(planted) in gpu_stdout


def test_short_row_raises_as_the_cpu_route(tmp_path):
    good = call_row("chr1", 10, 0.3, 0.7)
    inp = write_rows(tmp_path / "calls.tsv", [good, "\t".join(good.split("\t")[:8]), good])
    with pytest.raises(IndexError):
        cmf.main(["-i", inp, "-o", str(tmp_path / "c.out")])
    with pytest.raises(IndexError):
        cmf.main(["-i", inp, "-o", str(tmp_path / "g.out"), "--on", "gpu"])


def test_input_forms(gold, tmp_path, capsys):
    rows = gold["input_rows"]
    a = write_rows(tmp_path / "a.tsv", rows[:150])
    b = write_rows(tmp_path / "b.tsv", rows[150:151])
    z = str(tmp_path / "c.tsv.gz")
    with gzip.open(z, "wb") as f:
        f.write(("\n".join(rows[151:]) + "\n").encode())
    cpu, gpu, cpu_stdout, gpu_stdout = both_routes(tmp_path, ["-i", a, "-i", b, "-i", z, "--prob_cf", "0.2"], capsys)
    assert gpu == cpu and gpu_stdout == cpu_stdout and gpu
    d = tmp_path / "calls"
    d.mkdir()
    write_rows(d / "p1.calls.tsv", rows[:200])
    write_rows(d / "p2.calls.tsv", rows[200:])
    write_rows(d / "notes.txt", ["ignored"])
    (d / "empty.calls.tsv").write_bytes(b"")
    cpu, gpu, cpu_stdout, gpu_stdout = both_routes(tmp_path, ["-i", str(d), "--file_uid", "calls.tsv", "--sort"], capsys)
    assert gpu == cpu and gpu_stdout == cpu_stdout and gpu
    cpu, gpu, cpu_stdout, gpu_stdout = both_routes(tmp_path, ["call_freq", "-i", a, "-i", z, "--bed"], capsys, via=deepsignal.main)
    assert gpu == cpu and gpu_stdout == cpu_stdout and gpu
    assert deepsignal.main(["call_freq", "-i", a, "-o", str(tmp_path / "dev.out"), "--on", "gpu", "--device", "0"]) == 0


def test_call_mods_result_file_on_the_gpu(small_weights, tmp_path, capsys):
    """600 synthetic sites over 40 positions through call_mods on the engine, then its result file through both routes."""
    from deepsignal_amd import call_modifications as cm, synth
    from deepsignal_amd.utils.process_utils import code2base_dna
    n, npos = 600, 40
    feats = synth.synthetic_features(n, seed=77)
    tsv, calls = str(tmp_path / "features.tsv"), str(tmp_path / "calls.tsv")
    with open(tsv, "w") as f:
        for i in range(n):
            info = "chr%d\t%d\t%s\t%d\tread_%03d\tt" % (1 + (i % npos) % 3, 1000 + 7 * (i % npos), "+-"[(i % npos) % 2],
                                                       5000 - (i % npos), i // npos)
            f.write("\t".join([info, "".join(code2base_dna[int(c)] for c in feats["kmer"][i]),
                               ",".join("%s" % np.float32(x) for x in feats["means"][i]),
                               ",".join("%s" % np.float32(x) for x in feats["stds"][i]),
                               ",".join(str(int(x)) for x in feats["sanums"][i]),
                               ",".join("%s" % np.float32(x) for x in feats["signals"][i]), "1"]) + "\n")
    e = eng.Engine(max_batch=128)
    e.load_weights(small_weights)
    cm.call_mods(tsv, "unused", calls, 17, 360, 128, 0.001, 2, 1, True, True, True, True, None, engine=e)
    e.close()
    capsys.readouterr()
    cpu, gpu, cpu_stdout, gpu_stdout = both_routes(tmp_path, ["call_freq", "-i", calls], capsys, via=deepsignal.main)
    assert gpu == cpu and gpu_stdout == cpu_stdout
    assert gpu.count(b"\n") == npos
