"""CPU: the host half of `call_freq --on gpu` held to Python -- ds_freq_locate (rows, chromosome ids, flags) and ds_freq_reference
(the row grammar and the aggregation the device kernels are built from), plus the Python glue of the gpu route run on top of the
checker. The reference script's own outputs (tests/golden/frequency_golden.json) are the yardstick for the tables."""
import io
import json
import os

import numpy as np
import pytest

from deepsignal_amd import call_modification_frequency as cmf
from deepsignal_amd import engine as eng

from freq_cases import KMER, ReferenceBackend, bits, call_row, random_rows, stats_tuple

GOLD = os.path.join(os.path.dirname(__file__), "golden", "frequency_golden.json")
OK, HOST = eng.TEXT_ROW_OK, eng.TEXT_ROW_HOST


@pytest.fixture(scope="module")
def gold():
    with open(GOLD) as f:
        return json.load(f)


def checker_stats(files, prob_cf=0.0, batch_rows=1 << 20, info=None):
    return cmf.calculate_mods_frequency_gpu(files, prob_cf, batch_rows=batch_rows, info=info, make_engine=ReferenceBackend)


def rows_status(rows, chrom=None):
    text = ("\n".join(rows) + "\n").encode()
    begin, end, c, flags, names = eng.freq_locate(text)
    assert len(begin) == len(rows)
    return eng.freq_reference(text, begin, end, c if chrom is None else chrom, flags)


@pytest.mark.parametrize("idx", [0, 1, 2, 3])
def test_goldens_through_the_checker(gold, idx, tmp_path, capsys):
    case = gold["cases"][idx]
    inp, out = str(tmp_path / "calls.tsv"), str(tmp_path / "freq.tsv")
    with open(inp, "w") as f:
        f.write("\n".join(gold["input_rows"]) + "\n")
    ap_cf = float(case["flags"][case["flags"].index("--prob_cf") + 1]) if "--prob_cf" in case["flags"] else 0.0
    cpu = cmf.calculate_mods_frequency([inp], ap_cf)
    cpu_out = capsys.readouterr().out
    info = {}
    stats = checker_stats([inp], ap_cf, batch_rows=64, info=info)
    assert capsys.readouterr().out == cpu_out                    # the "calls used" line
    assert info["host_rows"] == 0
    assert stats_tuple(stats) == stats_tuple(cpu)                # dict order = unsorted output order
    cmf.write_sitekey2stats(stats, out, "--sort" in case["flags"], "--bed" in case["flags"])
    assert open(out).read().splitlines() == case["output"]


@pytest.mark.parametrize("seed,nrows,nsites,nchrom", [(1, 1, 1, 1), (2, 37, 5, 2), (3, 500, 300, 5), (4, 2000, 120, 3),
                                                      (5, 2000, 1, 1)])
def test_random_files_bit_equal(seed, nrows, nsites, nchrom, tmp_path, capsys):
    rows = random_rows(seed, nrows, nsites, nchrom)
    inp = str(tmp_path / "calls.tsv")
    with open(inp, "w") as f:
        f.write("\n".join(rows) + "\n")
    for cf in (0.0, 0.3):
        cpu = cmf.calculate_mods_frequency([inp], cf)
        got = checker_stats([inp], cf, batch_rows=256)
        assert stats_tuple(got) == stats_tuple(cpu)


def _digits(rng, n):
    return str(int(rng.integers(1, 10))) + "".join(str(int(d)) for d in rng.integers(0, 10, n - 1))


def test_accepted_tokens_are_float_bit_for_bit():
    rng = np.random.default_rng(7)
    toks = ["0.0", "1.0", "-0.0", "0", "1", "1.", ".5", "-.5", "007.50", "1e22", "1e-22", "1E+5", "123456789012345e-22", "1.23456789012345e36",
            "0.000000000000000000001", "9.999999e-08", "2.5e-05", "0.99999994"]
    for n in range(1, 16):
        for _ in range(12):
            d = _digits(rng, n)
            cut = int(rng.integers(0, n + 1))
            t = d[:cut] + ("." + d[cut:] if cut < n or rng.random() < 0.3 else "")
            if rng.random() < 0.4:
                frac = n - cut
                t += "e%+d" % int(rng.integers(-22 + frac, 22 + frac + 1))      # net exponent in [-22, 22]
            toks.append(("-" if rng.random() < 0.2 else "") + t)
    toks += [str(np.float32(x)) for x in rng.random(200)] + [str(np.float32(10.0 ** -x)) for x in rng.uniform(3, 13, 100)]
    out = rows_status([call_row("chr1", 5, t, "0.5", label=1) for t in toks])
    assert (out["status"] == OK).all(), [t for t, s in zip(toks, out["status"]) if s != OK]
    for t, v in zip(toks, out["row_p0"]):
        assert bits(float(v)) == bits(float(t)), t
    assert bits(float(out["row_p0"][2])) == bits(-0.0)


HOSTILE_PROBS = ["2.7581529e-17", "123456789012345e-23", "1.23456789012345e37", "nan", "inf", "-inf", "1e-30", "1e23", "1e-23", "+0.5", "0_5", "1234567890123456", "", ".", "-", "1e", "0x1p-1",
                 "0.5 ", "1.2.3", "٠.٥"]


def test_forms_outside_the_grammar_are_host_rows():
    rows = [call_row("chr1", 5, t, "0.5", label=1) for t in HOSTILE_PROBS]
    rows += [call_row("chr1", 5, "0.5", t, label=1) for t in ("nan", "1e-30")]
    rows += [call_row("chr1", p, "0.25", "0.75") for p in ("+5", "5_0", str(1 << 40), "-1", "1" * 19, "5.0", "")]
    rows += ["\t".join(call_row("chr1", 5, "0.25", "0.75").split("\t")[:k]) for k in (1, 8, 9)]
    rows += [call_row("chr1", 5, "0.25", "0.75", label=t) for t in ("+1", "1.0", "1234567890", "x")]
    rows += [call_row("chr1", 5, "0.25", "0.75", pis="9x")]
    out = rows_status(rows)
    assert (out["status"] == HOST).all(), [r for r, s in zip(rows, out["status"]) if s != HOST]
    assert len(out["first_row"]) == 0 and out["used"] == 0
    # positions at the edges of the key, a negative zero, extra columns: the device takes them
    good = [call_row("chr1", 0, "0.25", "0.75"), call_row("chr1", (1 << 40) - 1, "0.25", "0.75"), call_row("chr1", "-0", "0.25", "0.75"),
            call_row("chr1", "007", "0.25", "0.75") + "\textra\tcolumns", call_row("chr1", 5, "0.25", "0.75", label="-1")]
    out = rows_status(good)
    assert (out["status"] == OK).all()
    assert out["row_pos"].tolist() == [0, (1 << 40) - 1, 0, 7, 5] and out["row_met"].tolist() == [1, 1, 1, 1, 0]
    # chromosome ids outside [0, 2^23)
    out = rows_status(good[:3], chrom=[(1 << 23) - 1, 1 << 23, -1])
    assert out["status"].tolist() == [OK, HOST, HOST]


def test_locate_agrees_with_python_lines():
    body = [call_row("chr2", 1, 0.2, 0.8), call_row("chr1", 2, 0.2, 0.8), call_row("chr2", 3, 0.2, 0.8), " " + call_row("chrS", 4, 0.2, 0.8),
            call_row("chr1", 5, 0.2, 0.8) + "\r", "", call_row("chré", 6, 0.2, 0.8), call_row("chr1", 7, 0.2, 0.8) + "\t",
            "a\rb", call_row("chr3", 8, 0.2, 0.8) + "\x1c", call_row("chr3", 9, 0.2, 0.8)]
    for tail in ("\n", ""):
        data = ("\n".join(body) + tail).encode("utf-8")
        begin, end, chrom, flags, names = eng.freq_locate(data)
        assert [data[b:e] for b, e in zip(begin, end)] == [r.encode("utf-8") for r in body]
        assert flags.tolist() == [0, 0, 0, 1, 1, 1, 1, 1, 1, 1, 0]
        assert names == [b"chr2", b"chr1", b"chr3"]              # first-appearance order, flagged rows register nothing
        assert chrom.tolist() == [0, 1, 0, -1, -1, -1, -1, -1, -1, -1, 2]
        # an unflagged row is one Python line whose strip() changes nothing
        for b, e, f in zip(begin, end, flags):
            lines = list(io.TextIOWrapper(io.BytesIO(data[b:e] + b"\n"), encoding="utf-8"))
            if not f:
                assert len(lines) == 1 and lines[0].strip() == data[b:e].decode("ascii")
    for data, n in ((b"", 0), (b"\n", 1), (b"x", 1), (b"x\n\n", 2)):
        begin, end, chrom, flags, names = eng.freq_locate(data)
        assert len(begin) == n == len(io.BytesIO(data).readlines())
    trunc = ("\n".join(body[:3]) + "\n").encode()[:-20]         # cut in the middle of a row
    begin, end, chrom, flags, names = eng.freq_locate(trunc)
    assert len(begin) == 3 and end[-1] == len(trunc)


def test_host_rows_take_the_cpu_routes_expressions(tmp_path, capsys):
    rows = [call_row("chr1", 10, 0.3, 0.7), call_row("chr1", 10, "nan", "0.5", label=1), call_row("chr1", 10, "1e-30", "inf", label=0),
            " " + call_row("chr1", 10, "+0.5", "0.25", label=1), call_row("chr1", 1 << 40, 0.1, 0.9), call_row("chr1", 10, 0.6, 0.4) + "\r",
            call_row("chr1", -3, 0.1, 0.9), call_row("chr1", 1 << 40, 0.2, 0.8), call_row("chr9", "1_0", 0.2, 0.8),
            "\t".join(call_row("chr1", 10, 0.45, 0.55).split("\t")[:9])]       # nine columns: fine unless it opens a site
    inp = str(tmp_path / "calls.tsv")
    with open(inp, "wb") as f:
        f.write(("\n".join(rows) + "\n").encode())
    for cf in (0.0, 0.2):
        cpu = cmf.calculate_mods_frequency([inp], cf)
        cpu_out = capsys.readouterr().out
        info = {}
        got = checker_stats([inp], cf, batch_rows=4, info=info)
        out = capsys.readouterr().out
        assert stats_tuple(got) == stats_tuple(cpu)
        assert info["host_rows"] == 9
        assert out.splitlines()[-1] == cpu_out.splitlines()[-1] and "9 row(s) parsed on the host" in out
    assert ("chr1", 1 << 40) in cpu and ("chr1", -3) in cpu and ("chr9", 10) in cpu


def test_malformed_rows_raise_as_the_cpu_route(tmp_path):
    good = call_row("chr1", 10, 0.3, 0.7)
    for bad, exc in (("\t".join(good.split("\t")[:8]), IndexError), ("", IndexError), (call_row("chr1", "x", 0.3, 0.7), ValueError),
                     (call_row("chr1", 10, "zero", 0.7), ValueError), (call_row("chr2", 10, 0.3, 0.7, pis="9x"), ValueError)):
        inp = str(tmp_path / "calls.tsv")
        with open(inp, "w") as f:
            f.write("\n".join([good, good, bad, good]) + "\n")
        with pytest.raises(exc):
            cmf.calculate_mods_frequency([inp])
        with pytest.raises(exc):
            checker_stats([inp], batch_rows=2)


def test_bare_carriage_return_goes_the_cpu_route(tmp_path, capsys):
    a, b = call_row("chr1", 10, 0.3, 0.7), call_row("chr1", 11, 0.3, 0.7)
    inp, out1, out2 = str(tmp_path / "calls.tsv"), str(tmp_path / "a.tsv"), str(tmp_path / "b.tsv")
    with open(inp, "wb") as f:
        f.write((a + "\r" + b + "\n" + a + "\n").encode())
    with pytest.raises(cmf._CpuRoute):
        checker_stats([inp])
    assert cmf.main(["-i", inp, "-o", out1]) == 0
    assert open(out1).read().count("\n") == 2


def test_flag_validation(tmp_path):
    inp = str(tmp_path / "calls.tsv")
    open(inp, "w").write(call_row("chr1", 10, 0.3, 0.7) + "\n")
    for argv in (["--device", "0"], ["--on", "tpu"], ["--on", "gpu", "--device", "-1"], ["--on", "gpu", "--prob_cf", "nan"]):
        with pytest.raises(SystemExit):
            cmf.main(["-i", inp, "-o", str(tmp_path / "o.tsv")] + argv)
    from deepsignal_amd import deepsignal
    with pytest.raises(SystemExit):
        deepsignal.main(["call_freq", "-i", inp, "-o", str(tmp_path / "o.tsv"), "--device", "1"])
    assert deepsignal.main(["call_freq", "-i", inp, "-o", str(tmp_path / "o.tsv"), "--sort"]) == 0
    assert open(str(tmp_path / "o.tsv")).read().startswith("chr1\t10\t+\t990\t")
    e = object.__new__(eng.Engine)                               # argument checks come before any library call
    for call in (lambda: eng.Engine.freq_begin(e, 0, 16), lambda: eng.Engine.freq_begin(e, 16, 0),
                 lambda: eng.Engine.freq_begin(e, 16, 16, float("nan")), lambda: eng.Engine.freq_begin(e, (1 << 30) + 1, 16)):
        with pytest.raises(ValueError):
            call()
    with pytest.raises(ValueError):
        cmf.calculate_mods_frequency_gpu([inp], batch_rows=0, make_engine=ReferenceBackend)
