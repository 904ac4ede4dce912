"""CPU: the host half of `evaluate --on gpu` held to Python -- ds_eval_locate (rows, flags, the bare carriage return) and
ds_eval_reference (the routines the device kernels are built from), and the Python glue of the gpu route run on top of the checker.
The reference script's own outputs (tests/golden/evaluate_golden.json) and the cpu route are the yardsticks."""
import re

import numpy as np
import pytest

from deepsignal_amd import call_modification_frequency as cmf
from deepsignal_amd import engine as eng
from deepsignal_amd import evaluate_mods_call as ev

from evaluate_cases import CheckerBackend, call_row, case_texts, load_gold, run_route, write_inputs

OK, HOST = eng.TEXT_ROW_OK, eng.TEXT_ROW_HOST
ALL, SAMPLE, TRUTH = eng.EVAL_SET_ALL, eng.EVAL_SET_SAMPLE, eng.EVAL_TRUTH
ROW = "chr1\t100\t+\t900\tread\tt\t0.25\t0.75\t1\tACGTACGTCGACGTACG"


@pytest.fixture(scope="module")
def gold():
    return load_gold()


@pytest.mark.parametrize("idx", range(7))
def test_goldens_through_the_checker(gold, idx, tmp_path, capsys):
    case = gold["cases"][idx]
    paths = write_inputs(tmp_path, *case_texts(case))
    info = {}
    got = run_route(tmp_path, capsys, paths, "gpu", seed=case.get("seed"), batch_rows=64 if idx < 6 else 1 << 16, info=info,
                    make_engine=CheckerBackend)
    assert got == (("\n".join(case["output"]) + "\n").encode(), case["stdout"])
    assert info["host_rows"] == (1 if case["name"] == "nan as prob_1" else 0)
    assert info["rows"] == int(case["output"][29].split("\t")[15])


def hostile_rows(r, n):
    """Result rows in every form the two routes must agree on, most of them plain."""
    rows = []
    for k in range(n):
        u = r.random()
        p1 = "%.*f" % (int(r.integers(1, 7)), r.random())
        if u < 0.6:
            rows.append(call_row(r, p1))
        elif u < 0.7:
            rows.append(call_row(r, p1, sep=["  ", " \t", "\t\t", " "][int(r.integers(0, 4))]))
        elif u < 0.8:
            rows.append(["  ", "\t", ""][int(r.integers(0, 3))] + call_row(r, p1) + ["  ", "\t x y", "\x0c", " \x0b"][int(r.integers(0, 4))])
        else:
            p1 = ["nan", "inf", "-inf", "1e-30", "+0.5", "1_0.5", "0.1234567890123456", "-0.0", "1.5", "-0.25", "5e-1", ".5", "1.",
                  "0.50", "Infinity", "NaN"][int(r.integers(0, 16))]
            lab = ["0", "1", "2", "-1", "+1", "1_0", "00", "1234567890", " 1"][int(r.integers(0, 9))]
            rows.append(call_row(r, p1, p0_text=["0.5", "-0.0", "1e2", "nan"][int(r.integers(0, 4))], label=0).replace("\t0\tACG", "\t%s\tACG" % lab))
    return rows


@pytest.mark.parametrize("seed,n_un,n_me,num_sites,batch", [(1, 1, 1, 100000, 64), (2, 300, 200, 100000, 64), (3, 700, 900, 250, 256),
                                                             (4, 1500, 40, 100, 1 << 20), (5, 64, 65, 64, 7)])
def test_random_files_gpu_route_equals_cpu_route(seed, n_un, n_me, num_sites, batch, tmp_path, capsys):
    r = np.random.default_rng(seed)
    paths = write_inputs(tmp_path, "\n".join(hostile_rows(r, n_un)) + "\n", "\r\n".join(hostile_rows(r, n_me)))
    cpu = run_route(tmp_path, capsys, paths, "cpu", seed=seed, num_sites=num_sites)
    info = {}
    gpu = run_route(tmp_path, capsys, paths, "gpu", seed=seed, num_sites=num_sites, batch_rows=batch, info=info, make_engine=CheckerBackend)
    assert gpu == cpu
    assert info["rows"] == n_un + n_me and (n_un < 100 or 0 < info["host_rows"] < info["rows"] - 100)


def test_checker_counts_equal_the_cpu_routes_integers():
    """ds_eval_reference against set_stats, integer for integer: counts per cut-off and U2 / P / N, with a sample that leaves rows out."""
    for seed in range(4):
        r = np.random.default_rng(100 + seed)
        rows = [call_row(r, "%.2f" % v) for v in r.random(900)]
        for i in range(0, 900, 7):
            f = rows[i].split("\t")
            f[8] = "2" if i % 2 else "0"
            rows[i] = "\t".join(f)
        text = ("\n".join(rows) + "\n").encode()
        begin, end, flags, ff = eng.eval_locate(text)
        truth = r.random(900) < 0.45
        sample = r.random(900) < 0.7
        mask = (ALL + SAMPLE * sample + TRUTH * truth).astype(np.uint8)
        out = eng.eval_reference(text, begin, end, flags, mask, ev.PROB_CFS)
        assert ff == 0 and (out["status"] == OK).all()
        vals = [ev.row_values(x.split()) for x in rows]
        p0, p1, lab = (np.array([v[k] for v in vals]) for k in range(3))
        assert out["p0"].tolist() == p0.tolist() and out["p1"].tolist() == p1.tolist() and out["called"].tolist() == (lab != 0).tolist()
        for k, member in enumerate((sample, np.ones(900, bool))):
            st = ev.set_stats(p0[member], p1[member], lab[member] != 0, truth[member])
            assert out["counts"][k].tolist() == [st.tp, st.fp, st.tn, st.fn] + st.called + st.correct
            assert (out["u2"][k], out["p"][k], out["n"][k]) == ev.exact_auc_parts(p1[member], truth[member])


FLOATS = ["0", "1", "0.5", "-0.5", "-0.0", "0.0", "1.", ".5", "-.5", "1e0", "1E-2", "5e+1", "1e22", "1e-22", "1e23", "1e-23", "123456789012345",
          "1234567890123456", "0.000000000000001", "00.5", "1.5e3", "1e400", "1e-30", "1e-400", "nan", "NaN", "inf", "-inf", "Infinity", "+1", "+.5",
          "1_0", "1_0.5", "0x10", "1e", "e5", ".", "-", "", "1..2", "1e5.0", "--1", "0.5f", "١"]
INTS = ["0", "1", "-1", "2", "007", "-0", "123456789", "1234567890", "999999999999999999", "1000000000000000000", "+1", "1_0", "1.0", "x", "-",
        "1e3", "0x1", "٣"]


def python_says(raw: bytes):
    try:
        return ev.row_values(ev._python_fields(raw))
    except (ValueError, IndexError):
        return None


def checker_says(raw: bytes):
    begin, end, flags, ff = eng.eval_locate(raw)
    assert len(begin) == 1
    out = eng.eval_reference(raw, begin, end, flags, np.array([ALL], np.uint8), ev.PROB_CFS)
    if out["status"][0] != OK:
        return None
    return float(out["p0"][0]), float(out["p1"][0]), int(out["called"][0])


def same(a: float, b: float) -> bool:
    return np.float64(a).tobytes() == np.float64(b).tobytes()


def test_every_token_rule_is_pythons():
    """A row the checker takes has the values Python reads, bit for bit; a row Python refuses is never taken; the plain forms are
    taken and the forms outside the device grammar are left to Python."""
    f = ROW.split("\t")
    for col, tokens in ((6, FLOATS), (7, FLOATS), (1, INTS), (3, INTS), (8, INTS)):
        for tok in tokens:
            if tok == "":
                continue
            g = list(f)
            g[col] = tok
            raw = "\t".join(g).encode()
            want, got = python_says(raw), checker_says(raw)
            if got is not None:
                assert want is not None, (col, tok)
                assert same(got[0], want[0]) and same(got[1], want[1]) and got[2] == int(want[2] != 0), (col, tok)
    for tok in ("0", "0.5", "-0.0", "1.", ".5", "1E-2", "1e22", "1e-22", "123456789012345", "00.5"):
        assert checker_says(ROW.replace("0.75", tok).encode()) is not None, tok
    for tok in ("nan", "inf", "1e-30", "+0.5", "1_0", "1234567890123456", "1e23"):
        raw = ROW.replace("0.75", tok).encode()
        assert checker_says(raw) is None and python_says(raw) is not None, tok
    for lab, called in (("0", 0), ("1", 1), ("2", 1), ("-1", 1), ("-0", 0), ("00", 0)):
        assert checker_says(ROW.replace("\t1\tACG", "\t%s\tACG" % lab).encode())[2] == called
    assert checker_says("\t".join(f[:9]).encode()) is None and python_says("\t".join(f[:9]).encode()) is None      # too few fields
    assert checker_says(("  " + ROW.replace("\t", " \t  ") + " \t extra  ").encode()) == (0.25, 0.75, 1)


def test_locate_follows_pythons_split_and_line_rules():
    """Every byte value at the start, in the middle and at the end of a row: an unflagged row's fields between runs of space or tab
    are line.rstrip().split()'s; a flagged row is one of the listed kinds."""
    assert [c for c in range(128) if chr(c).isspace()] == [9, 10, 11, 12, 13, 28, 29, 30, 31, 32]
    special = {0x0b, 0x0c, 0x0d, 0x1c, 0x1d, 0x1e, 0x1f}
    for c in range(256):
        if c == 10:
            continue
        ch = bytes([c])
        for raw in (ch + ROW.encode(), ROW.encode().replace(b"read", b"re" + ch + b"ad"), ROW.encode() + ch, ch):
            begin, end, flags, ff = eng.eval_locate(raw)
            assert begin.tolist() == [0] and end.tolist() == [len(raw)]
            blank = raw.strip(b" \t") == b""
            assert bool(flags[0]) == (c >= 0x80 or c in special or blank), (c, raw)
            assert bool(ff & eng.EVAL_BARE_CR) == (c == 13 and not raw.endswith(b"\r")), (c, raw)
            if not flags[0]:
                assert [t for t in re.split(b"[ \t]+", raw) if t] == [t.encode() for t in ev._python_fields(raw)], (c, raw)
    b, e, fl, ff = eng.eval_locate(b"a b\r\n\n  \t\nc\n\nd")
    assert list(zip(b.tolist(), e.tolist())) == [(0, 4), (5, 5), (6, 9), (10, 11), (12, 12), (13, 14)] and fl.tolist() == [1, 1, 1, 0, 1, 0] and ff == 0
    assert [len(eng.eval_locate(t)[0]) for t in (b"", b"\n", b"a", b"a\n", b"a\n\n")] == [0, 1, 1, 1, 2]
    assert eng.eval_locate(b"a\rb\n")[3] == eng.EVAL_BARE_CR and eng.eval_locate(b"a\r\r\nb")[3] == eng.EVAL_BARE_CR
    assert eng.eval_locate(b"a\r\nb\r")[3] == 0
    big = ("\n".join(["x"] * 5000)).encode()                      # more rows than the first guess
    assert len(eng.eval_locate(big)[0]) == 5000


def test_host_rows_raise_and_fall_back_as_the_cpu_route(tmp_path, capsys):
    for bad, exc in (("\n", IndexError), ("chr1\t1\t+\t2\tr\tt\t0.5\t0.5\t1\n", IndexError), (ROW.replace("\t100\t", "\tx\t") + "\n", ValueError)):
        paths = write_inputs(tmp_path, ROW + "\n", ROW + "\n" + bad + ROW + "\n")
        capsys.readouterr()
        with pytest.raises(exc):
            ev.evaluate_gpu(paths[0], paths[1], str(tmp_path / "r.tsv"), make_engine=CheckerBackend)
        assert capsys.readouterr().out == "there are 1 basemod candidates totally\n"
    paths = write_inputs(tmp_path, "", "")
    with pytest.raises(ZeroDivisionError):
        ev.evaluate_gpu(paths[0], paths[1], str(tmp_path / "r.tsv"), make_engine=CheckerBackend)
    assert capsys.readouterr().out == "there are 0 basemod candidates totally\n" * 2 + "0 0 0 0\n"
    paths = write_inputs(tmp_path, ROW + "\n", ROW + "\rx\n")
    with pytest.raises(cmf._CpuRoute, match="bare carriage return"):
        ev.evaluate_gpu(paths[0], paths[1], str(tmp_path / "r.tsv"), make_engine=CheckerBackend)
    assert capsys.readouterr().out == ""


def test_checker_arguments():
    text = (ROW + "\n").encode()
    b, e, fl, _ = eng.eval_locate(text)
    with pytest.raises(ValueError):
        eng.eval_reference(text, b, e, fl, np.array([8], np.uint8), ev.PROB_CFS)
    with pytest.raises(ValueError):
        eng.eval_reference(text, b, e, fl, np.array([ALL], np.uint8), np.zeros(33))
    out = eng.eval_reference(text, b, e, np.array([1], np.uint8), np.array([ALL | TRUTH], np.uint8), [0.0, 0.6])
    assert out["status"].tolist() == [HOST] and out["counts"].tolist() == [[0] * 8, [0] * 8]
    out = eng.eval_reference(text, b, e, np.array([1], np.uint8), np.array([ALL | TRUTH], np.uint8), [0.0, 0.6], {0: (0.2, float("inf"), 5)})
    assert out["counts"].tolist() == [[0] * 8, [1, 0, 0, 0, 1, 1, 1, 1]] and out["p"] == [0, 0]       # counted, kept out of the scores
    out = eng.eval_reference(b"", [], [], [], [], [0.0])
    assert out["counts"].tolist() == [[0] * 6, [0] * 6] and out["u2"] == [0, 0]


def test_bare_carriage_return_takes_the_cpu_route_whole_and_says_so(tmp_path, capsys):
    """Found by ds_eval_locate before a device is opened: `--on gpu` on such a file needs no GPU, and its stdout stays the script's."""
    from deepsignal_amd import deepsignal
    paths = write_inputs(tmp_path, ROW + "\n" + ROW.replace("0.75", "0.25") + "\r" + ROW + "\n", ROW + "\n")
    outs = []
    for on in ("cpu", "gpu"):
        out = str(tmp_path / (on + ".tsv"))
        capsys.readouterr()
        assert deepsignal.main(["evaluate", "--unmethylated", paths[0], "--methylated", paths[1], "--result_file", out, "--on", on]) == 0
        cap = capsys.readouterr()
        outs.append((open(out, "rb").read(), cap.out))
        assert ("bare carriage return" in cap.err and "running the cpu route" in cap.err) == (on == "gpu")
    assert outs[0] == outs[1] and outs[0][1].startswith("there are 3 basemod candidates totally\n")
