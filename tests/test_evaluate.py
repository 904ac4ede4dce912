"""CPU: `evaluate --on cpu` held to the reference script's own outputs (tests/golden/evaluate_golden.json, written by running
scripts/evaluate_mods_call.py), its exceptions to Python's, its sample to random.shuffle's, and its exact AUROC to scikit-learn's
trapezoid where that is installed."""
import random
import subprocess
import sys

import numpy as np
import pytest

from deepsignal_amd import deepsignal
from deepsignal_amd import evaluate_mods_call as ev

from evaluate_cases import case_texts, load_gold, run_route, write_inputs

NCASES = 7


@pytest.fixture(scope="module")
def gold():
    g = load_gold()
    assert len(g["cases"]) == NCASES
    return g


def expected(case):
    return ("\n".join(case["output"]) + "\n").encode(), case["stdout"]


@pytest.mark.parametrize("idx", range(NCASES))
def test_goldens_cpu_route(gold, idx, tmp_path, capsys):
    case = gold["cases"][idx]
    paths = write_inputs(tmp_path, *case_texts(case))
    assert run_route(tmp_path, capsys, paths, "cpu", seed=case.get("seed")) == expected(case)


def test_goldens_cover_what_they_are_for(gold):
    by_name = {c["name"]: c for c in gold["cases"]}
    auc = lambda c, row: c["output"][row].split("\t")[14]
    assert auc(by_name["perfect separation"], 1) == "1.000" and auc(by_name["inverted separation"], 1) == "0.000"
    assert auc(by_name["one class: no unmethylated call"], 29) == "0.000" and auc(by_name["nan as prob_1"], 29) == "0.000"
    sub = by_name["subsampled"]
    assert sub["output"][1].split("\t")[15] == "200000" and int(sub["output"][29].split("\t")[15]) > 200000
    assert sub["output"][1] != sub["output"][29].replace("all_sites", "_100000")
    bal = by_name["balanced, with ties"]
    assert "\t2\t" in bal["unmethylated"] and " \t " in bal["unmethylated"] and "\n \t" in bal["methylated"]
    assert [r.split("\t")[1] for r in bal["output"][1:29]] == ["%.3f" % (0.025 * k) for k in range(28)]


def test_subcommand_and_script(gold, tmp_path, capsys):
    """The golden through `deepsignal evaluate` and through the module's file run as a script."""
    case = gold["cases"][0]
    want_file, want_out = expected(case)
    paths = write_inputs(tmp_path, *case_texts(case))
    out = str(tmp_path / "r.tsv")
    capsys.readouterr()
    assert deepsignal.main(["evaluate", "--unmethylated", paths[0], "--methylated", paths[1], "--result_file", out]) == 0
    assert capsys.readouterr().out == want_out and open(out, "rb").read() == want_file
    out2 = str(tmp_path / "r2.tsv")
    got = subprocess.run([sys.executable, ev.__file__, "--unmethylated", paths[0], "--methylated", paths[1], "--result_file", out2,
                          "--num_sites", "100", "--seed", "3"], check=True, stdout=subprocess.PIPE).stdout.decode()
    rows = open(out2).read().splitlines()
    assert got.splitlines()[:2] == want_out.splitlines()[:2] and len(rows) == 30
    assert rows[1].startswith("_100\t0.000\t") and rows[1].split("\t")[15] == "200" and rows[29] == case["output"][29]
    with pytest.raises(SystemExit):
        deepsignal.main(["evaluate", "--unmethylated", paths[0], "--methylated", paths[1], "--result_file", out, "--device", "1"])
    capsys.readouterr()


def test_index_shuffle_picks_the_rows_the_script_picks():
    """random.shuffle of a list of records and of a list of indices draw the same numbers: after random.seed(s) the script's first
    num_sites records of each file are ours."""
    for seed, n_un, n_me, num in ((7, 50, 31, 20), (8, 10, 40, 25), (9, 3, 2, 2)):
        random.seed(seed)
        un, me = ["u%d" % i for i in range(n_un)], ["m%d" % i for i in range(n_me)]
        random.shuffle(un)
        random.shuffle(me)
        for rng in (random.Random(seed), None):
            if rng is None:
                random.seed(seed)
                rng = random
            picks = ev.sample_rows(n_un, n_me, num, rng)
            assert ["u%d" % i for i in picks[0]] == un[:num] and ["m%d" % i for i in picks[1]] == me[:num]
    state = random.getstate()
    picks = ev.sample_rows(5, 7, 7, random)          # nothing to choose: no number is drawn
    assert [p.tolist() for p in picks] == [list(range(5)), list(range(7))] and random.getstate() == state


ROW = "chr1\t100\t+\t900\tread\tt\t0.25\t0.75\t1\tACGTACGTCGACGTACG"


@pytest.mark.parametrize("bad,exc,text", [("\n", IndexError, "list index out of range"),
                                          ("chr1\t100\t+\t900\tread\tt\t0.25\t0.75\t1\n", IndexError, "list index out of range"),
                                          (ROW.replace("\t100\t", "\tx\t") + "\n", ValueError, "invalid literal for int() with base 10: 'x'"),
                                          (ROW.replace("0.75", "0.7.5") + "\n", ValueError, "could not convert string to float: '0.7.5'"),
                                          ("chr1\tx\n", ValueError, "invalid literal for int() with base 10: 'x'")])
def test_malformed_rows_raise_what_the_script_raises(bad, exc, text, tmp_path, capsys):
    """ModRecord's order of evaluation: fields[0], int(fields[1]), fields[2], int(fields[3]) ... fields[9]. A bad row in the second
    file comes after the first file's line on stdout."""
    paths = write_inputs(tmp_path, ROW + "\n", ROW + "\n" + bad + ROW + "\n")
    capsys.readouterr()
    with pytest.raises(exc) as info:
        ev.evaluate_cpu(paths[0], paths[1], str(tmp_path / "r.tsv"))
    assert text in str(info.value)
    assert capsys.readouterr().out == "there are 1 basemod candidates totally\n"


def test_empty_tested_set_is_the_scripts_zero_division(tmp_path, capsys):
    paths = write_inputs(tmp_path, "", "")
    with pytest.raises(ZeroDivisionError):
        ev.evaluate_cpu(paths[0], paths[1], str(tmp_path / "r.tsv"))
    assert capsys.readouterr().out == "there are 0 basemod candidates totally\n" * 2 + "0 0 0 0\n"
    paths = write_inputs(tmp_path, ROW + "\n", ROW + "\n")
    with pytest.raises(ZeroDivisionError):
        ev.evaluate_cpu(paths[0], paths[1], str(tmp_path / "r.tsv"), num_sites=0)


def test_cutoffs_are_numpys_own_doubles():
    assert ev.PROB_CFS.size == 28 and ev.PROB_CFS[3] != 0.075 and ev.PROB_CFS[3] == 3 * 0.025
    p0, p1 = np.array([0.0, 0.075]), np.array([0.075, 0.0])      # |p1 - p0| is the literal 0.075, below 3 * 0.025 = 0.07500000000000001
    assert 0.075 >= 0.075 and not 0.075 >= ev.PROB_CFS[3]
    st = ev.set_stats(p0, p1, np.array([True, False]), np.array([True, False]))
    assert st.called[:5] == [2, 2, 2, 0, 0] and st.correct[:5] == [2, 2, 2, 0, 0]
    st = ev.set_stats(np.array([0.5]), np.array([float("nan")]), np.array([True]), np.array([True]))
    assert st.called == [0] * 28 and st.auroc == 0


def test_exact_auc_small_cases():
    assert ev.exact_auc([0.1, 0.2, 0.3, 0.4], [False, False, True, True]) == 1.0
    assert ev.exact_auc([0.4, 0.3, 0.2, 0.1], [False, False, True, True]) == 0.0
    assert ev.exact_auc([0.5, 0.5, 0.5], [False, True, True]) == 0.5
    assert ev.exact_auc([-0.0, 0.0], [False, True]) == 0.5
    assert ev.exact_auc([0.1, 0.2], [True, True]) == 0 and ev.exact_auc([0.1, float("inf")], [False, True]) == 0
    assert ev.exact_auc([0.1, float("nan")], [False, True]) == 0 and ev.exact_auc([], []) == 0
    assert ev.exact_auc_parts(np.array([0.1, 0.2, 0.2, 0.3]), np.array([False, True, False, True])) == (2 * 1 + 1 + 2 * 2, 2, 2)


def test_exact_auc_is_sklearns_trapezoid():
    metrics = pytest.importorskip("sklearn.metrics")
    rng = np.random.default_rng(12)
    for n, places in ((2, 1), (50, 1), (400, 2), (3000, 2), (3000, 8), (20000, 3)):
        for _ in range(4):
            truth = rng.random(n) < rng.uniform(0.2, 0.8)
            truth[0], truth[1] = True, False
            scores = np.round(np.clip(rng.normal(0.4 + 0.2 * truth, 0.25), -0.2, 1.2), places)
            assert abs(ev.exact_auc(scores, truth) - metrics.roc_auc_score(truth, scores)) <= 1e-12
