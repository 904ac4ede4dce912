"""GPU: `evaluate --on gpu` -- the device kernels (csrc/ds_eval.hip) against the CPU checker built from the same routines, and the
command line against the cpu route and the reference script's goldens, byte for byte. Every compared value is an integer."""
import numpy as np
import pytest

from deepsignal_amd import deepsignal
from deepsignal_amd import engine as eng
from deepsignal_amd import evaluate_mods_call as ev

from evaluate_cases import case_texts, load_gold, write_inputs

pytestmark = pytest.mark.gpu

OK, HOST = eng.TEXT_ROW_OK, eng.TEXT_ROW_HOST
ALL, SAMPLE, TRUTH = eng.EVAL_SET_ALL, eng.EVAL_SET_SAMPLE, eng.EVAL_TRUTH
CF = ev.PROB_CFS


@pytest.fixture(scope="module")
def gold():
    return load_gold()


@pytest.fixture(scope="module")
def engine():
    e = eng.Engine(device=0, max_batch=64, slots=1)
    yield e
    e.close()


def row(p1, p0=None, label=None):
    """A result row around the texts p1 / p0 (default: the complement of p1 at six places), label 1 where p1 > p0 unless given."""
    if p0 is None:
        p0 = "%.6f" % (1 - float(p1))
    if label is None:
        label = int(float(p1) > float(p0))
    return "chr1\t100\t+\t900\tread\tt\t%s\t%s\t%d\tACGTACGTCGACGTACG" % (p0, p1, label)


def masks(n, seed, sample_every=None):
    """A byte per row: every row in `all`, truth at random, the sample everything or all but every sample_every-th row."""
    r = np.random.default_rng(seed)
    m = np.full(n, ALL | SAMPLE, np.uint8)
    if sample_every:
        m[::sample_every] = ALL
    m[r.random(n) < 0.5] |= TRUTH
    return m


def device_and_checker(engine, rows, mask, batch_rows, cf=CF, given=None, force_host=(), total=None):
    """The rows through eval_parse / eval_accumulate in batches, and through the checker: the device's result after every integer
    of it has been held to the checker's. given: {row: (p0, p1, called)} for the rows either leaves to the caller."""
    text = ("\n".join(rows) + "\n").encode()
    begin, end, flags, ff = eng.eval_locate(text)
    n = len(begin)
    assert n == len(rows) == len(mask)
    flags = flags.copy()
    flags[list(force_host)] = 1
    given = given or {}
    ref = eng.eval_reference(text, begin, end, flags, mask, cf, given)
    parsed = eng.eval_reference(text, begin, end, flags, mask, cf)["status"]
    assert sorted(np.flatnonzero(parsed == HOST).tolist()) == sorted(given)
    engine.eval_begin(n if total is None else total, batch_rows, cf)
    try:
        for s in range(0, n, batch_rows):
            t = min(n, s + batch_rows)
            status = engine.eval_parse(text, begin[s:t], end[s:t], flags[s:t])
            assert status.tolist() == parsed[s:t].tolist()
            over = [i for i in range(s, t) if i in given]
            engine.eval_accumulate(mask[s:t], [i - s for i in over], *([given[i][k] for i in over] for k in range(3)))
        got = engine.eval_result()
    finally:
        engine.eval_end()
    assert got["rows"] == n
    assert got["counts"].tolist() == ref["counts"].tolist()
    assert (got["u2"], got["p"], got["n"]) == (ref["u2"], ref["p"], ref["n"])
    return got


def scores_rows(values, places=6):
    return [row("%.*f" % (places, v)) for v in values]


@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257])
def test_row_counts_at_wave_and_workgroup_edges(engine, n):
    r = np.random.default_rng(n)
    got = device_and_checker(engine, scores_rows(np.round(r.random(n), 2)), masks(n, n), 1 << 20)
    assert int(got["counts"][1][:4].sum()) == n and got["p"][1] + got["n"][1] == n


def test_counters_and_table_span_four_batches(engine):
    r = np.random.default_rng(200)
    rows = scores_rows(np.round(r.random(200), 2))
    for i in range(0, 200, 5):
        rows[i] = rows[i].replace("\t1\tACG", "\t2\tACG").replace("\t0\tACG", "\t-3\tACG")
    got = device_and_checker(engine, rows, masks(200, 1), 64)
    assert got["distinct"] <= 101 and got["rows"] == 200
    assert engine.eval_times()["batches"] >= 4


def test_ties(engine):
    r = np.random.default_rng(7)
    seven = [0.1, 0.25, 0.5, 0.5000001, 0.75, 0.9, 1.0]
    m = masks(500, 2)
    got = device_and_checker(engine, scores_rows(r.choice(seven, 500), 7), m, 128)
    assert got["distinct"] == 7 and 0 < got["u2"][1] < 2 * got["p"][1] * got["n"][1]
    got = device_and_checker(engine, scores_rows([0.5] * 300), masks(300, 3), 1 << 20)
    assert got["distinct"] == 1 and got["u2"] == [got["p"][k] * got["n"][k] for k in range(2)]


def test_signed_zero_negative_and_large_scores(engine):
    rows = [row("-0.0", "0.5"), row("0.0", "0.5"), row("+0.0", "0.5"), row("-0", "0.5"), row("-0.25", "1.25"), row("-1e3", "0.5"),
            row("1.5", "-0.5"), row("1e22", "0.0"), row("-1e-22", "0.0"), row("1e-22", "0.0"), row("0.25", "0.75")]
    given = {2: (0.5, 0.0, 0)}
    m = np.array([ALL | SAMPLE | (TRUTH if i % 2 else 0) for i in range(len(rows))], np.uint8)
    got = device_and_checker(engine, rows, m, 1 << 20, given=given)
    assert got["distinct"] == 8                      # the four zeros are one score
    # -0.0 and 0.0 both through overrides: one score again, between the negative and the positive ones
    rows = [row("0.5", "0.5")] * 4
    given = {0: (0.5, -0.0, 1), 1: (0.5, 0.0, 0), 2: (0.5, -1.0, 0), 3: (0.5, 1.0, 1)}
    got = device_and_checker(engine, rows, np.array([ALL | SAMPLE | TRUTH, ALL | SAMPLE, ALL | SAMPLE, ALL | SAMPLE | TRUTH], np.uint8), 1 << 20,
                             given=given, force_host=range(4))
    assert got["distinct"] == 3 and got["u2"] == [7, 7]      # pos at 0 (1 below, tied with 1) -> 3, pos at 1 (2 below) -> 4


@pytest.mark.parametrize("distinct", [255, 256, 257, 65535, 65536, 65537])
def test_scan_levels(engine, distinct):
    """Distinct-score counts one below, at and one above each level boundary of the scan (256-element spans) that a batch of 2^20 rows
    can reach; a few scores twice so that the prefix sums are not the ranks."""
    r = np.random.default_rng(distinct)
    values = np.arange(distinct) / 100000.0
    values = np.concatenate([values, values[:: max(1, distinct // 50)]])
    r.shuffle(values)
    got = device_and_checker(engine, scores_rows(values, 5), masks(len(values), distinct, sample_every=3), 1 << 20)
    assert got["distinct"] == distinct


def test_table_at_its_load_cap(engine):
    """512 rows, 512 distinct scores, 1024 slots: the table is exactly half full."""
    values = np.arange(512) / 1000.0
    got = device_and_checker(engine, scores_rows(values, 3), masks(512, 9), 200, total=512)
    assert got["distinct"] == 512
    got = device_and_checker(engine, scores_rows(np.arange(32) / 100.0, 2), masks(32, 10), 32, total=32)      # the smallest table
    assert got["distinct"] == 32


def test_sample_differs_from_all(engine):
    r = np.random.default_rng(11)
    m = masks(1000, 4, sample_every=4)
    got = device_and_checker(engine, scores_rows(np.round(r.random(1000), 2)), m, 300)
    assert int(got["counts"][0][:4].sum()) == 750 and int(got["counts"][1][:4].sum()) == 1000
    assert got["p"][0] < got["p"][1] and got["u2"][0] != got["u2"][1]


def test_cutoff_edges_one_ulp_either_side(engine):
    """|p1 - p0| one ulp below, at and one ulp above three cut-offs, both signs, through the caller's values: exactly the rows at
    or above stand, and the sign decides `correct`."""
    given, k = {}, 0
    for c in (CF[3], CF[4], CF[27]):
        for d in (np.nextafter(c, 0), c, np.nextafter(c, 1)):
            for sign in (1.0, -1.0):
                given[k] = (0.0, float(sign * d), int(sign > 0))
                k += 1
    rows = [row("0.5", "0.5")] * k
    m = np.array([ALL | SAMPLE | (TRUTH if i % 3 else 0) for i in range(k)], np.uint8)
    got = device_and_checker(engine, rows, m, 1 << 20, given=given, force_host=range(k))
    called = got["counts"][1][4:4 + CF.size]
    assert called[3] == 16 and called[4] == 10 and called[27] == 4 and called[0] == k == 18


HOST_FORMS = [row("nan"), row("inf", "0.5"), row("1e-30"), row("+0.5"), row("1_0", "0.5"), row("0.1234567890123456"), row("0.5", "NaN"),
              row("0.5").replace("\t100\t", "\t+100\t"), row("0.5", label=1).replace("\t1\tACG", "\t1_0\tACG"), row("0.5").replace("\t900\t", "\t1234567890123456789\t"),
              row("0.5") + "\x0b", "\x1c" + row("0.5"), row("0.5").replace("read", "réad"), row("0.5") + "\r"]
UNREADABLE = ["\t".join(row("0.5").split("\t")[:9]), "", " \t "]          # Python raises on these: a kernel-level test gives them values


def test_host_rows_mixed_among_device_rows(engine):
    r = np.random.default_rng(5)
    rows = scores_rows(np.round(r.random(150), 2))
    given = {}
    for k, form in enumerate(HOST_FORMS + UNREADABLE):
        at = 3 + 9 * k
        rows[at] = form
        if form in UNREADABLE:
            given[at] = (0.25, 0.75, 1)
        else:
            p0, p1, lab = ev.row_values(ev._python_fields(form.encode()))
            given[at] = (p0, p1, int(lab != 0))
    got = device_and_checker(engine, rows, masks(150, 6, sample_every=5), 64, given=given)
    assert got["p"][1] + got["n"][1] == 150 - 2          # nan and inf as prob_1 are counted, not ranked
    # a batch whose host rows get no values is refused
    text = ("\n".join(rows[:20]) + "\n").encode()
    b, e, fl, _ = eng.eval_locate(text)
    engine.eval_begin(20, 20, CF)
    try:
        assert (engine.eval_parse(text, b, e, fl) == HOST).sum() == 2
        with pytest.raises(RuntimeError, match="left to the caller"):
            engine.eval_accumulate(np.full(20, ALL, np.uint8))
    finally:
        engine.eval_end()


def run_cli(tmp_path, capsys, paths, on, name, extra=()):
    out = str(tmp_path / name)
    capsys.readouterr()
    assert deepsignal.main(["evaluate", "--unmethylated", paths[0], "--methylated", paths[1], "--result_file", out, "--on", on, *extra]) == 0
    cap = capsys.readouterr()
    with open(out, "rb") as f:
        return f.read(), cap.out, cap.err


@pytest.mark.parametrize("idx", range(6))
def test_command_line_gpu_equals_cpu_on_the_goldens(gold, idx, tmp_path, capsys):
    case = gold["cases"][idx]
    paths = write_inputs(tmp_path, *case_texts(case))
    cpu = run_cli(tmp_path, capsys, paths, "cpu", "cpu.tsv")
    gpu = run_cli(tmp_path, capsys, paths, "gpu", "gpu.tsv", ["--device", "0"])
    assert gpu[:2] == cpu[:2] == (("\n".join(case["output"]) + "\n").encode(), case["stdout"])
    total = int(case["output"][29].split("\t")[15])
    assert gpu[2] == "--on gpu: %d of %d rows read by Python\n" % (1 if case["name"] == "nan as prob_1" else 0, total) and cpu[2] == ""


def test_command_line_subsampled_golden(gold, tmp_path, capsys):
    case = gold["cases"][6]
    paths = write_inputs(tmp_path, *case_texts(case))
    gpu = run_cli(tmp_path, capsys, paths, "gpu", "gpu.tsv", ["--seed", str(case["seed"])])
    assert gpu[:2] == (("\n".join(case["output"]) + "\n").encode(), case["stdout"])
