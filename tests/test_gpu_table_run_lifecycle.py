"""GPU: the call order of a table run -- ds_{freq,combine,eval}_{begin,parse,accumulate,result,end} -- pinned per route: what each
call refuses and in which words, that a refused call leaves the run as it was, and what the time getters count. Every refusal here
is made on the host before any device work; the runs are three rows in batches of two. The expected texts are literals."""
import math

import numpy as np
import pytest

from deepsignal_amd import combine_strands as cs
from deepsignal_amd import engine as eng

from combine_cases import table_row, write_bytes
from freq_cases import call_row

pytestmark = pytest.mark.gpu

OK, HOST = eng.TEXT_ROW_OK, eng.TEXT_ROW_HOST
DS_OK, DS_ERR_INVALID = 0, -1
TOTAL, BATCH = 3, 2
CALLS = [call_row("chr1", 10, 0.25, 0.75), call_row("chr2", 20, 0.75, 0.25), call_row("chr1", 10, 0.125, 0.875)]
FASTA = b">c1\nAACGTTAATTAATTAATTAATTAATTAATTAATT\n"
TABLE = [table_row("c1", 2, "+"), table_row("c1", 3, "-", "0.500", "0.250", 2, 1, 3), table_row("c1", 2, "+", "0.125", "3.000", 0, 5, 5)]
CF = np.array([0.0, 0.5], np.float64)
MASK = np.array([eng.EVAL_SET_SAMPLE | eng.EVAL_SET_ALL | eng.EVAL_TRUTH, eng.EVAL_SET_ALL, eng.EVAL_SET_ALL | eng.EVAL_TRUTH], np.uint8)


class Route:
    """One route's calls under one set of names. begin .. times go through Engine; raw_* call the library entry as Engine does,
    past Engine's own checks, with valid arrays of the right sizes, and return the code."""
    name = ""
    site_fields = ()

    def __init__(self, e):
        self.e, self.lib, self.h = e, e._lib, e._h

    def error(self) -> str:
        return self.lib.ds_last_error(self.h).decode()

    def refused(self, rc, what: str) -> None:
        assert rc == DS_ERR_INVALID and self.error() == what

    def raises(self, call, what: str) -> None:
        """An Engine call that reaches the library and is refused there."""
        with pytest.raises(RuntimeError) as info:
            call()
        assert str(info.value).endswith("failed (%d): %s" % (DS_ERR_INVALID, what))

    def end(self):
        getattr(self.e, self.name + "_end")()

    def raw_end(self) -> int:
        return getattr(self.lib, "ds_%s_end" % self.name)(self.h)

    def times(self, reset=False) -> dict:
        return getattr(self.e, self.name + "_times")(reset)

    def result(self) -> dict:
        return getattr(self.e, self.name + "_result")()

    def rest_and_check(self, done: int) -> None:
        """Carry the open run, `done` rows of it accumulated and no batch pending, to its end: the result is the checker's."""
        for s in range(done, TOTAL, BATCH):
            assert HOST not in self.parse(s, min(TOTAL, s + BATCH)).tolist()
            self.accumulate()
        got = self.result()
        self.end()
        self.check(got)

    def ordered(self, d):
        order = np.lexsort((d["pos"], d["chrom"]))
        return [d[k][order].tobytes() for k in self.site_fields]


class FreqRoute(Route):
    name = "freq"
    site_fields = ("first_row", "chrom", "pos", "sum0", "sum1", "met", "unmet")

    def __init__(self, e, tmp_path=None):
        Route.__init__(self, e)
        self.text = ("\n".join(CALLS) + "\n").encode()
        self.b, self.en, self.chrom, self.flags, names = eng.freq_locate(self.text)
        assert len(self.b) == TOTAL

    def begin(self, total=TOTAL, batch=BATCH):
        self.e.freq_begin(total, batch, 0.0)

    def raw_begin(self, total, batch) -> int:
        return self.lib.ds_freq_begin(self.h, total, batch, 0.0)

    def parse(self, s, t):
        return self.e.freq_parse(self.text, self.b[s:t], self.en[s:t], self.chrom[s:t], self.flags[s:t])

    def raw_parse(self, s, t) -> int:
        keep, addr, b, en, chrom, flags = eng._batch_rows_args(self.text, self.b[s:t], self.en[s:t], self.chrom[s:t], self.flags[s:t], t - s)
        status = np.empty(t - s, np.int32)
        return self.lib.ds_freq_parse(self.h, addr, t - s, b.ctypes.data, en.ctypes.data, chrom.ctypes.data, flags.ctypes.data, status.ctypes.data)

    def accumulate(self, rows=()):
        m = len(rows)
        return self.e.freq_accumulate(rows, [0] * m, [0] * m, [0.0] * m, [0.0] * m, [0] * m)

    def raw_accumulate(self) -> int:
        i32, i64, f64 = np.zeros(1, np.int32), np.zeros(1, np.int64), np.zeros(1, np.float64)
        return self.lib.ds_freq_accumulate(self.h, 0, i32.ctypes.data, i32.ctypes.data, i64.ctypes.data, f64.ctypes.data, f64.ctypes.data,
                                           i32.ctypes.data)

    def check(self, got) -> None:
        ref = eng.freq_reference(self.text, self.b, self.en, self.chrom, self.flags, 0.0)
        assert got["rows"] == TOTAL and got["used"] == ref["used"] == TOTAL and len(got["pos"]) == 2
        assert self.ordered(got) == self.ordered(ref)


class CombineRoute(Route):
    name = "combine"
    site_fields = ("chrom", "pos", "sum0", "sum1", "met", "unmet", "cov", "last_plus")

    def __init__(self, e, tmp_path):
        Route.__init__(self, e)
        self.g = cs._Genome(write_bytes(tmp_path / "g.fa", FASTA))
        self.g.select("")
        self.text = ("\n".join(TABLE) + "\n").encode()
        self.b, self.en, local, self.flags, names = eng.freq_locate(self.text)
        self.chrom = np.array([self.g.rec_id.get(n.decode(), -1) for n in names] + [-1], np.int32)[local]
        assert len(self.b) == TOTAL
        self.chunks = 0                      # genome chunks given to the device so far
        self.bitmap = None

    def begin(self, total=TOTAL, batch=BATCH):
        self.e.combine_begin(eng.COMBINE_TABLE, self.g.rec_len, total, batch)
        for sb, se, sbit, scarry in self.g.chunks(16):
            self.e.combine_genome(self.g.data, sb, se, sbit, scarry)
            self.chunks += 1
        self.bitmap = self.e.combine_bitmap()

    def raw_begin(self, total, batch) -> int:
        rec_len = np.ascontiguousarray(self.g.rec_len, np.int64)
        return self.lib.ds_combine_begin(self.h, eng.COMBINE_TABLE, rec_len.size, rec_len.ctypes.data, total, batch)

    def parse(self, s, t):
        return self.e.combine_parse(self.text, self.b[s:t], self.en[s:t], self.chrom[s:t], self.flags[s:t])

    def raw_parse(self, s, t) -> int:
        keep, addr, b, en, chrom, flags = eng._batch_rows_args(self.text, self.b[s:t], self.en[s:t], self.chrom[s:t], self.flags[s:t], t - s)
        status = np.empty(t - s, np.int32)
        return self.lib.ds_combine_parse(self.h, addr, t - s, b.ctypes.data, en.ctypes.data, chrom.ctypes.data, flags.ctypes.data,
                                         status.ctypes.data)

    def accumulate(self, rows=()):
        return self.e.combine_accumulate(rows, [None] * len(rows))

    def raw_accumulate(self) -> int:
        i32, i64, f64 = np.zeros(1, np.int32), np.zeros(1, np.int64), np.zeros(1, np.float64)
        return self.lib.ds_combine_accumulate(self.h, 0, i32.ctypes.data, i32.ctypes.data, i32.ctypes.data, i64.ctypes.data, i32.ctypes.data,
                                              f64.ctypes.data, f64.ctypes.data, i64.ctypes.data, i64.ctypes.data, i64.ctypes.data)

    def check(self, got) -> None:
        ref = eng.combine_reference(eng.COMBINE_TABLE, self.text, self.b, self.en, self.chrom, self.flags, self.g.rec_len, self.bitmap)
        assert ref["status"].tolist() == [OK] * TOTAL
        assert got["rows"] == TOTAL and got["pos"].tolist() == [2] and got["cov"].tolist() == [12]
        assert self.ordered(got) == self.ordered(ref)


class EvalRoute(Route):
    name = "eval"

    def __init__(self, e, tmp_path=None):
        Route.__init__(self, e)
        self.text = ("\n".join(CALLS) + "\n").encode()
        self.b, self.en, self.flags, ff = eng.eval_locate(self.text)
        assert len(self.b) == TOTAL and ff == 0
        self.at, self.n = 0, BATCH           # the rows [at, at + n) are the batch parsed last

    def begin(self, total=TOTAL, batch=BATCH):
        self.e.eval_begin(total, batch, CF)

    def raw_begin(self, total, batch) -> int:
        return self.lib.ds_eval_begin(self.h, total, batch, CF.size, CF.ctypes.data)

    def parse(self, s, t):
        status = self.e.eval_parse(self.text, self.b[s:t], self.en[s:t], self.flags[s:t])
        self.at, self.n = s, t - s
        return status

    def raw_parse(self, s, t) -> int:
        keep, addr, b, en, _, flags = eng._batch_rows_args(self.text, self.b[s:t], self.en[s:t], np.zeros(t - s, np.int32), self.flags[s:t], t - s)
        status = np.empty(t - s, np.int32)
        return self.lib.ds_eval_parse(self.h, addr, t - s, b.ctypes.data, en.ctypes.data, flags.ctypes.data, status.ctypes.data)

    def accumulate(self, rows=()):
        m = len(rows)
        return self.e.eval_accumulate(MASK[self.at:self.at + self.n], rows, [0.0] * m, [0.0] * m, [0] * m)

    def raw_accumulate(self) -> int:
        mask = np.ascontiguousarray(MASK[:BATCH])
        i32, f64 = np.zeros(1, np.int32), np.zeros(1, np.float64)
        return self.lib.ds_eval_accumulate(self.h, mask.ctypes.data, 0, i32.ctypes.data, f64.ctypes.data, f64.ctypes.data, i32.ctypes.data)

    def check(self, got) -> None:
        ref = eng.eval_reference(self.text, self.b, self.en, self.flags, MASK, CF)
        assert ref["status"].tolist() == [OK] * TOTAL
        assert got["rows"] == TOTAL and got["counts"].tobytes() == ref["counts"].tobytes() and int(got["counts"][1][:4].sum()) == TOTAL
        assert (got["u2"], got["p"], got["n"]) == (ref["u2"], ref["p"], ref["n"])


ROUTES = {"freq": FreqRoute, "combine": CombineRoute, "eval": EvalRoute}


@pytest.fixture(scope="module")
def engine():
    e = eng.Engine(device=0, max_batch=64, slots=1)
    yield e
    e.close()


@pytest.fixture(params=sorted(ROUTES))
def route(request, engine, tmp_path):
    r = ROUTES[request.param](engine, tmp_path)
    yield r
    r.end()              # a failed test leaves no run behind for the next


def test_calls_without_a_run(route):
    n = route.name
    no_run = "ds_%s_%%s: no run is open (ds_%s_begin first)" % (n, n)
    route.refused(route.raw_parse(0, 2), no_run % "parse")
    route.refused(route.raw_accumulate(), no_run % "accumulate")
    route.raises(route.result, no_run % "result")
    assert route.raw_end() == DS_OK
    route.begin()
    assert route.raw_end() == DS_OK and route.raw_end() == DS_OK
    route.end()          # and through Engine
    route.refused(route.raw_parse(0, 2), no_run % "parse")
    route.begin()
    route.rest_and_check(0)


def test_a_second_begin_is_refused_and_the_first_run_goes_on(route):
    n = route.name
    route.begin()
    assert route.parse(0, 2).tolist() == [OK, OK]
    open_text = "ds_%s_begin: a run is open on this handle (ds_%s_end first)" % (n, n)
    route.raises(route.begin, open_text)
    route.refused(route.raw_begin(TOTAL, BATCH), open_text)
    route.refused(route.raw_begin(TOTAL, 0), open_text)
    route.accumulate()           # the batch parsed before the refusals
    route.rest_and_check(2)


def test_a_bad_begin_leaves_no_run(route):
    n = route.name
    route.refused(route.raw_begin(TOTAL, 0), "ds_%s_begin: batch_rows must be in [1, 2^24]" % n)
    route.refused(route.raw_accumulate(), "ds_%s_accumulate: no run is open (ds_%s_begin first)" % (n, n))
    route.begin()
    route.rest_and_check(0)


def test_batches_go_strictly_in_sequence(route):
    n = route.name
    route.begin()
    no_batch = "ds_%s_accumulate: no parsed batch (ds_%s_parse first)" % (n, n)
    route.refused(route.raw_accumulate(), no_batch)              # before the first batch
    route.refused(route.raw_parse(0, 3), "ds_%s_parse: nrows must be in [1, batch_rows]" % n)
    route.refused(route.raw_accumulate(), no_batch)              # the refused batch is no batch
    assert route.parse(0, 2).tolist() == [OK, OK]
    previous = "ds_%s_parse: the previous batch has not been accumulated" % n
    route.raises(lambda: route.parse(2, 3), previous)
    route.refused(route.raw_parse(0, 3), previous)
    route.raises(route.result, "ds_%s_result: a parsed batch has not been accumulated" % n)
    route.accumulate()
    route.refused(route.raw_accumulate(), no_batch)              # accumulate twice
    assert route.result()["rows"] == 2                           # between batches the result may be read
    route.raises(lambda: route.parse(0, 2), "ds_%s_parse: more rows than ds_%s_begin was told of" % (n, n))
    route.refused(route.raw_accumulate(), no_batch)
    route.rest_and_check(2)
    route.refused(route.raw_accumulate(), "ds_%s_accumulate: no run is open (ds_%s_begin first)" % (n, n))


def test_the_python_layers_own_refusals(route):
    n = route.name
    low = 0 if n == "combine" else 1
    with pytest.raises(ValueError, match=r"total_rows must be in \[%d, 2\^30\]" % low):
        route.begin(low - 1, BATCH)
    with pytest.raises(ValueError, match=r"total_rows must be in \[%d, 2\^30\]" % low):
        route.begin((1 << 30) + 1, BATCH)
    for bad in (0, (1 << 24) + 1):
        with pytest.raises(ValueError, match=r"batch_rows must be in \[1, 2\^24\]"):
            route.begin(TOTAL, bad)
    needs = "%s_accumulate needs a batch from %s_parse" % (n, n)
    route.begin()
    with pytest.raises(ValueError, match=needs):
        route.accumulate()
    with pytest.raises(ValueError, match=r"a batch holds 1 \.\. batch_rows rows of an open run"):
        route.parse(0, 3)
    with pytest.raises(ValueError, match=needs):
        route.accumulate()
    assert route.parse(0, 2).tolist() == [OK, OK]
    for rows in ([1, 0], [0, 0], [2], [-1]):
        with pytest.raises(ValueError, match="override rows must be ascending indices of the batch"):
            route.accumulate(rows)
    route.accumulate()
    with pytest.raises(ValueError, match=needs):
        route.accumulate()
    route.rest_and_check(2)
    with pytest.raises(ValueError, match=needs):
        route.accumulate()
    with pytest.raises(ValueError, match=r"a batch holds 1 \.\. batch_rows rows of an open run"):
        route.parse(0, 2)


def test_streaming_and_counted_runs_keep_apart(engine):
    r = FreqRoute(engine)
    chrom, pos = np.zeros(2, np.int32), np.array([10, 20], np.int64)
    act, pred = np.array([[0.25, 0.75], [0.75, 0.25]], np.float32), np.array([1, 0], np.int32)
    try:
        status, opened = np.empty(2, np.int32), np.zeros(2, np.int32)
        rc = engine._lib.ds_freq_push(engine._h, 2, chrom.ctypes.data, pos.ctypes.data, act.ctypes.data, 2, pred.ctypes.data,
                                      status.ctypes.data, opened.ctypes.data)
        r.refused(rc, "ds_freq_push: no run is open (ds_freq_begin_stream first)")
        r.begin()
        r.raises(lambda: engine.freq_push(chrom, pos, act, pred), "ds_freq_push: no streaming run is open (ds_freq_begin_stream first)")
        r.raises(lambda: engine.freq_begin_stream(1, BATCH), "ds_freq_begin_stream: a run is open on this handle (ds_freq_end first)")
        r.rest_and_check(0)
        engine.freq_begin_stream(1, BATCH)
        r.raises(lambda: r.parse(0, 2), "ds_freq_parse: the open run is a streaming one (ds_freq_push)")
        r.raises(r.begin, "ds_freq_begin: a run is open on this handle (ds_freq_end first)")
        assert engine.freq_push(chrom, pos, act, pred).tolist() == [OK, OK]
        r.raises(lambda: engine.freq_push(chrom, pos, act, pred), "ds_freq_push: the previous batch has not been accumulated")
        r.raises(lambda: r.parse(0, 2), "ds_freq_parse: the open run is a streaming one (ds_freq_push)")
        assert engine.freq_accumulate().tolist() == [1, 1]
        got = engine.freq_result()
        assert got["rows"] == 2 and got["used"] == 2 and sorted(got["pos"].tolist()) == [10, 20]
    finally:
        engine.freq_end()


def test_a_freq_run_and_an_eval_run_on_one_handle(engine):
    f, v = FreqRoute(engine), EvalRoute(engine)
    try:
        f.begin()
        v.begin()
        assert f.parse(0, 2).tolist() == [OK, OK]
        assert v.parse(0, 2).tolist() == [OK, OK]
        v.accumulate()
        f.raises(f.result, "ds_freq_result: a parsed batch has not been accumulated")
        assert v.result()["rows"] == 2
        f.accumulate()
        assert v.parse(2, 3).tolist() == [OK]
        f.rest_and_check(2)              # ends the freq run; the eval run has a batch pending
        v.raises(v.result, "ds_eval_result: a parsed batch has not been accumulated")
        v.accumulate()
        got = v.result()
        v.end()
        v.check(got)
    finally:
        f.end()
        v.end()


def assert_times(t: dict, batches: int, **counters) -> None:
    assert t["batches"] == batches and all(t[k] == v for k, v in counters.items())
    ms = [v for k, v in t.items() if k.endswith("_ms")]
    assert ms and all(math.isfinite(v) and v >= 0 for v in ms)


def test_times_count_ended_runs_and_the_open_one(route):
    route.times(reset=True)
    chunks = lambda: {"chunks": route.chunks} if route.name == "combine" else {}
    route.chunks = 0
    route.begin()
    route.rest_and_check(0)              # two batches, ended
    assert_times(route.times(), 2, **chunks())
    route.begin()
    assert route.parse(0, 2).tolist() == [OK, OK]
    route.accumulate()                   # one batch, the run stays open
    t = route.times()
    assert_times(t, 3, **chunks())
    assert route.name != "combine" or route.chunks >= 2
    assert route.times(reset=True) == t
    zeros = route.times()
    assert zeros["batches"] == 0 and zeros.get("chunks", 0) == 0 and all(v == 0 for k, v in zeros.items() if k.endswith("_ms"))
    route.chunks = 0
    route.rest_and_check(2)              # one more batch
    assert_times(route.times(), 1, **chunks())
    assert_times(route.times(reset=True), 1, **chunks())
    assert route.times()["batches"] == 0


def growths_of(slots: int, sites: int, nrows: int):
    """ds_freq.h: the table doubles until 2 * (sites + rows of the batch) <= slots -> (doublings, slots)."""
    n = 0
    while 2 * (sites + nrows) > slots:
        slots, n = 2 * slots, n + 1
    return n, slots


def test_stream_times_count_ended_runs_and_the_open_one(engine):
    chrom, pos = np.zeros(2, np.int32), np.array([10, 20], np.int64)
    act, pred = np.array([[0.25, 0.75], [0.75, 0.25]], np.float32), np.array([1, 0], np.int32)

    def push(s, t):
        assert engine.freq_push(chrom[s:t], pos[s:t] + 5 * s, act[s:t], pred[s:t]).tolist() == [OK] * (t - s)
        engine.freq_accumulate()

    first, slots = growths_of(1, 0, 2)               # a batch of two new sites into a table of one slot
    second, _ = growths_of(slots, 2, 1)              # then one row, a third site
    assert (first, second) == (2, 1)
    try:
        engine.freq_stream_times(reset=True)
        engine.freq_times(reset=True)
        engine.freq_begin_stream(1, BATCH)
        push(0, 2)
        push(1, 2)
        assert engine.freq_result()["rows"] == 3 and len(engine.freq_result()["pos"]) == 3
        engine.freq_end()
        assert engine.freq_stream_times()["growths"] == first + second
        engine.freq_begin_stream(1, BATCH)
        push(0, 2)
        t = engine.freq_stream_times()
        assert t["growths"] == 2 * first + second and all(math.isfinite(t[k]) and t[k] >= 0 for k in ("values_ms", "rehash_ms"))
        assert engine.freq_times()["batches"] == 3
        assert engine.freq_stream_times(reset=True) == t
        assert engine.freq_stream_times() == {"values_ms": 0.0, "rehash_ms": 0.0, "growths": 0}
        push(1, 2)
        assert engine.freq_stream_times()["growths"] == second and engine.freq_times(reset=True)["batches"] == 4
        engine.freq_end()
        assert engine.freq_stream_times(reset=True)["growths"] == second
        assert engine.freq_stream_times()["growths"] == 0
    finally:
        engine.freq_end()


@pytest.mark.parametrize("name", sorted(ROUTES))
def test_close_with_a_run_open_and_a_batch_pending(name, tmp_path):
    e = eng.Engine(device=0, max_batch=64, slots=1)
    try:
        r = ROUTES[name](e, tmp_path)
        r.begin()
        assert r.parse(0, 2).tolist() == [OK, OK]
    finally:
        e.close()
    e.close()            # and twice
