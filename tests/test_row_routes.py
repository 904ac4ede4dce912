"""CPU: every route of call_modifications._RowPipeline -- parsed arrays (submit / submit_parts), row spans (submit_text), fast5 reads
(submit_reads) -- on the stand-in engine of tests/test_harness.py: batches filled across items, tickets bounded by the slots and
waited in order, rows in feed order, the frequency tap seeing what the writer sees, and errors surfacing on the feeding thread."""
import os
import threading
import types

import numpy as np
import pytest

from deepsignal_amd import call_modifications as cm, extract_features as ef, fastio
from deepsignal_amd.utils.process_utils import code2base_dna

from test_harness import _AsyncStandIn, _items_for_pipeline

HERE = os.path.dirname(os.path.abspath(__file__))
pytestmark = pytest.mark.skipif(not os.path.exists(os.path.join(os.path.dirname(HERE), "deepsignal_amd", "libdeepsignal_hip.so")),
                                reason="native library not built (row formatter, CPU checkers)")
N, CUTS = 333, [0, 5, 70, 71, 200, 333]
ROUTES = ("arrays", "text", "reads")


class Feeds:
    """What each route is fed with, built once: the items of _items_for_pipeline(N, CUTS) written as a feature file (item k = read
    k, so the reader cuts the same items again) and read back parsed (arrays) and located (text), and the reads of
    tests/golden/fast5/plain as device-route records."""

    def __init__(self, tmp):
        feats, items = _items_for_pipeline(N, CUTS)
        self.path = os.path.join(tmp, "features.tsv")
        with open(self.path, "w") as f:
            for k, (s0, e0) in enumerate(zip(CUTS[:-1], CUTS[1:])):
                for i in range(s0, e0):
                    f.write("\t".join(["chr1", str(1000 + i), "+", str(i), "read_%d" % k, "t", "".join(code2base_dna[int(c)] for c in feats["kmer"][i])]
                                      + [",".join("%.6f" % x for x in feats[c][i]) for c in ("means", "stds")]
                                      + [",".join(str(int(x)) for x in feats["sanums"][i]), ",".join("%.6f" % x for x in feats["signals"][i]), "1"]) + "\n")
        self.text = open(self.path, "rb").read()
        rd = fastio.FeatureReader(self.path)
        self.arrays = list(rd.items(1))
        rd.close()
        rd = fastio.FeatureReader(self.path)
        self.spans = list(rd.spans(1))
        rd.close()
        assert [len(it.labels) for it in self.arrays] == [len(it.begin) for it in self.spans] == list(np.diff(CUTS))
        self.task = (ef.get_fast5s(os.path.join(HERE, "golden", "fast5", "plain")), "RawGenomeCorrected_000", "BaseCalled_template", "mad",
                     ["CG"], 0, None, 17, 360, 1, None)
        self.records = cm._fast5_reads_task(self.task)[0]

    def pipe(self, route, eng, sink, rows_sink=None):
        """(pipeline, the items to feed it) of one route; `sink` as _RowPipeline takes it."""
        if route == "arrays":
            return cm._RowPipeline(eng, 64, sink, rows_sink), self.arrays
        if route == "text":
            return cm._TextPipeline(eng, 64, sink, types.SimpleNamespace(data=self.text), rows_sink), self.spans
        pipe = cm._ReadsPipeline(eng, "mad", rows_sink, text=sink is not None)
        pipe.sink = sink
        return pipe, self.records

    def run(self, route, eng, sink, rows_sink=None):
        pipe, items = self.pipe(route, eng, sink, rows_sink)
        try:
            for tag, it in enumerate(items):
                pipe.feed(it, tag)
            pipe.flush()
        finally:
            pipe.close()
        return pipe


@pytest.fixture(scope="module")
def feeds(tmp_path_factory):
    return Feeds(str(tmp_path_factory.mktemp("row_routes")))


def _engine(route, **kw):
    return _AsyncStandIn(max_batch=7 if route == "reads" else 64, **kw)      # 7: reads straddle batches, more tickets than slots


def test_text_route_fills_batches_across_items_and_writes_the_array_routes_bytes(feeds):
    eng, got = _AsyncStandIn(), []
    pipe, items = feeds.pipe("text", eng, lambda tag, data: got.append((tag, data)))
    assert pipe.pipelined
    for tag, it in enumerate(items):
        pipe.feed(it, tag)
        assert pipe.live_tags() <= set(range(tag + 1))
    pipe.flush()
    assert not pipe.live_tags() and not eng.pending
    pipe.close()
    assert eng.batches == [64] * 5 + [13] and pipe.nsites == N       # (the stand-in asserts: waited in order, <= slots in flight)
    assert [t for t, _ in got] == sorted(t for t, _ in got)
    ref = []
    feeds.run("arrays", _AsyncStandIn(), lambda tag, data: ref.append(data))
    assert b"".join(d for _, d in got) == b"".join(ref) and b"".join(ref).count(b"\n") == N
    with pytest.raises(ValueError, match="parse_on='gpu' needs batch_size <= engine.max_batch"):
        cm._TextPipeline(eng, 65, None, None)


def _host_items(task):
    """The host-extracted features of the task's reads as array-route items, one per read, and the (chrom, pos, strand, read) of
    the sites whose middle base alone has >= 360 samples (the device route draws another subsample there)."""
    items, sub = [], set()
    for fp in task[0]:
        (info, kmer, means, stds, lens, signals, labels), = cm._read_features_from_fast5s([fp], *task[1:])[0]
        blob = [s.encode() for s in info]
        off = np.zeros(len(blob) + 1, np.int64)
        off[1:] = np.cumsum([len(b) for b in blob])
        items.append(fastio.FeatureItem(np.frombuffer(b"".join(blob), np.uint8), off, np.asarray(kmer, np.int32), np.asarray(means, np.float32),
                                        np.asarray(stds, np.float32), np.asarray(lens, np.float32), np.asarray(signals, np.float32),
                                        np.asarray(labels, np.int32)))
        sub.update((s.split("\t")[0], s.split("\t")[1], s.split("\t")[2], s.split("\t")[4]) for s, l in zip(info, lens) if l[8] >= 360)
    return items, sub


def _same_rows(got, want, sub):
    got, want = got.decode().splitlines(), want.decode().splitlines()
    assert len(got) == len(want) > 0
    for g, w in zip(got, want):
        cg, cw = g.split("\t"), w.split("\t")
        if (cw[0], cw[1], cw[2], cw[4]) in sub:
            assert cg[:6] == cw[:6] and cg[9] == cw[9]
        else:
            assert g == w


def _array_route_bytes(items, max_batch):
    ref = []
    pipe = cm._RowPipeline(_AsyncStandIn(max_batch=max_batch), 1, lambda tag, data: ref.append(data))
    for it in items:
        pipe.feed(it)
    pipe.flush()
    pipe.close()
    return b"".join(ref)


@pytest.mark.parametrize("style,norm,cap", [("plain", "mad", 7), ("ont", "zscore", 64), ("latest", "mad", 4096)])
def test_reads_route_writes_the_array_routes_rows_of_the_host_features(style, norm, cap):
    task = (ef.get_fast5s(os.path.join(HERE, "golden", "fast5", style)), "RawGenomeCorrected_000", "BaseCalled_template", norm, ["CG"], 0,
            None, 17, 360, 1, None)
    records, failed = cm._fast5_reads_task(task)
    assert failed == 0 and all(r[0] == "gpu" for r in records)
    eng = _AsyncStandIn(max_batch=cap)
    pipe = cm._ReadsPipeline(eng, norm)
    got = b"".join(cm._rows_from_device(records, pipe, 16))
    pipe.close()
    items, sub = _host_items(task)
    _same_rows(got, _array_route_bytes(items, cap), sub)
    nsites = sum(len(it.labels) for it in items)
    assert pipe.nsites == nsites == sum(eng.batches) and not eng.pending
    assert all(n == cap for n in eng.batches[:-1]) and 0 < eng.batches[-1] <= cap
    if cap == 7:
        assert len(eng.batches) > eng.slots and max(len(r[2]) for r in records) > cap      # more tickets than slots; reads straddle


def test_reads_route_keeps_a_host_route_read_between_device_route_reads_in_place(feeds):
    """A "cpu" record (a read the device route cannot take: its payload is the host route's queue items) waits for the rows before
    it; the pipeline is flushed per file batch and lives on for the next one."""
    recs = list(feeds.records)
    assert len(recs) >= 3
    mid = len(recs) // 2
    fp = feeds.task[0][mid]
    recs[mid] = ("cpu", cm._read_features_from_fast5s([fp], *feeds.task[1:]))
    items, sub = _host_items(feeds.task)
    want = _array_route_bytes(items, 7)
    seen = []
    eng = _engine("reads")
    pipe = cm._ReadsPipeline(eng, "mad", lambda *a: seen.append(fastio.format_rows(*a)))
    try:
        for _ in range(2):                                 # two file batches through one pipeline
            got = b"".join(cm._rows_from_device(recs, pipe, 16))
            _same_rows(got, want, sub)
            assert b"".join(seen) == got and not eng.pending and not pipe.inflight
            del seen[:]
    finally:
        pipe.close()
    assert pipe.nsites == 2 * want.count(b"\n") and len(items[mid].labels) > 0
    ragged = lambda n: [7] * (n // 7) + [n % 7] * (n % 7 > 0)
    before, after = (sum(len(r[2]) for r in part) for part in (recs[:mid], recs[mid + 1:]))
    assert eng.batches == 2 * (ragged(before) + ragged(after))        # one ragged batch per flush: at the host-route read, at the end


@pytest.mark.parametrize("route", ROUTES)
def test_rows_sink_sees_what_the_writer_sees(feeds, route):
    wrote, seen, alone = [], [], []
    feeds.run(route, _engine(route), lambda tag, data: wrote.append(data), lambda *a: seen.append(fastio.format_rows(*a)))
    assert b"".join(seen) == b"".join(wrote) and b"".join(wrote).count(b"\n") > 0
    pipe = feeds.run(route, _engine(route), None, lambda *a: alone.append(fastio.format_rows(*a)))
    assert b"".join(alone) == b"".join(wrote)
    if route == "reads":
        assert pipe.chunks == []                           # sink=None: no row text is made


def _helper_threads():
    return {t for t in threading.enumerate() if t is not threading.main_thread()}


@pytest.mark.parametrize("route", ROUTES)
def test_a_failing_sink_surfaces_on_the_feeding_thread(feeds, route):
    def sink(tag, data):
        raise IOError("disk full")
    before = _helper_threads()
    with pytest.raises(IOError, match="disk full"):
        feeds.run(route, _engine(route), sink)
    assert _helper_threads() <= before


@pytest.mark.parametrize("route", ROUTES)
def test_a_failing_wait_surfaces_and_close_leaves_nothing_behind(feeds, route):
    eng = _engine(route, fail_wait=3)
    before = _helper_threads()
    with pytest.raises(RuntimeError, match="wait 3 failed"):
        feeds.run(route, eng, lambda tag, data: None)
    assert eng.waits >= 3 and not eng.pending              # close() waited what was still in flight
    assert _helper_threads() <= before


def test_text_route_names_the_malformed_row_as_the_host_route_does(tmp_path):
    """A ticket that straddles two items, the malformed row in the second: TextRowError.row counts within the ticket, the message
    names the row as the reader counts it (the host route's message, ds_tsv_parse_into)."""
    import text_cases as tc
    rows = tc.make_rows(30, 17, 360, seed=5, sites_per_read=3)
    rows[13] = rows[13].replace(b",", b";", 1)
    path = str(tmp_path / "bad.tsv")
    with open(path, "wb") as f:
        f.write(b"\n".join(rows) + b"\n")
    rd = fastio.FeatureReader(path)
    with pytest.raises(ValueError) as host:
        list(rd.items(2))
    rd.close()
    rd = fastio.FeatureReader(path)
    spans = list(rd.spans(2))                              # items of 6 rows; tickets of 8: the second holds rows 8 .. 15 of items 1 and 2
    rd.close()
    eng = _AsyncStandIn(max_batch=8)
    pipe = cm._TextPipeline(eng, 8, lambda tag, data: None, types.SimpleNamespace(data=open(path, "rb").read()))
    with pytest.raises(ValueError) as text:
        for it in spans:
            pipe.feed(it)
        pipe.flush()
    pipe.close()
    off = sum(len(r) + 1 for r in rows[:13])
    assert str(text.value) == str(host.value) == "feature file: row 14 (line at byte offset %d): malformed feature row" % off
    assert type(text.value) is ValueError and eng.batches[:2] == [8, 8] and not eng.pending
