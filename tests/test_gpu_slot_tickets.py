"""GPU: the lifecycle of a pipeline slot's ticket, whatever route put it there (ds_submit* / ds_wait*, and the blocking diagnostics
that borrow the next slot). One small engine per test -- max_batch 8, two slots: the smallest shapes at which n < max_batch,
n == max_batch and the wrap-around of the slots all occur. Every result is compared with the blocking call for the same input:
floats as uint32, text byte for byte."""
import ctypes

import numpy as np
import pytest

from deepsignal_amd import synth, weights
from deepsignal_amd.engine import Engine, ReadBatch, base_codes, extract_rows_reference, format_values, pack_info

import text_cases as tc

pytestmark = pytest.mark.gpu

K, S, B, SLOTS = 17, 360, 8, 2
FEATURES = ("kmer", "means", "stds", "sanums", "signals")


@pytest.fixture(scope="module")
def w3():
    return weights.random_weights(seed=3, lstm_bias_std=0.1)


@pytest.fixture
def eng(w3):
    e = Engine(device=0, max_batch=B, slots=SLOTS)
    e.load_weights(w3)
    assert e.slots == SLOTS
    yield e
    e.close()


def _reads(i, nsites):
    """(ReadBatch of `nsites` CG sites of one seeded read, info, info_off, label): the arguments of submit_rows / extract_rows"""
    raw, starts, lengths, bases, scaling, offset = synth.synthetic_read(300 + 70 * i, 40 + i, long_bases=i % 2)
    codes = base_codes(bases)
    locs = [loc for loc in range(8, len(codes) - 8) if codes[loc] == 1 and codes[loc + 1] == 2][:nsites]
    assert len(locs) == nsites
    rows = [("chrX\t%d\t-\t%d\tread%d\tt" % (loc, 5 * loc, i)).encode() for loc in locs]
    return (ReadBatch([(raw, starts, lengths, codes, scaling, offset, 500 + i)], [0] * nsites, locs, norm=("mad", "zscore")[i % 2],
                      seed=3),) + pack_info(rows) + (i % 2,)


def _text(n, seed):
    return tc.pack(tc.make_rows(n, K, S, seed=seed))


def _same_forward(got, want):
    return np.array_equal(tc.bits(got[0]), tc.bits(want[0])) and np.array_equal(got[1], want[1])


def _same_text(got, want):
    """wait_text's six results"""
    return _same_forward(got, want) and all(np.array_equal(g, w) for g, w in zip(got[2:], want[2:]))


def _same_rows(got, want):
    return got[0] == want[0] and np.array_equal(got[1], want[1])


def _run_reads(e, batch):
    """The blocking counterpart of wait(submit_reads(batch)): the extracted features through run()"""
    f = e.extract(batch)
    return e.run(*(f[k] for k in FEATURES))


def _as_text_ticket(t):
    return (t[0], t[1], 64, None)


def test_a_wait_of_the_wrong_kind_is_refused_and_the_ticket_stays(eng):
    """(a) forward, text and rows tickets: the two other waits raise with their own name, the right one then returns the blocking
    call's results."""
    reads = _reads(0, 5)
    blob, begin, end = _text(6, seed=21)
    want_fwd = _run_reads(eng, reads[0])
    want_text = eng.wait_text(eng.submit_text(blob, begin, end))
    want_rows = eng.extract_rows(*reads)

    t = eng.submit_reads(reads[0])
    with pytest.raises(RuntimeError, match="ds_wait_text: "):
        eng.wait_text(_as_text_ticket(t))
    with pytest.raises(RuntimeError, match="ds_wait_rows: "):
        eng.wait_rows(t)
    assert _same_forward(eng.wait(t), want_fwd)

    t = eng.submit_text(blob, begin, end)
    with pytest.raises(RuntimeError, match="ds_wait: "):
        eng.wait(t[:2])
    with pytest.raises(RuntimeError, match="ds_wait_rows: "):
        eng.wait_rows(t[:2])
    assert _same_text(eng.wait_text(t), want_text)

    t = eng.submit_rows(*reads)
    with pytest.raises(RuntimeError, match="ds_wait: "):
        eng.wait(t)
    with pytest.raises(RuntimeError, match="ds_wait_text: "):
        eng.wait_text(_as_text_ticket(t))
    assert _same_rows(eng.wait_rows(t), want_rows)

    for wait, ticket, name in ((eng.wait, t, "ds_wait: "), (eng.wait_text, _as_text_ticket(t), "ds_wait_text: "),
                               (eng.wait_rows, t, "ds_wait_rows: ")):      # collected: nothing is in flight any more
        with pytest.raises(RuntimeError, match=name):
            wait(ticket)


def test_every_entry_point_refuses_a_full_pipeline(eng):
    """(b) both slots in flight: every call that needs a slot raises with its own name; with the oldest ticket waited, the ones
    that borrow the idle slot work, and the ticket still in flight is collected with the blocking call's bytes."""
    reads0, reads1 = _reads(0, 5), _reads(1, 8)
    blob, begin, end = _text(4, seed=22)
    f = eng.extract(reads0[0])
    arrays = [f[k] for k in FEATURES]
    want_fwd = eng.run(*arrays)
    want_rows1 = eng.extract_rows(*reads1)
    want_rows0 = eng.extract_rows(*reads0)
    want_text = eng.wait_text(eng.submit_text(blob, begin, end))
    want_parse = eng.parse_text(blob, begin, end)
    act = np.asarray([[0.5, 0.5], [0.9, 0.1], [0.45, 0.55]], np.float32)
    want_sel = eng.recheck_select(act, 0.2)
    values = [1.5, -2.25, 1e-5]

    borrowers = {
        "ds_extract": lambda: eng.extract(reads0[0]),
        "ds_parse_text": lambda: eng.parse_text(blob, begin, end),
        "ds_extract_rows": lambda: eng.extract_rows(*reads0),
        "ds_recheck_select": lambda: eng.recheck_select(act, 0.2),
        "ds_format_values": lambda: format_values(values, engine=eng),
    }
    submits = {
        "ds_submit": lambda: eng.submit(*arrays),
        "ds_submit_parts": lambda: eng.submit_parts([tuple(a[:2] for a in arrays), tuple(a[2:] for a in arrays)]),
        "ds_submit_reads": lambda: eng.submit_reads(reads0[0]),
        "ds_submit_text": lambda: eng.submit_text(blob, begin, end),
        "ds_submit_rows": lambda: eng.submit_rows(*reads0),
    }
    whole_handle = {"ds_forward": lambda: eng.run(*arrays), "ds_set_recheck": lambda: eng.set_recheck(None, 0.0)}

    t_fwd = eng.submit_reads(reads0[0])
    t_rows = eng.submit_rows(*reads1)
    for name, call in list(submits.items()) + list(borrowers.items()) + list(whole_handle.items()):
        with pytest.raises(RuntimeError, match=name + r".*in flight"):
            call()
    assert _same_forward(eng.wait(t_fwd), want_fwd)

    got = {name: call() for name, call in borrowers.items()}
    for k in FEATURES:
        assert np.array_equal(tc.bits(got["ds_extract"][k]), tc.bits(f[k])), k
    for k in want_parse:
        assert np.array_equal(tc.bits(got["ds_parse_text"][k]), tc.bits(want_parse[k])), k
    assert _same_rows(got["ds_extract_rows"], want_rows0)
    assert np.array_equal(got["ds_recheck_select"], want_sel)
    assert got["ds_format_values"] == format_values(values)
    for name, call in whole_handle.items():          # a rows ticket is still in flight
        with pytest.raises(RuntimeError, match=name + r".*in flight"):
            call()

    t = submits["ds_submit"]()
    with pytest.raises(RuntimeError, match=r"ds_submit_parts.*in flight"):
        submits["ds_submit_parts"]()
    assert _same_rows(eng.wait_rows(t_rows), want_rows1)
    assert _same_forward(eng.wait(t), want_fwd)
    assert _same_forward(eng.wait(submits["ds_submit_parts"]()), want_fwd)
    assert _same_forward(eng.wait(submits["ds_submit_reads"]()), want_fwd)
    assert _same_text(eng.wait_text(submits["ds_submit_text"]()), want_text)
    assert _same_rows(eng.wait_rows(submits["ds_submit_rows"]()), want_rows0)
    assert _same_forward(eng.run(*arrays), want_fwd)


def test_a_refused_batch_consumes_no_slot(eng):
    """(c) nsites out of range and a row with end < begin: refused, and the next `slots` submits take the slots in order."""
    reads = _reads(0, 5)
    big = _reads(1, B + 1)
    blob, begin, end = _text(3, seed=23)
    want_fwd = _run_reads(eng, reads[0])
    want_rows = eng.extract_rows(*reads)
    t = eng.submit_reads(reads[0])
    assert _same_forward(eng.wait(t), want_fwd)
    next_slot = (t[0] + 1) % SLOTS

    with pytest.raises(RuntimeError, match="nsites"):
        eng.submit_reads(big[0])
    with pytest.raises(RuntimeError, match="nsites"):
        eng.submit_rows(*big)
    bad_end = end.copy()
    bad_end[1] = begin[1] - 1
    text = np.frombuffer(blob, np.uint8)
    ticket = ctypes.c_int32(-1)
    rc = eng._lib.ds_submit_text(eng._h, text.ctypes.data, 3, begin.ctypes.data, bad_end.ctypes.data, ctypes.byref(ticket))
    assert rc < 0 and "bad span" in eng._lib.ds_last_error(eng._h).decode() and ticket.value == -1

    t0 = eng.submit_reads(reads[0])
    t1 = eng.submit_rows(*reads)
    assert (t0[0], t1[0]) == (next_slot, (next_slot + 1) % SLOTS)
    assert _same_forward(eng.wait(t0), want_fwd)
    assert _same_rows(eng.wait_rows(t1), want_rows)


def test_mixed_tickets_wrap_over_the_slots(eng):
    """(d) forward, rows, text, forward, rows over two slots, two in flight, each waited before its slot is taken again."""
    reads = [_reads(i, n) for i, n in enumerate((5, 8, 3))]
    blob, begin, end = _text(B, seed=24)
    want_text = eng.wait_text(eng.submit_text(blob, begin, end))
    order = [("fwd", reads[0]), ("rows", reads[1]), ("text", None), ("fwd", reads[2]), ("rows", reads[0])]
    want = [_run_reads(eng, r[0]) if kind == "fwd" else eng.extract_rows(*r) if kind == "rows" else want_text for kind, r in order]
    submit = {"fwd": lambda r: eng.submit_reads(r[0]), "rows": lambda r: eng.submit_rows(*r),
              "text": lambda r: eng.submit_text(blob, begin, end)}
    wait = {"fwd": eng.wait, "rows": eng.wait_rows, "text": eng.wait_text}
    same = {"fwd": _same_forward, "rows": _same_rows, "text": _same_text}
    tickets, got = [], []
    for kind, r in order:
        if len(tickets) - len(got) == SLOTS:
            got.append(wait[order[len(got)][0]](tickets[len(got)]))
        tickets.append(submit[kind](r))
    while len(got) < len(order):
        got.append(wait[order[len(got)][0]](tickets[len(got)]))
    assert [t[0] for t in tickets] == [(tickets[0][0] + i) % SLOTS for i in range(len(order))]
    for i, (kind, _) in enumerate(order):
        assert same[kind](got[i], want[i]), (i, kind)


@pytest.mark.parametrize("host_rows", [(0, 1, 2, 3, 4, 5, 6, 7), (1, 4, 6)], ids=["m_eq_max_batch", "m_lt_max_batch"])
def test_rows_left_to_the_host_are_forwarded_on_the_slot(eng, tmp_path, host_rows):
    """(e) a text ticket of max_batch rows of which all, or three, are forms the device leaves to the host parser: those rows go
    through the forward once more on the ticket's slot, as a full batch (one copy of the staging block) or as a partial one
    (a copy per array). Everything equals run() on the host parser's arrays."""
    rows = tc.make_rows(B, K, S, seed=25)
    for n, i in enumerate(host_rows):
        c = rows[i].split(b"\t")
        col, j, tok = ((7, n % K, b"+0.5"), (8, 0, b"0.12345678901234567"))[n % 2]
        t = c[col].split(b",")
        t[j] = tok
        c[col] = b",".join(t)
        rows[i] = b"\t".join(c)
    assert [tc.row_in_grammar(r, K, S) for r in rows] == [i not in host_rows for i in range(B)]
    host = tc.host_arrays_of(rows, K, S, tmp_path)
    blob, begin, end = tc.pack(rows)
    want = eng.run(*(host[k] for k in ("kmer", "means", "stds", "lens", "signals")))
    assert np.isfinite(want[0]).all()
    before = eng.text_stats()
    act, pred, kmer, labels, info, off = eng.wait_text(eng.submit_text(blob, begin, end))
    after = eng.text_stats()
    assert after["host_rows"] - before["host_rows"] == len(host_rows) and after["rows"] - before["rows"] == B
    assert _same_forward((act, pred), want)
    assert np.array_equal(kmer, host["kmer"]) and np.array_equal(labels, host["labels"])
    assert np.array_equal(np.diff(off), host["info_len"])
    assert info.tobytes() == b"".join(b"\t".join(r.split(b"\t")[:6]) for r in rows)


def test_profiled_extract_rows_after_a_refused_one(eng):
    """(f) with profiling on, a call refused after its timing events exist (a bad info_off; a short buffer is refused earlier)
    leaves the next call and the timing sums working."""
    reads = _reads(0, 5)
    want = extract_rows_reference(*reads)
    eng.set_profiling(1)
    eng.rows_times(reset=True)
    with pytest.raises(RuntimeError, match="info_off"):
        eng.extract_rows(reads[0], reads[1], reads[2][::-1].copy(), reads[3])
    assert eng.rows_times()["batches"] == 0
    assert _same_rows(eng.extract_rows(*reads), want)
    times = eng.rows_times()
    assert times["batches"] == 1 and all(times[k] >= 0 for k in times)
    eng.set_profiling(0)
    assert _same_rows(eng.wait_rows(eng.submit_rows(*reads)), want)
