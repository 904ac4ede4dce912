"""GPU: feature-TSV rows parsed on the device (`call_mods --parse_on gpu`; ds_submit_text / ds_wait_text / ds_parse_text,
csrc/ds_tsv_parse.hip). tsv_parse_kernel against the CPU checker built from the same token routines (ds_parse_text_reference,
itself held to the host reader and to Python's float() by tests/test_text_parse_reference.py), and the text route through the
pipeline, the recheck and call_mods against the host-parsed route. Every comparison is bit for bit or byte for byte."""
import os

import numpy as np
import pytest

import text_cases as tc

pytestmark = pytest.mark.gpu

K, S = 17, 360
STEP = 1024            # bytes of a row the kernel looks at per step; DS_TEXT_BYTES_PER_ROW = 6144 sizes a slot's text block
BLOCK_PER_ROW = 6144


@pytest.fixture(scope="module", autouse=True)
def _built():
    import __graft_entry__ as g
    g.build()


@pytest.fixture(scope="module")
def eng(small_weights):
    """256-site fp32 engine, three slots."""
    from deepsignal_amd.engine import Engine
    e = Engine(device=0, max_batch=256, slots=3)
    e.load_weights(small_weights)
    yield e
    e.close()


@pytest.fixture(scope="module")
def rows256():
    """256 rows of the default geometry, "%.6f" values with a few exponent forms, and the checker's arrays for them."""
    from deepsignal_amd.engine import parse_text_reference
    rows = tc.make_rows(256, K, S, seed=5)
    for i in range(0, 256, 7):                          # what `extract` prints for small values
        c = rows[i].split(b"\t")
        sig = c[10].split(b",")
        sig[i % S], sig[(3 * i) % S] = b"1e-06", b"-1.2e-05"
        c[10] = b",".join(sig)
        rows[i] = b"\t".join(c)
    blob, begin, end = tc.pack(rows)
    ref = parse_text_reference(blob, begin, end, K, S)
    assert (ref["status"] == tc.OK).all()
    return rows, blob, begin, end, ref


def _check(got, ref, idx=None, what=""):
    """status of every row, values of the rows the device parsed"""
    rs = ref["status"] if idx is None else ref["status"][idx]
    assert np.array_equal(got["status"], rs), what
    ok = np.flatnonzero(rs == tc.OK)
    sub = ref if idx is None else {k: ref[k][idx] for k in tc.ARRAYS + ("info_len",)}
    tc.assert_rows_equal(got, sub, ok, what)
    assert np.array_equal(got["info_len"][ok], sub["info_len"][ok]), what


@pytest.mark.parametrize("n", [1, 63, 64, 65, 256])
def test_row_counts(eng, rows256, n):
    rows, blob, begin, end, ref = rows256
    _check(eng.parse_text(blob, begin[:n], end[:n]), ref, np.arange(n), "n=%d" % n)


def test_short_rows_of_the_9_100_geometry():
    """250 .. 900 bytes: whole rows below one 1 KiB step."""
    from deepsignal_amd.engine import Engine, parse_text_reference
    rows = []
    for fmt, seed in (("%.0f", 1), ("%.2f", 2), ("%.3f", 3)):
        rows += tc.make_rows(40, 9, 100, seed=seed, fmt=fmt)
    assert min(map(len, rows)) < 400 and 700 < max(map(len, rows)) < STEP
    blob, begin, end = tc.pack(rows)
    e = Engine(device=0, max_batch=256, kmer_len=9, signal_len=100)
    try:
        _check(e.parse_text(blob, begin, end), parse_text_reference(blob, begin, end, 9, 100))
    finally:
        e.close()


def _wide_rows(n, seed):
    """28-character values: sign, zeros, 22 fraction digits of which 14 significant (about 11 KB a row)"""
    rng = np.random.default_rng(seed)
    rows = []
    for i in range(n):
        tok = lambda: ("-" if rng.integers(2) else "0") + "0000.%022d" % int(rng.integers(1, 10 ** 14))
        rows.append("\t".join(["chr1", str(i), "+", "5", "w%d" % i, "t", "ACGTNACGTNACGTNAC"[:K], ",".join(tok() for _ in range(K)),
                               ",".join(tok() for _ in range(K)), ",".join("123456789" for _ in range(K)),
                               ",".join(tok() for _ in range(S)), "1"]).encode())
    return rows


def test_row_lengths_from_single_digits_to_wide_values(eng):
    from deepsignal_amd.engine import parse_text_reference
    rows = tc.make_rows(60, K, S, seed=11, fmt="%.0f") + tc.make_rows(60, K, S, seed=12) + _wide_rows(60, 13)
    rows = [rows[i] for i in np.random.default_rng(1).permutation(len(rows))]
    lens = sorted(map(len, rows))
    assert lens[0] < 1300 and lens[-1] > 11000 and sum(lens) + 16 * len(rows) < 256 * BLOCK_PER_ROW
    blob, begin, end = tc.pack(rows)
    ref = parse_text_reference(blob, begin, end, K, S)
    assert (ref["status"] == tc.OK).all()
    _check(eng.parse_text(blob, begin, end), ref)


def test_lengths_stepping_by_one_byte(eng, rows256):
    """1,100 rows = one row body behind a first column that grows by a byte per row: every separator, sign, dot, 'e' and last
    digit of the body falls on every byte of a 16-byte lane chunk and of a 1 KiB step, the first and the last included."""
    from deepsignal_amd.engine import parse_text_reference
    body = rows256[0][7].split(b"\t", 1)[1]               # a row with exponent-form tokens
    assert b"1e-06" in body and b"-1.2e-05" in body and b"-0." in body
    rows = [b"c" + b"x" * i + b"\t" + body for i in range(1100)]
    blob, begin, end = tc.pack(rows)
    ref = parse_text_reference(blob, begin, end, K, S)
    assert (ref["status"] == tc.OK).all()
    for k in tc.ARRAYS:
        assert (ref[k] == ref[k][0]).all()
    for a in range(0, 1100, 220):
        _check(eng.parse_text(blob, begin[a:a + 220], end[a:a + 220]), ref, np.arange(a, min(1100, a + 220)), "rows %d.." % a)


def test_spans_need_not_be_contiguous_nor_ordered_and_crlf_and_13_columns(eng, rows256):
    from deepsignal_amd.engine import parse_text_reference
    rows = rows256[0][:40]
    rows = [r + (b"\textra,1\t2" if i % 3 == 0 else b"") for i, r in enumerate(rows)]
    blob, begin, end = tc.pack(rows, sep=b"\r\n#junk,\t1.5\n")
    order = np.random.default_rng(2).permutation(40)
    crlf = np.where(np.arange(40) % 2 == 0, 1, 0)          # every other span keeps its '\r'
    b, e = begin[order], (end + crlf)[order]
    ref = parse_text_reference(blob, b, e, K, S)
    assert (ref["status"] == tc.OK).all() and np.array_equal(ref["kmer"], rows256[4]["kmer"][:40][order])
    _check(eng.parse_text(blob, b, e), ref)


def test_a_row_that_ends_with_the_block_and_one_too_long_for_it(rows256):
    """max_batch 2: the text block holds 2 x 6144 bytes. Row B behind row A ends at the block's last byte and is parsed on the
    device (its last step reads the block's pad); one byte more and it is not staged: status host."""
    from deepsignal_amd.engine import Engine, parse_text_reference
    a = rows256[0][0]
    room = 2 * BLOCK_PER_ROW - (len(a) + 15) // 16 * 16
    body = rows256[0][1].split(b"\t", 1)[1]
    e = Engine(device=0, max_batch=2)
    try:
        for extra, want in ((0, [tc.OK, tc.OK]), (1, [tc.OK, tc.HOST])):
            b = b"c" + b"x" * (room + extra - len(body) - 2) + b"\t" + body
            assert len(b) == room + extra
            blob, begin, end = tc.pack([a, b])
            ref = parse_text_reference(blob, begin, end, K, S)
            assert ref["status"].tolist() == [tc.OK, tc.OK]
            got = e.parse_text(blob, begin, end)
            assert got["status"].tolist() == want
            ok = np.flatnonzero(np.asarray(want) == tc.OK)
            tc.assert_rows_equal(got, ref, ok)
            assert np.array_equal(got["info_len"][ok], ref["info_len"][ok])
    finally:
        e.close()


def test_forms_outside_the_grammar_are_flagged_on_the_device(eng, rows256):
    from deepsignal_amd.engine import parse_text_reference
    rows = list(rows256[0][:24])

    def edit(i, col, tok_index, tok):
        c = rows[i].split(b"\t")
        if tok_index is None:
            c[col] = tok
        else:
            t = c[col].split(b",")
            t[tok_index] = tok
            c[col] = b",".join(t)
        rows[i] = b"\t".join(c)

    edit(1, 7, 0, b"+0.5"); edit(2, 10, 359, b"nan"); edit(3, 8, 16, b"12345678901234567"); edit(4, 10, 5, b"1e400")
    edit(5, 10, 100, b"inf"); edit(6, 9, 3, b"1234567890"); edit(7, 6, None, b"ACGTXACGTNACGTNAC"); edit(8, 6, None, b"ACGT")
    edit(9, 7, 4, b"1;5"); edit(10, 10, 0, b""); edit(11, 11, None, b"x")
    rows[12] = rows[12].replace(b",", b"\t", 1); rows[13] = b"\t".join(rows[13].split(b"\t")[:11]); rows[14] = b"\t\t\t"
    c = rows[15].split(b"\t"); c[7] += b",0.5"; c[8] = c[8].split(b",", 1)[1]; rows[15] = b"\t".join(c)     # 18 means, 16 stds
    blob, begin, end = tc.pack(rows)
    ref = parse_text_reference(blob, begin, end, K, S)
    assert ref["status"].tolist() == [0] + [1] * 15 + [0] * 8
    assert [tc.row_in_grammar(r, K, S) for r in rows] == [s == 0 for s in ref["status"]]
    _check(eng.parse_text(blob, begin, end), ref)


def test_a_rows_bits_do_not_depend_on_its_batch_mates(eng, rows256):
    rows, blob, begin, end, ref = rows256
    r = 100
    alone = eng.parse_text(blob, begin[r:r + 1], end[r:r + 1])
    for pos in (0, 32, 64):
        idx = np.concatenate([np.arange(64)[:pos], [r], np.arange(64)[pos:]])
        got = eng.parse_text(blob, begin[idx], end[idx])
        assert (got["status"] == tc.OK).all()
        tc.assert_rows_equal({k: got[k][pos:pos + 1] for k in tc.ARRAYS}, alone)
    tc.assert_rows_equal(alone, {k: ref[k][r:r + 1] for k in tc.ARRAYS})


def _host_route(engine, ref, idx):
    return engine.wait(engine.submit(*(ref[k][idx] for k in ("kmer", "means", "stds", "lens", "signals"))))


def test_pipeline_text_tickets_beside_a_submit_ticket(eng, rows256):
    """slots + 1 text tickets and one submit ticket through the three slots: act / pred equal submit() on the host-parsed arrays of
    the same rows; k-mer codes, labels and the info columns come back for the formatter; nothing took the host route."""
    rows, blob, begin, end, ref = rows256
    groups = [np.arange(a, b) for a, b in ((0, 60), (60, 61), (61, 125), (125, 190), (190, 256))]
    want = [_host_route(eng, ref, g) for g in groups]
    before = eng.text_stats()
    import collections
    q, got = collections.deque(), []

    def drain(limit):
        while len(q) > limit:
            kind, t = q.popleft()
            got.append(eng.wait_text(t) if kind == "text" else eng.wait(t))

    for i, g in enumerate(groups + [groups[0]]):
        drain(eng.slots - 1)
        if i == 2:
            q.append(("host", eng.submit(*(ref[k][g] for k in ("kmer", "means", "stds", "lens", "signals")))))
        else:
            q.append(("text", eng.submit_text(blob, begin[g], end[g])))
        if i == 1:
            assert len(q) == 2
    drain(0)
    assert eng.slots == 3 and len(got) == eng.slots + 3
    for i, g in enumerate(groups + [groups[0]]):
        w = want[i % len(groups)]
        assert np.array_equal(tc.bits(got[i][0]), tc.bits(w[0])) and np.array_equal(got[i][1], w[1]), i
        if i != 2:
            act, pred, kmer, labels, info, off = got[i]
            assert np.array_equal(kmer, ref["kmer"][g]) and np.array_equal(labels, ref["labels"][g])
            assert np.array_equal(np.diff(off), ref["info_len"][g])
            assert info.tobytes() == b"".join(b"\t".join(rows[j].split(b"\t")[:6]) for j in g)
    after = eng.text_stats()
    assert after["rows"] - before["rows"] == 256 + 60 - 64 and after["host_rows"] == before["host_rows"]
    assert eng.text_times()["batches"] > 0


def _planted(rows256, tmp_path, n=40):
    rows = list(rows256[0][:n])
    for i, col, j, tok in ((5, 7, 2, b"+0.5"), (17, 10, 300, b"nan"), (33, 8, 0, b"0.12345678901234567")):
        c = rows[i].split(b"\t")
        t = c[col].split(b",")
        t[j] = tok
        c[col] = b",".join(t)
        rows[i] = b"\t".join(c)
    return rows, tc.host_arrays_of(rows, K, S, tmp_path)


def test_three_planted_host_form_rows(eng, rows256, tmp_path):
    rows, host = _planted(rows256, tmp_path)
    blob, begin, end = tc.pack(rows)
    before = eng.text_stats()
    act, pred, kmer, labels, info, off = eng.wait_text(eng.submit_text(blob, begin, end))
    after = eng.text_stats()
    assert after["host_rows"] - before["host_rows"] == 3 and after["rows"] - before["rows"] == 40
    w_act, w_pred = _host_route(eng, host, np.arange(40))
    assert np.array_equal(act, w_act, equal_nan=True) and np.array_equal(pred, w_pred)      # (a NaN has no value to compare)
    fin = np.isfinite(w_act)
    assert np.array_equal(tc.bits(act)[fin], tc.bits(w_act)[fin])
    assert np.array_equal(kmer, host["kmer"]) and np.array_equal(labels, host["labels"]) and np.array_equal(np.diff(off), host["info_len"])


def _call(eng, tsv, out, parse_on, batch_size=32, f5_batch_num=7, **kw):
    from deepsignal_amd import call_modifications as cm
    return cm.call_mods(tsv, "unused", out, K, S, batch_size, 0.001, 2, 1, True, True, True, True, None, engine=eng,
                        f5_batch_num=f5_batch_num, parse_on=parse_on, **kw)


def test_a_planted_malformed_row_raises_the_host_routes_message(eng, rows256, tmp_path):
    rows = list(rows256[0][:30])
    rows[21] = rows[21].replace(b",", b";", 1)
    tsv = str(tmp_path / "bad.tsv")
    with open(tsv, "wb") as f:
        f.write(b"\n".join(rows) + b"\n")
    msgs = []
    for parse_on in ("cpu", "gpu"):
        with pytest.raises(ValueError) as ei:
            _call(eng, tsv, str(tmp_path / "o.tsv"), parse_on)
        msgs.append(str(ei.value))
    off = sum(len(r) + 1 for r in rows[:21])
    assert msgs[0] == msgs[1] == "feature file: row 22 (line at byte offset %d): malformed feature row" % off
    blob, begin, end = tc.pack(rows)
    from deepsignal_amd.engine import TextRowError
    with pytest.raises(TextRowError) as ei:
        eng.wait_text(eng.submit_text(blob, begin, end))
    assert ei.value.row == 21


def test_recheck_applies_to_the_text_route(stress_weights, rows256, tmp_path):
    """bf16_all coarse, fp32 fine, margin 0.2: the text route equals the submit route exactly, in a ticket that holds a
    host-form row too."""
    from deepsignal_amd.engine import Engine
    rows, host = _planted(rows256, tmp_path, n=200)
    keep = [i for i in range(200) if i != 17]             # (the NaN row: covered above)
    rows = [rows[i] for i in keep]
    host = {k: v[keep] for k, v in host.items()}
    blob, begin, end = tc.pack(rows)
    coarse, fine = Engine(device=0, max_batch=256, precision="bf16_all"), Engine(device=0, max_batch=256)
    try:
        coarse.load_weights(stress_weights)
        fine.load_weights(stress_weights)
        coarse.set_recheck(fine, 0.2)
        w_act, w_pred = _host_route(coarse, host, np.arange(len(rows)))
        s0 = coarse.recheck_stats()
        act, pred = coarse.wait_text(coarse.submit_text(blob, begin, end))[:2]
        assert coarse.text_stats()["host_rows"] == 2 and coarse.recheck_stats()["rechecked"] > s0["rechecked"] > 0
        assert np.array_equal(tc.bits(act), tc.bits(w_act)) and np.array_equal(pred, w_pred)
    finally:
        coarse.close()
        fine.close()


def _uneven_file(path, rows256, n=1000):
    """n rows in reads of 1 .. 23 rows"""
    rng = np.random.default_rng(3)
    base, out, read = rows256[0], [], 0
    while len(out) < n:
        for _ in range(int(rng.integers(1, 24))):
            if len(out) < n:
                c = base[len(out) % 256].split(b"\t")
                c[1], c[4] = b"%d" % len(out), b"read_%05d" % read
                out.append(b"\t".join(c))
        read += 1
    with open(path, "wb") as f:
        f.write(b"\n".join(out) + b"\n")
    return out


def test_cli_parse_on_gpu_writes_the_cpu_routes_bytes(small_weights, rows256, tmp_path, capsys):
    from deepsignal_amd import weights as W
    from deepsignal_amd.deepsignal import main
    model = str(tmp_path / "w.bin")
    W.save_weights(model, small_weights)
    tsv = str(tmp_path / "features.tsv")
    _uneven_file(tsv, rows256)
    outs = {}
    for parse_on in ("cpu", "gpu"):
        outs[parse_on] = str(tmp_path / ("calls_%s.tsv" % parse_on))
        assert main(["call_mods", "-i", tsv, "-m", model, "-o", outs[parse_on], "--batch_size", "32", "--engine_batch", "256",
                     "--f5_batch_num", "9", "--parse_on", parse_on]) == 0
    a, b = open(outs["cpu"], "rb").read(), open(outs["gpu"], "rb").read()
    assert a.count(b"\n") == 1000 and a == b
    assert "parse_on gpu: 1000 rows, 0 taken by the host parser" in capsys.readouterr().out


@pytest.mark.parametrize("form", ["crlf_and_blank_lines", "no_trailing_newline"])
def test_call_mods_line_end_forms(eng, rows256, tmp_path, form, capsys):
    """The forms of golden/malformed_tsv/ok_crlf_and_blank_lines.tsv and ok_no_trailing_newline.tsv at the default geometry (the
    corpus files are (5, 12) rows, below the engine's smallest signal window)."""
    rows = rows256[0][:50]
    data = b"\r\n\r\n".join(rows) + b"\r\n\n" if form == "crlf_and_blank_lines" else b"\n".join(rows)
    tsv = str(tmp_path / "f.tsv")
    with open(tsv, "wb") as f:
        f.write(data)
    outs = [str(tmp_path / ("o_%s.tsv" % p)) for p in ("cpu", "gpu")]
    assert _call(eng, tsv, outs[0], "cpu") == 50 and _call(eng, tsv, outs[1], "gpu") == 50
    a, b = open(outs[0], "rb").read(), open(outs[1], "rb").read()
    assert a.count(b"\n") == 50 and a == b
    assert "parse_on gpu: 50 rows, 0 taken by the host parser" in capsys.readouterr().out


def test_parse_on_gpu_usage_errors(eng, tmp_path):
    class NoText:
        max_batch, slots = 256, 1

        def run(self, *a):
            raise AssertionError("not reached")

    tsv = str(tmp_path / "f.tsv")
    open(tsv, "wb").close()
    for kw, engine, path in ((dict(native_io=False), eng, tsv), (dict(), NoText(), tsv), (dict(), eng, str(tmp_path))):
        with pytest.raises(ValueError, match="parse_on"):
            _call(engine, path, str(tmp_path / "o.tsv"), "gpu", **kw)
    with pytest.raises(ValueError, match="parse_on"):
        _call(eng, tsv, str(tmp_path / "o.tsv"), "tpu")


def test_sharded_route_with_one_rank(eng, rows256, tmp_path, capsys, monkeypatch):
    """force_sharded=True in a one-rank RCCL group (byte ranges, row gather) with parse_on gpu: the plain cpu route's bytes, and the
    summary line says the device parsed every row."""
    import socket
    import torch
    import torch.distributed as dist
    from deepsignal_amd import call_modifications as cm
    tsv = str(tmp_path / "features.tsv")
    _uneven_file(tsv, rows256, n=700)
    plain, sharded = str(tmp_path / "plain.tsv"), str(tmp_path / "sharded.tsv")
    assert _call(eng, tsv, plain, "cpu") == 700
    capsys.readouterr()
    monkeypatch.setattr(cm, "SHARD_CHUNK_BYTES", 256 << 10)           # about 10 byte ranges
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    torch.cuda.set_device(0)
    dist.init_process_group("nccl", init_method="tcp://127.0.0.1:%d" % port, rank=0, world_size=1, device_id=torch.device("cuda", 0))
    try:
        assert _call(eng, tsv, sharded, "gpu", dist=dist, force_sharded=True) == 700
    finally:
        dist.destroy_process_group()
    a, b = open(plain, "rb").read(), open(sharded, "rb").read()
    assert a.count(b"\n") == 700 and a == b
    assert "parse_on gpu: 700 rows, 0 taken by the host parser" in capsys.readouterr().out
