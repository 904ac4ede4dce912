"""CPU: ds_parse_text_reference -- the device's feature-TSV row parser (csrc/ds_tsv_device.h, the token routines
tsv_parse_kernel runs) on the host -- against the native host reader and against Python's float(): every row is either parsed
to the host route's bits or flagged for the host parser, never anything else. No tolerance anywhere."""
import json
import os

import numpy as np
import pytest

import text_cases as tc

HERE = os.path.dirname(os.path.abspath(__file__))
MALFORMED = os.path.join(HERE, "golden", "malformed_tsv")


@pytest.fixture(scope="module", autouse=True)
def _built():
    import __graft_entry__ as g
    g.build()


def _reference(blob, begin, end, K, S):
    from deepsignal_amd.engine import parse_text_reference
    return parse_text_reference(blob, begin, end, K, S)


@pytest.mark.parametrize("K,S,n", [(17, 360, 120), (9, 100, 150)])
def test_arrays_equal_the_host_readers_on_seeded_files(tmp_path, K, S, n):
    rows = tc.make_rows(n, K, S, seed=K)
    blob, begin, end = tc.pack(rows)
    got = _reference(blob, begin, end, K, S)
    want = tc.host_arrays_of(rows, K, S, tmp_path)
    assert (got["status"] == tc.OK).all()
    tc.assert_rows_equal(got, want)
    assert np.array_equal(got["info_len"], want["info_len"])


def test_arrays_equal_the_host_readers_on_the_reference_golden_rows(tmp_path):
    with open(os.path.join(HERE, "golden", "harness_golden.json")) as f:
        rows = [r.encode() for r in json.load(f)["cases"][0]["tsv_rows"]]
    blob, begin, end = tc.pack(rows)
    got = _reference(blob, begin, end, 17, 360)
    want = tc.host_arrays_of(rows, 17, 360, tmp_path)
    assert len(rows) > 0 and (got["status"] == tc.OK).all()
    tc.assert_rows_equal(got, want)
    assert np.array_equal(got["info_len"], want["info_len"])


def _token_rows(floats, ints):
    """One row of geometry (1, 1) per token: a float token in the means column, an integer token in the lens column."""
    rows = [b"\t".join([b"c", b"1", b"+", b"2", b"r%d" % i, b"t", b"A", t, b"0.5", b"7", b"0.25", b"1"]) for i, t in enumerate(floats)]
    rows += [b"\t".join([b"c", b"1", b"+", b"2", b"q%d" % i, b"t", b"A", b"0.5", b"0.5", t, b"0.25", b"1"]) for i, t in enumerate(ints)]
    return rows


DEVICE_FLOATS = ["0", "-0", "0.0", "-0.0", "-0.000000", "1", "12", "123", "1234", "12345", "123456", "1234567", "12345678", "123456789",
                 "1234567890", "12345678901", "123456789012", "1234567890123", "12345678901234", "123456789012345", "0.123456789012345",
                 "000123.4500", "0000000000000000000001.5", ".5", "-.5", "5.", "-5.", "1e-06", "1.2e-05", "1E+5", "-2.5E+2", "1e22", "1e-22",
                 "1.5e22", "123e20", "0.001e-19", "999999999999999e22", "0.000001", "16777217", "0.1", "0.3", "8.5", "1.e5", "1e05", "1e-000006", "10e22"]
HOST_FLOATS = ["1234567890123456", "0.1234567890123456", "1e23", "1e-23", "0.001e-20", "10e23", "1e", "1e+", "1e-", "e5", ".e5", "+1", "+0.5", "inf",
               "-inf", "nan", "NaN", "Infinity", "1e400", "1e-400", "0x10", "1.2.3", "1 ", " 1", "", "-", ".", "--1", "1e5.0", "1f"]
DEVICE_INTS = ["0", "-0", "7", "-12", "007", "123456789", "-123456789"]
HOST_INTS = ["1234567890", "-1234567890", "+5", "5.0", "1e2", "", "-", "5 "]


def test_directed_tokens_are_strtods_bits_or_flagged():
    floats = [t.encode() for t in DEVICE_FLOATS + HOST_FLOATS if "," not in t]
    ints = [t.encode() for t in DEVICE_INTS + HOST_INTS]
    blob, begin, end = tc.pack(_token_rows(floats, ints))
    got = _reference(blob, begin, end, 1, 1)
    nf = len(floats)
    for i, t in enumerate(floats):
        if t.decode() in DEVICE_FLOATS:
            assert got["status"][i] == tc.OK, t
            want = np.float32(float(t))
            assert got["means"][i, 0].view(np.uint32) == want.view(np.uint32), (t, got["means"][i, 0], want)
            assert tc.float_in_grammar(t), t
        else:
            assert got["status"][i] == tc.HOST, t
            assert not tc.float_in_grammar(t), t
    for i, t in enumerate(ints):
        if t.decode() in DEVICE_INTS:
            assert got["status"][nf + i] == tc.OK and got["lens"][nf + i, 0] == np.float32(int(t)), t
        else:
            assert got["status"][nf + i] == tc.HOST, t
    # the label column: the same integers, with trailing '\r' and spaces tolerated
    rows = [b"\t".join([b"c", b"1", b"+", b"2", b"r", b"t", b"A", b"0.5", b"0.5", b"7", b"0.25", t])
            for t in (b"1", b"0 ", b"1\r", b"-3 \r ", b"123456789", b"1234567890", b"+1", b" 1", b"1x", b"")]
    blob, begin, end = tc.pack(rows)
    got = _reference(blob, begin, end, 1, 1)
    assert got["status"].tolist() == [0, 0, 0, 0, 0, 1, 1, 1, 1, 1] and got["labels"][:5].tolist() == [1, 0, 1, -3, 123456789]


def test_a_million_random_tokens_of_the_grammar_are_pythons_float():
    rng = np.random.default_rng(2026)
    rows_n, S = 1000, 1000
    nd = rng.integers(1, 16, rows_n * S)
    lead = rng.integers(0, 10, rows_n * S)
    mant = [int(a * 10 ** (d - 1)) + int(b) for a, b, d in zip(rng.integers(1, 10, rows_n * S), rng.integers(0, 10 ** 15, rows_n * S) % (10 ** (nd - 1)), nd)]
    frac = rng.integers(0, 19, rows_n * S)
    kind = rng.integers(0, 10, rows_n * S)
    exps = rng.integers(-22, 23, rows_n * S)
    toks = []
    for m, d, f, k, x, z in zip(mant, nd, frac, kind, exps, lead):
        s = str(m)
        f = int(f)
        if f == 0:
            s = s + ("." if k == 0 else "")
        elif f < d:
            s = s[:-f] + "." + s[-f:]
        else:
            s = ("0." if k != 1 else ".") + "0" * (f - int(d)) + s
        if z == 0:
            s = "00" + s
        if k >= 7:                                       # exponent form: the NET exponent (exponent - fraction digits) drawn in [-22, 22]
            s += ("e%+03d", "E%d", "e%+d")[k - 7] % (int(x) + f)
        if m % 2:
            s = "-" + s
        toks.append(s)
    rows = []
    for r in range(rows_n):
        rows.append(("c\t1\t+\t2\tr%d\tt\tA\t0.5\t0.5\t7\t%s\t1" % (r, ",".join(toks[r * S:(r + 1) * S]))).encode())
    blob, begin, end = tc.pack(rows)
    got = _reference(blob, begin, end, 1, S)
    bad = np.flatnonzero(got["status"] != tc.OK)
    assert bad.size == 0, [t for t in toks[bad[0] * S:(bad[0] + 1) * S] if not tc.float_in_grammar(t.encode())][:5]
    want = np.array([float(t) for t in toks], np.float64).astype(np.float32).reshape(rows_n, S)
    diff = np.flatnonzero(got["signals"].view(np.uint32).ravel() != want.view(np.uint32).ravel())
    assert diff.size == 0, [(toks[i], got["signals"].ravel()[i], want.ravel()[i]) for i in diff[:5]]


def test_malformed_corpus_rows_are_the_hosts_bits_or_flagged(tmp_path):
    with open(os.path.join(MALFORMED, "manifest.json")) as f:
        man = json.load(f)
    K, S = man["kmer_len"], man["signal_len"]
    flagged = {}
    for name, verdict in sorted(man["files"].items()):
        data = open(os.path.join(MALFORMED, name), "rb").read()
        begin, end = tc.file_lines(data)
        got = _reference(data if data else b"\n", begin, end, K, S)
        rows = [data[b:e] for b, e in zip(begin, end)]
        in_grammar = np.array([tc.row_in_grammar(r, K, S) for r in rows], bool)
        # flagged exactly when the row holds a form outside the device's grammar
        assert np.array_equal(got["status"] == tc.OK, in_grammar), name
        flagged[name] = int((~in_grammar).sum())
        if verdict.startswith("ok"):
            want = tc.host_arrays(os.path.join(MALFORMED, name), K, S)
            assert want is not None and len(want["labels"]) == len(rows) == int(verdict[3:]), name
            ok = np.flatnonzero(got["status"] == tc.OK)
            if len(rows):
                tc.assert_rows_equal(got, want, ok, name)
                assert np.array_equal(got["info_len"][ok], want["info_len"][ok]), name
        else:
            # row by row: whatever the host parser refuses is flagged, never parsed; what it accepts is flagged or has its bits
            for i, r in enumerate(rows):
                want = tc.host_arrays_of([r], K, S, tmp_path, "one.tsv")
                if want is None:
                    assert got["status"][i] == tc.HOST, (name, i)
                elif got["status"][i] == tc.OK:
                    tc.assert_rows_equal({k: got[k][i:i + 1] for k in tc.ARRAYS}, want, None, name)
            if verdict == "error":
                assert flagged[name] >= 1, name
    assert flagged["ok_plus_signs_nan_inf.tsv"] >= 1 and flagged["ok_overflow_1e400_is_inf.tsv"] >= 1
    assert flagged["ok_plain.tsv"] == 0 and flagged["ok_crlf_and_blank_lines.tsv"] == 0 and flagged["ok_extra_columns_ignored.tsv"] == 0
