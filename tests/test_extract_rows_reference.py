"""CPU: the text half of the device `extract` route, run on the host. The number rule of csrc/ds_extract.h (ds_format_values with
no handle) against numpy's str(np.around(v, 6)), and the rows of ds_extract_rows_reference against the host extractor's
_features_to_str on every case of tests/extract_cases.py."""
import ctypes

import numpy as np
import pytest

from deepsignal_amd.engine import extract_reference, extract_rows_reference, format_values, load_library

import extract_cases as xc
import rows_cases as rc


def test_number_rule_matches_numpy_on_the_directed_table():
    values = rc.directed_values()
    assert len(values) > 60000
    got, want = format_values(values), rc.numpy_text(values)
    if got != want:
        g, w = got.split(b","), want.split(b",")
        bad = [(float(v), a, b) for v, a, b in zip(values, g, w) if a != b]
        raise AssertionError("%d of %d values differ, first: %r" % (len(bad) + abs(len(g) - len(w)), len(w), bad[:5]))


@pytest.mark.parametrize("values,text", [([1e-6], b"1e-06"), ([1.2e-5], b"1.2e-05"), ([1e-5], b"1e-05"), ([9.9e-5], b"9.9e-05"),
                                         ([1e-4], b"0.0001"), ([2.0, -13.25], b"2.0,-13.25"), ([-4e-7, 0.0], b"-0.0,0.0"),
                                         ([float("nan"), float("-inf")], b"nan,-inf"), ([], b"")])
def test_number_rule_examples(values, text):
    assert format_values(values) == text


def test_format_values_short_buffer_reports_the_bytes_needed():
    with pytest.raises(RuntimeError, match="31 bytes needed"):
        format_values([2.0] * 8, cap=30)
    assert format_values([2.0] * 8, cap=31) == b",".join([b"2.0"] * 8)


@pytest.mark.parametrize("name,norm", xc.case_norm_params())
def test_rows_match_the_host_extractor(name, norm):
    """Byte equality with _features_to_str for every row whose window is not SUB; SUB rows on every column but the signals. On all
    rows the signals column, narrowed to float32, carries the bits of ds_extract_reference's signals (degenerate cases: NaNs at
    the same places), which ties the text to the checker the kernels are judged by."""
    case = xc.BY_NAME[name]
    T, S = case.geometry
    for step in case.steps(norm):
        host, sub = rc.host_rows(step)
        batch, info, info_off = rc.step_inputs(step, host)
        text, row_off = extract_rows_reference(batch, info, info_off, rc.LABEL, T, S)
        rows = rc.split_rows(text, row_off)
        assert len(rows) == len(host)
        for i, (got, want) in enumerate(zip(rows, host)):
            if sub[i]:
                g, w = got.split("\t"), want.split("\t")
                assert len(g) == len(w) == 12 and g[:10] + g[11:] == w[:10] + w[11:], i
            else:
                assert got == want, i
        signals = np.array([[float(v) for v in r.split("\t")[10].split(",")] for r in rows], np.float64).astype(np.float32)
        assert xc.same_bits(signals, extract_reference(batch, T, S)["signals"], nan_positions=case.degenerate)
        if case.degenerate and norm == "mad":      # MAD == 0: the rows spell the specials out
            assert b"nan" in text and (name != "mad_is_zero" or (b",inf" in text and b"-inf" in text))


def test_row_offsets_and_short_buffer():
    step = xc.BY_NAME["window_modes_k9"].steps("mad")[0]
    host, _ = rc.host_rows(step)
    batch, info, info_off = rc.step_inputs(step, host)
    text, row_off = extract_rows_reference(batch, info, info_off, rc.LABEL, 9, 100)
    rc.split_rows(text, row_off)          # monotone offsets from 0, one newline per row at its end, last offset == byte count
    assert row_off.shape == (batch.nsites + 1,)
    lib = load_library()
    out = np.full(len(text), 0x55, np.uint8)
    off = np.full(batch.nsites + 1, -7, np.int64)
    got = lib.ds_extract_rows_reference(ctypes.byref(batch.desc), 9, 100, info.ctypes.data, info_off.ctypes.data, rc.LABEL,
                                        out.ctypes.data, len(text) - 1, off.ctypes.data)
    assert got == -len(text) and (out == 0x55).all() and (off == -7).all()
    got = lib.ds_extract_rows_reference(ctypes.byref(batch.desc), 9, 100, info.ctypes.data, info_off.ctypes.data, rc.LABEL,
                                        out.ctypes.data, len(text), off.ctypes.data)
    assert got == len(text) and out.tobytes() == text and np.array_equal(off, row_off)


def test_invalid_rows_inputs_are_refused():
    step = xc.BY_NAME["window_modes_k9"].steps("mad")[0]
    host, _ = rc.host_rows(step)
    batch, info, info_off = rc.step_inputs(step, host)
    bad = info_off.copy()
    bad[2] = bad[1] - 1
    with pytest.raises(RuntimeError, match="info_off"):
        extract_rows_reference(batch, info, bad, rc.LABEL, 9, 100)
    with pytest.raises(RuntimeError, match="ds_reads"):
        extract_rows_reference(batch, info, info_off, rc.LABEL, 10, 100)


class _CheckerEngine:
    """The rows interface of Engine on the CPU checker: lets the packing of `extract --extract_on gpu` run without a GPU."""
    slots = 2

    def __init__(self, max_batch):
        self.max_batch, self.sizes = max_batch, []

    def submit_rows(self, batch, info, info_off, label):
        self.sizes.append(batch.nsites)
        return extract_rows_reference(batch, info, info_off, label)

    def wait_rows(self, ticket):
        return ticket


@pytest.mark.parametrize("style,norm,cap", [("plain", "mad", 7), ("ont", "zscore", 64), ("latest", "mad", 4096)])
def test_device_route_packing_writes_the_host_routes_rows(style, norm, cap):
    """The worker task and the batch packing of `extract --extract_on gpu` (reads straddling batches of `cap` sites), with the
    CPU checker in the engine's place, against the host route's rows of the same files."""
    import os
    from deepsignal_amd import extract_features as ef
    d = os.path.join(os.path.dirname(__file__), "golden", "fast5", style)
    fast5s = ef.get_fast5s(d)
    task = (fast5s, "RawGenomeCorrected_000", "BaseCalled_template", norm, ["CG"], 0, None, 17, 360, 1, None)
    host, err = ef._extract_batch(task)
    assert err == 0 and host
    sub = {(f[0], str(f[1]), f[2], f[4]) for f in ef._extract_features(*task)[0] if f[9][8] >= 360}      # middle base >= S
    records, _ = ef._fast5_rows_task(task)
    assert all(r[0] == "gpu" for r in records)
    eng = _CheckerEngine(cap)
    chunks, failed = ef._rows_from_device(records, eng, norm, 1)
    got = b"".join(chunks).decode().splitlines()
    assert failed == 0 and len(got) == len(host) and sum(eng.sizes) == len(host)
    assert all(n == cap for n in eng.sizes[:-1]) and 0 < eng.sizes[-1] <= cap
    for g, w in zip(got, host):
        cw = w.split("\t")
        if (cw[0], cw[1], cw[2], cw[4]) in sub:
            cg = g.split("\t")
            assert cg[:10] + cg[11:] == cw[:10] + cw[11:]
        else:
            assert g == w
