"""GPU: every caller-owned output of the handle entries is written to its stated extent and nowhere else.

The rest of the suite holds the VALUES of every route to a reference, through wrappers that allocate exact-size outputs: a write
one element past n, max_batch rows written for n, a pitch of two floats at class_num 3 or a byte beyond `cap` would land in heap
or allocator padding unseen. Here every output lies between guard bands of the test's own allocation (tests/guard_bands.py):
the bands must come back intact and the extent must hold, byte for byte, what the engine wrapper returns for the same inputs on
the same handle (those values are held to their references elsewhere; every route here is deterministic). The device path
(ds_forward_device, whose scatter kernel writes straight into the caller's device memory) runs with banded device tensors.
"""
import ctypes

import numpy as np
import pytest

from deepsignal_amd import engine as E
from deepsignal_amd import synth, weights as W
from deepsignal_amd.engine import Engine

import guard_bands as gb
import hostile_cases as hc
import rows_cases as rc
import text_cases as tc
from combine_cases import random_table
from freq_cases import random_rows
import train_statement as ts
import train_statement_base as tsb

pytestmark = pytest.mark.gpu

B = 128                      # max_batch of the forward engines: the rows a band holds
KEYS = hc.KEYS
T9, S100 = 9, 100            # the short geometry
INVALID = -1                 # DS_ERR_INVALID


@pytest.fixture(scope="module", autouse=True)
def _built():
    import __graft_entry__ as g
    g.build()


def _args(f, lo=0, hi=None):
    return tuple(np.ascontiguousarray(f[k][lo:hi]) for k in KEYS)


def _ptrs(arrs):
    return tuple(a.ctypes.data for a in arrs)


# ---- engines, module-scoped ----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def engines(small_weights):
    """Default-geometry engines with max_batch 128 by (precision, slots, class_num), made at first use."""
    made = {}

    def get(precision="fp32", slots=1, class_num=2):
        key = (precision, slots, class_num)
        if key not in made:
            w = small_weights if class_num == 2 else W.random_weights(seed=8, lstm_bias_std=0.1, class_num=class_num)
            e = Engine(device=0, max_batch=B, precision=precision, slots=slots, class_num=class_num)
            e.load_weights(w)
            made[key] = e
        return made[key]
    yield get
    for e in made.values():
        e.close()


@pytest.fixture(scope="module")
def short_weights():
    return W.random_weights(seed=7, lstm_bias_std=0.1, kmer_len=T9, signal_len=S100)


@pytest.fixture(scope="module")
def short(short_weights):
    """Short geometry (kmer_len 9, signal_len 100), max_batch 128, three slots, weights loaded."""
    e = Engine(kmer_len=T9, signal_len=S100, device=0, max_batch=B, slots=3)
    e.load_weights(short_weights)
    yield e
    e.close()


@pytest.fixture(scope="module")
def short_feats():
    return synth.synthetic_features(2 * B + 5, seed=11, kmer_len=T9, signal_len=S100)


@pytest.fixture(scope="module")
def table_engine():
    """The table routes need no weights."""
    e = Engine(device=0, max_batch=64, slots=1)
    yield e
    e.close()


# ---- ds_forward_device ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def plain128():
    f = synth.synthetic_features(B, seed=hc.SEED)
    return {k: f[k] for k in KEYS}


def _device_inputs(f, n):
    import torch
    dev = torch.device("cuda", 0)
    return [torch.from_numpy(a).to(dev) for a in _args(f, 0, n)]


def _device_outputs(n, class_num):
    d_act = gb.banded((n, class_num), np.float32, B, device="cuda:0", what="d_act")
    d_pred = gb.banded((n,), np.int32, B, device="cuda:0", what="d_pred")
    return d_act, d_pred


DEVICE_CASES = [("fp32", 2, n) for n in (1, 31, 32, 33, 70, 127, 128)] + \
               [(p, 2, 70) for p in ("bf16", "bf16_all", "bf16x3", "fp16x2")] + [("fp32", 3, 1), ("fp32", 3, 33)]


@pytest.mark.parametrize("slots", [1, 3])
@pytest.mark.parametrize("precision,class_num,n", DEVICE_CASES)
def test_forward_device_writes_n_rows_and_no_other_byte(engines, plain128, precision, class_num, n, slots):
    """act[n, class_num] and pred[n] in banded device tensors; four runs per size (eager, captured, replayed twice), on one slot
    and rotating over three. The bits are those of ds_forward on the same rows."""
    eng = engines(precision, slots, class_num)
    act, pred = eng.run(*_args(plain128, 0, n))
    d_in = _device_inputs(plain128, n)
    d_act, d_pred = _device_outputs(n, class_num)
    for rep in range(4):
        d_act.refill()
        d_pred.refill()
        rcode = gb.call(eng._lib, "ds_forward_device", eng._h, n, *(x.data_ptr() for x in d_in), d_act, d_pred)
        assert rcode == 0, eng._lib.ds_last_error(eng._h)
        eng.sync()
        d_pred.check("d_pred, n = %d, run %d" % (n, rep))
        d_act.check("d_act, n = %d, run %d" % (n, rep))
        gb.same_bytes(d_act, act, "d_act, n = %d, run %d" % (n, rep))
        gb.same_bytes(d_pred, pred, "d_pred, n = %d, run %d" % (n, rep))


def test_forward_device_ragged_after_full(engines, plain128):
    """n = 128, then n = 1 on the same slot: nothing of the full batch reaches the bytes behind pred[0] / act[0]."""
    eng = engines("fp32", 1, 2)
    d_in = _device_inputs(plain128, B)
    act1, pred1 = eng.run(*_args(plain128, 0, 1))
    full = _device_outputs(B, 2)
    one = _device_outputs(1, 2)
    for n, (d_act, d_pred) in ((B, full), (1, one)):
        assert gb.call(eng._lib, "ds_forward_device", eng._h, n, *(x.data_ptr() for x in d_in), d_act, d_pred) == 0
        eng.sync()
        d_act.check()
        d_pred.check()
    gb.same_bytes(one[0], act1)
    gb.same_bytes(one[1], pred1)


def _nan_banded_input(a, rows_per_band):
    """`a` on the device between two bands of `rows_per_band` rows whose every 32-bit word is 0xFFFFFFFF: a NaN as float32."""
    import torch
    row = a.itemsize * int(np.prod(a.shape[1:]))
    band = (max(rows_per_band * row, gb.MIN_BAND_BYTES) + gb.ALIGN - 1) // gb.ALIGN * gb.ALIGN
    raw = torch.full((2 * band + a.nbytes + gb.ALIGN,), 0xFF, dtype=torch.uint8, device="cuda:0")
    at = (-raw.data_ptr()) % gb.ALIGN + band
    raw[at:at + a.nbytes] = torch.from_numpy(np.ascontiguousarray(a).reshape(-1).view(np.uint8)).to("cuda:0")
    return raw, raw.data_ptr() + at


@pytest.mark.parametrize("precision", ["fp32", "bf16_all"])
def test_forward_device_reads_only_its_n_input_rows(engines, plain128, precision):
    """The five inputs lie between NaN bands, so nothing finite stands behind row n - 1 or in front of row 0: a gather that is off
    by a row, or rows behind n that reach a site's result, change the outputs. (A gather that merely copies more rows than n
    into the slot's own workspace stays invisible by the isolation guarantee; it costs time, not correctness.)"""
    n = 70
    eng = engines(precision, 1, 2)
    act, pred = eng.run(*_args(plain128, 0, n))
    keep = [_nan_banded_input(a, B) for a in _args(plain128, 0, n)]
    d_act, d_pred = _device_outputs(n, 2)
    for rep in range(2):
        d_act.refill()
        d_pred.refill()
        assert gb.call(eng._lib, "ds_forward_device", eng._h, n, *(p for _, p in keep), d_act, d_pred) == 0
        eng.sync()
        d_act.check()
        d_pred.check()
        gb.same_bytes(d_act, act, "act with banded inputs, run %d" % rep)
        gb.same_bytes(d_pred, pred, "pred with banded inputs, run %d" % rep)


def test_forward_device_refusals_write_nothing(engines, plain128):
    eng = engines("fp32", 1, 2)
    d_in = [x.data_ptr() for x in _device_inputs(plain128, B)]
    d_act, d_pred = _device_outputs(B, 2)
    assert gb.call(eng._lib, "ds_forward_device", eng._h, B + 1, *d_in, d_act, d_pred) == INVALID
    assert gb.call(eng._lib, "ds_forward_device", eng._h, 70, *d_in, None, d_pred) == INVALID
    assert gb.call(eng._lib, "ds_forward_device", eng._h, 70, *d_in, d_act, None) == INVALID
    assert gb.call(eng._lib, "ds_forward_device", eng._h, 70, d_in[0], None, *d_in[2:], d_act, d_pred) == INVALID
    eng.sync()
    d_act.check()
    d_pred.check()
    assert d_act.untouched() and d_pred.untouched()


# ---- ds_forward, ds_submit / ds_wait, ds_submit_parts ------------------------------------------------------------------------------
def _host_outputs(n, class_num=2, rows=B):
    return gb.banded((n, class_num), np.float32, rows, what="act"), gb.banded((n,), np.int32, rows, what="pred")


@pytest.mark.parametrize("n", [1, 70, 2 * B + 5])
def test_forward_host_outputs(short, short_feats, n):
    """2 x max_batch + 5 rows: the chunk loop's offsets (three waits, the last one of five rows)."""
    a = _args(short_feats, 0, n)
    act, pred = short.run(*a)
    b_act, b_pred = _host_outputs(n)
    assert gb.call(short._lib, "ds_forward", short._h, n, *_ptrs(a), b_act, b_pred) == 0
    gb.same_bytes(b_act, act)
    gb.same_bytes(b_pred, pred)


@pytest.mark.parametrize("n", [70, 2 * B + 5])
def test_forward_with_a_recheck_on_a_smaller_fine_handle(short_weights, short_feats, n):
    """bf16_all checked again in fp32 on a fine handle of max_batch 32: the merge writes the selected rows of act / pred only."""
    fine = Engine(kmer_len=T9, signal_len=S100, device=0, max_batch=32, slots=2)
    fine.load_weights(short_weights)
    coarse = Engine(kmer_len=T9, signal_len=S100, device=0, max_batch=B, slots=3, precision="bf16_all")
    coarse.load_weights(short_weights)
    try:
        a = _args(short_feats, 0, n)
        plain_act, _ = coarse.run(*a)
        p = plain_act / plain_act.sum(axis=1, keepdims=True)
        margin = float(np.median(np.abs(p[:, 1] - p[:, 0])))            # about half the sites are checked again
        coarse.set_recheck(fine, margin)
        act, pred = coarse.run(*a)
        before = coarse.recheck_stats()["rechecked"]
        assert 0 < before < n
        b_act, b_pred = _host_outputs(n)
        assert gb.call(coarse._lib, "ds_forward", coarse._h, n, *_ptrs(a), b_act, b_pred) == 0
        gb.same_bytes(b_act, act)
        gb.same_bytes(b_pred, pred)
        sites, rechecked, forwards = (gb.scalar(np.int64) for _ in range(3))
        assert gb.call(coarse._lib, "ds_get_recheck_stats", coarse._h, sites, rechecked, forwards) == 0
        assert int(rechecked.view[0]) == 2 * before and int(sites.view[0]) == 2 * n
        launches, ms = gb.scalar(np.int64), gb.banded((1,), np.float64, 1)
        assert gb.call(coarse._lib, "ds_get_recheck_times", coarse._h, 0, launches, ms) == 0
        assert launches.written() and ms.written()
        # a ticket with a recheck: ds_wait merges into the caller's rows
        m = 70
        t = gb.scalar(np.int32)
        assert gb.call(coarse._lib, "ds_submit", coarse._h, m, *_ptrs(_args(short_feats, 0, m)), t) == 0
        w_act, w_pred = _host_outputs(m)
        assert gb.call(coarse._lib, "ds_wait", coarse._h, int(t.view[0]), w_act, w_pred) == 0
        ref_act, ref_pred = coarse.run(*_args(short_feats, 0, m))
        gb.same_bytes(w_act, ref_act)
        gb.same_bytes(w_pred, ref_pred)
    finally:
        coarse.close()
        fine.close()


def test_submit_wait_and_submit_parts(short, short_feats):
    n = 70
    a = _args(short_feats, 0, n)
    act, pred = short.wait(short.submit(*a))
    for rep in range(short.slots + 1):                    # every slot's pinned block, and the first one again
        t = gb.scalar(np.int32, "ticket")
        assert gb.call(short._lib, "ds_submit", short._h, n, *_ptrs(a), t) == 0
        assert 0 <= int(t.view[0]) < short.slots
        b_act, b_pred = _host_outputs(n)
        assert gb.call(short._lib, "ds_wait", short._h, int(t.view[0]), b_act, b_pred) == 0
        gb.same_bytes(b_act, act)
        gb.same_bytes(b_pred, pred)
    # a wait that is refused writes nothing
    b_act, b_pred = _host_outputs(n)
    assert gb.call(short._lib, "ds_wait", short._h, 0, b_act, b_pred) == INVALID
    assert b_act.untouched() and b_pred.untouched()
    # the same rows as four segments
    cuts = [0, 1, 32, 33, n]
    parts = [_args(short_feats, s, e) for s, e in zip(cuts[:-1], cuts[1:])]
    k = len(parts)
    counts = (ctypes.c_int32 * k)(*[e - s for s, e in zip(cuts[:-1], cuts[1:])])
    ptrs = [(ctypes.c_void_p * k)(*[p[j].ctypes.data for p in parts]) for j in range(5)]
    t = gb.scalar(np.int32, "ticket")
    assert gb.call(short._lib, "ds_submit_parts", short._h, k, counts, *ptrs, t) == 0
    b_act, b_pred = _host_outputs(n)
    assert gb.call(short._lib, "ds_wait", short._h, int(t.view[0]), b_act, b_pred) == 0
    gb.same_bytes(b_act, act)
    gb.same_bytes(b_pred, pred)
    # a ragged ticket right after a full one on the same slot
    one = Engine(kmer_len=T9, signal_len=S100, device=0, max_batch=B, slots=1)
    try:
        one.load_weights(W.random_weights(seed=7, lstm_bias_std=0.1, kmer_len=T9, signal_len=S100))
        one.wait(one.submit(*_args(short_feats, 0, B)))
        act1, pred1 = short.run(*_args(short_feats, 0, 1))
        t = gb.scalar(np.int32, "ticket")
        assert gb.call(one._lib, "ds_submit", one._h, 1, *_ptrs(_args(short_feats, 0, 1)), t) == 0
        b_act, b_pred = _host_outputs(1)
        assert gb.call(one._lib, "ds_wait", one._h, int(t.view[0]), b_act, b_pred) == 0
        gb.same_bytes(b_act, act1)
        gb.same_bytes(b_pred, pred1)
    finally:
        one.close()


# ---- extraction and rows ----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def read_batch():
    """70 CG sites of two synthetic reads at the short geometry, and the six leading columns of their rows."""
    return rc.two_read_batch(T9, "mad")


def test_extract_and_submit_reads(short, read_batch):
    batch = read_batch[0]
    n = batch.nsites
    assert n == 70 < B
    ref = short.extract(batch)
    outs = [gb.banded(ref[k].shape, ref[k].dtype, B, what=k) for k in KEYS]
    assert gb.call(short._lib, "ds_extract", short._h, ctypes.byref(batch.desc), *outs) == 0, short._lib.ds_last_error(short._h)
    for k, b in zip(KEYS, outs):
        gb.same_bytes(b, ref[k], k)
    act, pred = short.wait(short.submit_reads(batch))
    t = gb.scalar(np.int32, "ticket")
    assert gb.call(short._lib, "ds_submit_reads", short._h, ctypes.byref(batch.desc), t) == 0
    b_act, b_pred = _host_outputs(n)
    assert gb.call(short._lib, "ds_wait", short._h, int(t.view[0]), b_act, b_pred) == 0
    gb.same_bytes(b_act, act)
    gb.same_bytes(b_pred, pred)


def _row_outputs(nbytes, n, longest):
    return (gb.banded((nbytes,), np.uint8, B * longest, what="out"), gb.banded((n + 1,), np.int64, B, what="row_off"))


def test_rows_exact_capacity_and_one_byte_short(short, read_batch):
    batch, info, info_off = read_batch
    n, lib, h = batch.nsites, short._lib, short._h
    text, off = short.extract_rows(batch, info, info_off, rc.LABEL)
    total, longest = len(text), int(np.diff(off).max())
    desc, ip, op = ctypes.byref(batch.desc), info.ctypes.data, info_off.ctypes.data
    # the blocking entry
    out, row_off = _row_outputs(total, n, longest)
    assert gb.call(lib, "ds_extract_rows", h, desc, ip, op, rc.LABEL, out, total, row_off) == total
    gb.same_bytes(out, np.frombuffer(text, np.uint8))
    gb.same_bytes(row_off, off)
    out, row_off = _row_outputs(total - 1, n, longest)
    assert gb.call(lib, "ds_extract_rows", h, desc, ip, op, rc.LABEL, out, total - 1, row_off) == -total
    assert out.untouched() and row_off.untouched()
    out, _ = _row_outputs(total, n, longest)
    assert gb.call(lib, "ds_extract_rows", h, desc, ip, op, rc.LABEL, out, total, None) == total        # row_off is optional
    gb.same_bytes(out, np.frombuffer(text, np.uint8))
    # the ticket pair: a short buffer keeps the ticket
    t = gb.scalar(np.int32, "ticket")
    assert gb.call(lib, "ds_submit_rows", h, desc, ip, op, rc.LABEL, t) == 0
    out, row_off = _row_outputs(total - 1, n, longest)
    assert gb.call(lib, "ds_wait_rows", h, int(t.view[0]), out, total - 1, row_off) == -total
    assert out.untouched() and row_off.untouched()
    out, row_off = _row_outputs(total, n, longest)
    assert gb.call(lib, "ds_wait_rows", h, int(t.view[0]), out, total, row_off) == total
    gb.same_bytes(out, np.frombuffer(text, np.uint8))
    gb.same_bytes(row_off, off)
    out, row_off = _row_outputs(total, n, longest)
    assert gb.call(lib, "ds_wait_rows", h, int(t.view[0]), out, total, row_off) == INVALID                # consumed
    assert out.untouched() and row_off.untouched()
    batches, ms = gb.scalar(np.int64), gb.banded((5,), np.float64, 1)
    assert gb.call(lib, "ds_get_rows_times", h, 0, batches, ms) == 0
    assert batches.written() and ms.written()


def test_format_values_on_the_device(short):
    values = np.ascontiguousarray(rc.directed_values()[:700])
    want = E.format_values(values, engine=short)
    total = len(want)
    out = gb.banded((total,), np.uint8, 28 * B, what="out")
    assert gb.call(short._lib, "ds_format_values", short._h, values.size, values.ctypes.data, out, total) == total
    gb.same_bytes(out, np.frombuffer(want, np.uint8))
    out = gb.banded((total - 1,), np.uint8, 28 * B, what="out")
    assert gb.call(short._lib, "ds_format_values", short._h, values.size, values.ctypes.data, out, total - 1) == -total
    assert out.untouched()


# ---- text ----------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def text70():
    rows = tc.make_rows(70, T9, S100, seed=5)
    return tc.pack(rows)


def test_parse_text(short, text70):
    blob, begin, end = text70
    n = len(begin)
    ref = short.parse_text(blob, begin, end)
    assert (ref["status"] == tc.OK).all()
    outs = [gb.banded(ref[k].shape, ref[k].dtype, B, what=k) for k in E._TEXT_ORDER]
    keep = np.frombuffer(blob, np.uint8)
    rcode = gb.call(short._lib, "ds_parse_text", short._h, keep.ctypes.data, n, begin.ctypes.data, end.ctypes.data, *outs)
    assert rcode == 0, short._lib.ds_last_error(short._h)
    for k, b in zip(E._TEXT_ORDER, outs):
        gb.same_bytes(b, ref[k], k)
    outs[6] = None                                         # info_len is optional
    for b in outs[:6] + outs[7:]:
        b.refill()
    assert gb.call(short._lib, "ds_parse_text", short._h, keep.ctypes.data, n, begin.ctypes.data, end.ctypes.data, *outs) == 0
    gb.same_bytes(outs[7], ref["status"])
    rows, host_rows = gb.scalar(np.int64), gb.scalar(np.int64)
    assert gb.call(short._lib, "ds_get_text_stats", short._h, rows, host_rows) == 0
    assert rows.written() and host_rows.written()
    batches, ms = gb.scalar(np.int64), gb.banded((3,), np.float64, 1)
    assert gb.call(short._lib, "ds_get_text_times", short._h, 0, batches, ms) == 0
    assert int(batches.view[0]) >= 2 and ms.written()


def _text_outputs(n, info_bytes):
    return [gb.banded((n, 2), np.float32, B, what="act"), gb.banded((n,), np.int32, B, what="pred"),
            gb.banded((n, T9), np.int32, B, what="kmer"), gb.banded((n,), np.int32, B, what="labels"),
            gb.banded((info_bytes,), np.uint8, B * 64, what="info"), gb.banded((n + 1,), np.int64, B, what="info_off")]


def test_wait_text_exact_info_capacity_and_one_short(short, text70):
    """A short info_cap (include/deepsignal_hip.h, ds_wait_text): DS_ERR_INVALID, nothing in info, act / pred / kmer / labels and
    all n + 1 info_off entries written (info_off[n] = the bytes needed), the ticket consumed."""
    blob, begin, end = text70
    n, lib, h = len(begin), short._lib, short._h
    keep = np.frombuffer(blob, np.uint8)
    ref = short.wait_text(short.submit_text(blob, begin, end))
    need = int(ref[5][n])
    assert need == ref[4].size > 0

    def submit():
        t = gb.scalar(np.int32, "ticket")
        assert gb.call(lib, "ds_submit_text", h, keep.ctypes.data, n, begin.ctypes.data, end.ctypes.data, t) == 0
        return int(t.view[0])
    t = submit()
    outs = _text_outputs(n, need)
    assert gb.call(lib, "ds_wait_text", h, t, *outs[:5], need, outs[5]) == 0, lib.ds_last_error(h)
    for b, want in zip(outs, ref):
        gb.same_bytes(b, want)
    t = submit()
    outs = _text_outputs(n, need - 1)
    assert gb.call(lib, "ds_wait_text", h, t, *outs[:5], need - 1, outs[5]) == INVALID
    assert b"bytes needed" in lib.ds_last_error(h)
    assert outs[4].untouched()
    for b, want in zip(outs[:4] + outs[5:], ref[:4] + ref[5:]):
        gb.same_bytes(b, want)
    outs = _text_outputs(n, need)
    assert gb.call(lib, "ds_wait_text", h, t, *outs[:5], need, outs[5]) == INVALID            # the failed wait consumed the ticket
    assert all(b.untouched() for b in outs)


def test_recheck_select(short):
    n = 70
    rng = np.random.default_rng(3)
    act = rng.random((n, 2)).astype(np.float32)
    act[5], act[69] = (np.nan, 0.5), (0.5, np.inf)
    want = short.recheck_select(act, 0.3)
    assert 0 < want.size < n
    count, index = gb.scalar(np.int32, "count"), gb.banded((n,), np.int32, B, what="index")
    assert gb.call(short._lib, "ds_recheck_select", short._h, n, act.ctypes.data, ctypes.c_float(0.3), count, index) == 0
    assert int(count.view[0]) == want.size and index.view[:want.size].tolist() == want.tolist()      # index[count .. n) is not specified


# ---- frequency -----------------------------------------------------------------------------------------------------------------------
def _sorted_columns(cols, keys):
    order = np.lexsort(tuple(np.asarray(cols[k]) for k in reversed(keys)))
    return {k: np.asarray(v)[order] for k, v in cols.items()}


def test_freq_parse_and_result(table_engine):
    eng = table_engine
    lib, h = eng._lib, eng._h
    text = ("\n".join(random_rows(5, 200, 40, 3)) + "\n").encode()
    begin, end, chrom, flags, names = E.freq_locate(text)
    n = len(begin)
    keep = np.frombuffer(text, np.uint8)
    eng.freq_begin(n, n)
    try:
        want_status = eng.freq_parse(text, begin, end, chrom, flags)
        eng.freq_accumulate()
        ref = eng.freq_result()
    finally:
        eng.freq_end()
    sites = len(ref["first_row"])
    assert 1 < sites <= 40 and (want_status == E.TEXT_ROW_OK).all()
    fields = E._FREQ_SITE_FIELDS
    eng.freq_begin(n, n)
    try:
        status = gb.banded((n,), np.int32, n, what="status")
        rcode = gb.call(lib, "ds_freq_parse", h, keep.ctypes.data, n, begin.ctypes.data, end.ctypes.data, chrom.ctypes.data, flags.ctypes.data,
                        status)
        assert rcode == 0, lib.ds_last_error(h)
        gb.same_bytes(status, want_status)
        eng._freq.pending = n
        eng.freq_accumulate()
        for cap in (sites, sites - 1):
            outs = [gb.banded((cap,), dt, n, what=k) for k, dt in fields]
            rows, used = gb.scalar(np.int64, "rows"), gb.scalar(np.int64, "used")
            got = gb.call(lib, "ds_freq_result", h, cap, *outs, rows, used)
            if cap < sites:
                assert got == INVALID and all(b.untouched() for b in outs)
            else:
                assert got == sites and int(rows.view[0]) == ref["rows"] and int(used.view[0]) == ref["used"]
                a = _sorted_columns({k: b.array() for (k, _), b in zip(fields, outs)}, ["first_row"])
                w = _sorted_columns({k: ref[k] for k, _ in fields}, ["first_row"])
                for k, _ in fields:
                    assert a[k].tobytes() == w[k].tobytes(), k
        batches, ms = gb.scalar(np.int64), gb.banded((4,), np.float64, 1)
        assert gb.call(lib, "ds_get_freq_times", h, 0, batches, ms) == 0
        assert int(batches.view[0]) >= 2 and ms.written()
    finally:
        eng.freq_end()


def test_freq_push_and_values(table_engine):
    eng = table_engine
    lib, h = eng._lib, eng._h
    act = np.array([[0.2, 0.8], [0.5, 0.5], [0.0, 0.0], [0.3, 0.7], [0.1, 0.9], [0.4, 0.6], [0.25, 0.75]], np.float32)
    chrom = np.array([0, 1, 0, 1, 0, -1, 0], np.int32)
    pos = np.array([7, 9, 7, 9, 7, 3, 1 << 40], np.int64)
    pred = np.array([1, 0, 1, 1, 1, 1, 1], np.int32)
    over = ([2, 5, 6], [0, 2, 2], [7, 3, 3], [float("nan"), 0.4, 0.5], [0.5, 0.6, 0.5], [1, 1, 1])
    n = len(pred)
    eng.freq_begin_stream(1, 16, 0.3)
    try:
        want_status = eng.freq_push(chrom, pos, act, pred)
        want_opened = eng.freq_accumulate(*over)
    finally:
        eng.freq_end()
    eng.freq_begin_stream(1, 16, 0.3)
    try:
        status, opened = gb.banded((n,), np.int32, 16, what="status"), gb.banded((n,), np.int32, 16, what="opened")
        rcode = gb.call(lib, "ds_freq_push", h, n, chrom.ctypes.data, pos.ctypes.data, act.ctypes.data, 2, pred.ctypes.data, status, opened)
        assert rcode == 0, lib.ds_last_error(h)
        gb.same_bytes(status, want_status)
        eng._freq.pending = n
        eng.freq_accumulate(*over)                   # the library fills `opened` now
        opened.check()
        status.check()
        gb.same_bytes(opened, want_opened)
        growths, ms = gb.scalar(np.int64), gb.banded((2,), np.float64, 1)
        assert gb.call(lib, "ds_get_freq_stream_times", h, 0, growths, ms) == 0
        assert growths.written() and ms.written()
    finally:
        eng.freq_end()
    rows = np.random.default_rng(4).random((100, 2)).astype(np.float32)
    rows[3] = (np.nan, 1.0)
    w0, w1, ws = eng.freq_values(rows)
    p0, p1, st = gb.banded((100,), np.float64, 100), gb.banded((100,), np.float64, 100), gb.banded((100,), np.int32, 100)
    assert gb.call(lib, "ds_freq_values", h, 100, rows.ctypes.data, 2, p0, p1, st) == 0
    gb.same_bytes(p0, w0)
    gb.same_bytes(p1, w1)
    gb.same_bytes(st, ws)


# ---- combine -------------------------------------------------------------------------------------------------------------------------
def test_combine_parse_result_and_bitmap(table_engine):
    eng = table_engine
    lib, h = eng._lib, eng._h
    rng = np.random.default_rng(12)
    seq = "".join(rng.choice(list("ACGTcg"), 333, p=[0.1, 0.3, 0.3, 0.1, 0.1, 0.1]))
    fasta = (">ctg0\n" + seq + "\n").encode()
    seg = [np.array([6], np.int64), np.array([6 + len(seq)], np.int64), np.array([0], np.int64), np.array([0], np.uint8)]
    rec_len = np.array([len(seq)], np.int64)
    text = ("\n".join(random_table(3, {"ctg0": seq.upper()}, 150)) + "\n").encode()
    keep = np.frombuffer(text, np.uint8)
    begin, end, local, flags, names = E.freq_locate(text)
    chrom = np.array([0 if nm == b"ctg0" else -1 for nm in names] + [-1], np.int32)[local]
    n = len(begin)

    def accumulate(status):
        host = np.flatnonzero(np.asarray(status) == E.TEXT_ROW_HOST).tolist()
        eng.combine_accumulate(host, [None] * len(host))

    eng.combine_begin(E.COMBINE_TABLE, rec_len, n, n)
    try:
        eng.combine_genome(fasta, *seg)
        want_bitmap = eng.combine_bitmap()
        want_status = eng.combine_parse(text, begin, end, chrom, flags)
        accumulate(want_status)
        ref = eng.combine_result()
    finally:
        eng.combine_end()
    sites, words = len(ref["pos"]), want_bitmap.size
    assert sites > 1 and words == 11 and want_bitmap.any()
    fields = E._COMBINE_SITE_FIELDS
    eng.combine_begin(E.COMBINE_TABLE, rec_len, n, n)
    try:
        eng.combine_genome(fasta, *seg)
        for cap in (words, words - 1):
            bitmap = gb.banded((cap,), np.uint32, 1024, what="bitmap")
            got = gb.call(lib, "ds_combine_bitmap", h, cap, bitmap)
            if cap < words:
                assert got == INVALID and bitmap.untouched()
            else:
                assert got == 0
                gb.same_bytes(bitmap, want_bitmap)
        status = gb.banded((n,), np.int32, n, what="status")
        rcode = gb.call(lib, "ds_combine_parse", h, keep.ctypes.data, n, begin.ctypes.data, end.ctypes.data, chrom.ctypes.data, flags.ctypes.data,
                        status)
        assert rcode == 0, lib.ds_last_error(h)
        gb.same_bytes(status, want_status)
        eng._combine.pending = n
        accumulate(want_status)
        for cap in (sites, sites - 1):
            outs = [gb.banded((cap,), dt, n, what=k) for k, dt in fields]
            rows = gb.scalar(np.int64, "rows")
            got = gb.call(lib, "ds_combine_result", h, cap, *outs, rows)
            if cap < sites:
                assert got == INVALID and all(b.untouched() for b in outs)
            else:
                assert got == sites and int(rows.view[0]) == ref["rows"]
                a = _sorted_columns({k: b.array() for (k, _), b in zip(fields, outs)}, ["chrom", "pos"])
                w = _sorted_columns({k: ref[k] for k, _ in fields}, ["chrom", "pos"])
                for k, _ in fields:
                    assert a[k].tobytes() == w[k].tobytes(), k
        chunks, batches, ms = gb.scalar(np.int64), gb.scalar(np.int64), gb.banded((5,), np.float64, 1)
        assert gb.call(lib, "ds_get_combine_times", h, 0, chunks, batches, ms) == 0
        assert int(chunks.view[0]) >= 2 and int(batches.view[0]) >= 2 and ms.written()
    finally:
        eng.combine_end()


# ---- evaluate ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ncf", [1, 32])
def test_eval_parse_and_result(table_engine, ncf):
    """counts is 2 x (4 + 2 ncf) entries: six at one cut-off, not the 68 of the 32 the run may take."""
    eng = table_engine
    lib, h = eng._lib, eng._h
    r = np.random.default_rng(ncf)
    n = 120
    rows = ["chr1\t100\t+\t900\tread\tt\t%.6f\t%.6f\t%d\tACGTACGTCGACGTACG" % (1 - p, p, p > 0.5) for p in np.round(r.random(n), 2)]
    text = ("\n".join(rows) + "\n").encode()
    keep = np.frombuffer(text, np.uint8)
    begin, end, flags, _ = E.eval_locate(text)
    mask = np.full(n, E.EVAL_SET_ALL | E.EVAL_SET_SAMPLE, np.uint8)
    mask[::3] = E.EVAL_SET_ALL
    mask[r.random(n) < 0.5] |= E.EVAL_TRUTH
    cf = np.linspace(0.0, 0.9, ncf)
    eng.eval_begin(n, n, cf)
    try:
        want_status = eng.eval_parse(text, begin, end, flags)
        eng.eval_accumulate(mask)
        ref = eng.eval_result()
    finally:
        eng.eval_end()
    assert (want_status == E.TEXT_ROW_OK).all()
    eng.eval_begin(n, n, cf)
    try:
        status = gb.banded((n,), np.int32, n, what="status")
        rcode = gb.call(lib, "ds_eval_parse", h, keep.ctypes.data, n, begin.ctypes.data, end.ctypes.data, flags.ctypes.data, status)
        assert rcode == 0, lib.ds_last_error(h)
        gb.same_bytes(status, want_status)
        eng._eval.pending = n
        eng.eval_accumulate(mask)
        counts = gb.banded((2, 4 + 2 * ncf), np.int64, E.EVAL_MAX_CF, what="counts")
        u2, pn, nn = gb.banded((2,), np.uint64, 1, what="u2"), gb.banded((2,), np.int64, 1, what="pn"), gb.banded((2,), np.int64, 1, what="nn")
        nrows, distinct = gb.scalar(np.int64, "rows"), gb.scalar(np.int64, "distinct")
        assert gb.call(lib, "ds_eval_result", h, counts, u2, pn, nn, nrows, distinct) == 0, lib.ds_last_error(h)
        gb.same_bytes(counts, ref["counts"])
        assert u2.view.tolist() == ref["u2"] and pn.view.tolist() == ref["p"] and nn.view.tolist() == ref["n"]
        assert int(nrows.view[0]) == n and int(distinct.view[0]) == ref["distinct"]
        batches, ms = gb.scalar(np.int64), gb.banded((4,), np.float64, 1)
        assert gb.call(lib, "ds_get_eval_times", h, 0, batches, ms) == 0
        assert batches.written() and ms.written()
    finally:
        eng.eval_end()


# ---- training, on max_batch = 96 handles -----------------------------------------------------------------------------------------------
TB = 96
T5, S40 = 5, 40


@pytest.fixture(scope="module")
def train_engines():
    made = {}

    def get(kind):
        if kind not in made:
            if kind == "signal":
                kw = dict(signal_len=S40, is_cnn=True, is_rnn=False)
                w = W.random_weights(seed=7, signal_len=S40, randomize_bn=True, is_cnn=True, is_rnn=False)
            else:
                kw = dict(kmer_len=T5, is_cnn=False, is_base=kind == "base")
                w = W.random_weights(seed=7, kmer_len=T5, is_cnn=False, is_base=kind == "base")
            e = Engine(max_batch=TB, **kw)
            e.load_weights(w)
            made[kind] = e
        return made[kind]
    yield get
    for e in made.values():
        e.close()


def _train_outputs(n, logits):
    out = [gb.scalar(np.float32, "loss"), gb.banded((n,), np.int32, TB, what="pred")]
    return out + ([gb.banded((n, 2), np.float32, TB, what="logits")] if logits else [])


def _loss_bits(x):
    return np.array([x], np.float32)


@pytest.mark.parametrize("n", [1, 70])
@pytest.mark.parametrize("kind", ["rnn", "base"])
def test_train_step_and_eval_outputs(train_engines, kind, n):
    eng = train_engines(kind)
    lib, h, base = eng._lib, eng._h, kind == "base"
    feats = tsb.train_features(n, T5, 70 + n) if base else ts.train_features(n, T5, 70 + n)
    labels = np.random.default_rng(n).integers(0, 2, n).astype(np.int32)
    m, s, a = (np.ascontiguousarray(feats[k], np.float32) for k in ("means", "stds", "sanums"))
    kmer = np.ascontiguousarray(feats["kmer"], np.int32) if base else None
    kp = kmer.ctypes.data if base else None
    rows = (m.ctypes.data, s.ctypes.data, a.ctypes.data, labels.ctypes.data)
    try:
        eng.train_begin(keep_prob=0.5, seed=5, base=True)
        loss, pred = eng.train_step(m, s, a, labels, 1e-3, kmer=kmer if base else np.zeros_like(m, np.int32))
        e_loss, e_pred, e_logits = eng.train_eval(m, s, a, labels, kmer=kmer)
        eng.train_begin(keep_prob=0.5, seed=5, base=True)
        b_loss, b_pred = _train_outputs(n, False)
        rcode = gb.call(lib, "ds_train_step_base", h, n, kp, *rows, ctypes.c_float(1e-3), b_loss, b_pred)
        assert rcode == 0, lib.ds_last_error(h)
        gb.same_bytes(b_loss, _loss_bits(loss))
        gb.same_bytes(b_pred, pred)
        b_loss, b_pred, b_logits = _train_outputs(n, True)
        assert gb.call(lib, "ds_train_eval", h, n, kp, *rows, b_loss, b_pred, b_logits) == 0, lib.ds_last_error(h)
        gb.same_bytes(b_loss, _loss_bits(e_loss))
        gb.same_bytes(b_pred, e_pred)
        gb.same_bytes(b_logits, e_logits)
        b_loss, b_pred, _ = _train_outputs(n, True)
        assert gb.call(lib, "ds_train_eval", h, n, kp, *rows, b_loss, b_pred, None) == 0          # logits are optional
        gb.same_bytes(b_pred, e_pred)
        if not base:                                        # ds_train_step proper, on a run opened by ds_train_begin
            eng.train_begin(keep_prob=0.5, seed=5)
            loss, pred = eng.train_step(m, s, a, labels, 1e-3)
            eng.train_begin(keep_prob=0.5, seed=5)
            b_loss, b_pred = _train_outputs(n, False)
            assert gb.call(lib, "ds_train_step", h, n, *rows, ctypes.c_float(1e-3), b_loss, b_pred) == 0, lib.ds_last_error(h)
            gb.same_bytes(b_loss, _loss_bits(loss))
            gb.same_bytes(b_pred, pred)
    finally:
        eng.train_end()


@pytest.mark.parametrize("n", [1, 70])
def test_train_signal_step_and_eval_outputs(train_engines, n):
    eng = train_engines("signal")
    lib, h = eng._lib, eng._h
    rng = np.random.default_rng(70 + n)
    sig, labels = rng.normal(0.0, 1.0, (n, S40)).astype(np.float32), rng.integers(0, 2, n).astype(np.int32)
    try:
        eng.train_begin(keep_prob=0.5, seed=5)
        loss, pred = eng.train_step_signal(sig, labels, 1e-3)
        e_loss, e_pred, e_logits = eng.train_eval_signal(sig, labels)
        eng.train_begin(keep_prob=0.5, seed=5)
        b_loss, b_pred = _train_outputs(n, False)
        rcode = gb.call(lib, "ds_train_step_signal", h, n, sig.ctypes.data, labels.ctypes.data, ctypes.c_float(1e-3), b_loss, b_pred)
        assert rcode == 0, lib.ds_last_error(h)
        gb.same_bytes(b_loss, _loss_bits(loss))
        gb.same_bytes(b_pred, pred)
        b_loss, b_pred, b_logits = _train_outputs(n, True)
        assert gb.call(lib, "ds_train_eval_signal", h, n, sig.ctypes.data, labels.ctypes.data, b_loss, b_pred, b_logits) == 0
        gb.same_bytes(b_loss, _loss_bits(e_loss))
        gb.same_bytes(b_pred, e_pred)
        gb.same_bytes(b_logits, e_logits)
    finally:
        eng.train_end()


def _getter(lib, h, entry, name, want, dtype):
    """cap == count: the wrapper's bytes; cap == count - 1: refused, extent untouched."""
    count = int(want.size)
    out = gb.banded((count,), dtype, 1, what="%s(%s)" % (entry, name))
    assert gb.call(lib, entry, h, name.encode(), out, count) == count, lib.ds_last_error(h)
    gb.same_bytes(out, want)
    out = gb.banded((count - 1,), dtype, 1, what="%s(%s), cap one short" % (entry, name))
    assert gb.call(lib, entry, h, name.encode(), out, count - 1) == INVALID
    assert out.untouched()


def test_train_getters_at_exact_capacity_and_one_short(train_engines):
    n = 70
    eng = train_engines("base")
    feats = tsb.train_features(n, T5, 9)
    labels = np.random.default_rng(9).integers(0, 2, n).astype(np.int32)
    try:
        eng.train_begin(keep_prob=0.5, seed=5, base=True)
        eng.train_step(feats["means"], feats["stds"], feats["sanums"], labels, 1e-3, kmer=feats["kmer"])
        names = E.trainable_names(True)
        for name in (names[0], names[1], names[-1]):       # the embedding, an LSTM kernel, the last dense kernel
            _getter(eng._lib, eng._h, "ds_train_get_tensor", name, eng.train_tensor(name), np.float32)
            _getter(eng._lib, eng._h, "ds_train_get_grad", name, eng.train_grad(name), np.float32)
        for stream in ("fw_l0", "bw_l2", "fc1", "fc2"):
            _getter(eng._lib, eng._h, "ds_train_get_mask", stream, eng.train_mask(stream, n), np.uint8)
        steps, ms = gb.scalar(np.int64), gb.banded((5,), np.float64, 1)
        assert gb.call(eng._lib, "ds_get_train_times", eng._h, 0, steps, ms) == 0
        assert steps.written() and ms.written()
    finally:
        eng.train_end()
    eng = train_engines("signal")
    rng = np.random.default_rng(2)
    sig, labels = rng.normal(0.0, 1.0, (n, S40)).astype(np.float32), rng.integers(0, 2, n).astype(np.int32)
    try:
        eng.train_begin(keep_prob=0.5, seed=5)
        eng.train_step_signal(sig, labels, 1e-3)
        for tap in ("stem1", "m4.b1", "m11.b5", "feat", "logits"):
            _getter(eng._lib, eng._h, "ds_train_get_tap", tap, eng.train_tap(tap, n), np.float32)
        for stream in ("fc1", "fc2"):
            _getter(eng._lib, eng._h, "ds_train_get_mask", stream, eng.train_mask(stream, n), np.uint8)
        name = E.signal_trainable_names(S40)[0]
        _getter(eng._lib, eng._h, "ds_train_get_tensor", name, eng.train_tensor(name), np.float32)
        _getter(eng._lib, eng._h, "ds_train_get_grad", name, eng.train_grad(name), np.float32)
    finally:
        eng.train_end()


# ---- diagnostics -----------------------------------------------------------------------------------------------------------------------
def test_get_intermediate_at_and_below_the_size(engines, plain128):
    eng = engines("fp32", 1, 2)
    n = 70
    eng.run(*_args(plain128, 0, n))
    for name, shape in (("logits", (n, 2)), ("lstm_fw_l2", (n, 17, 256))):      # the second is re-laid from [T][max_batch][256]
        want = eng.intermediate(name, shape)
        out = gb.banded(shape, np.float32, B, what=name)
        assert gb.call(eng._lib, "ds_get_intermediate", eng._h, name.encode(), out, want.size) == want.size
        gb.same_bytes(out, want, name)
        out = gb.banded((want.size - 1,), np.float32, B * int(np.prod(shape[1:])), what=name + ", capacity one short")
        assert gb.call(eng._lib, "ds_get_intermediate", eng._h, name.encode(), out, want.size - 1) == INVALID
        assert out.untouched()


def _name_extents(lib, h, entry, full, tail):
    """name_cap in {1, 2, len(name), len(name) + 1}: at most name_cap bytes are written and the byte at name_cap - 1 is NUL."""
    raw = full.encode()
    for cap in (1, 2, len(raw), len(raw) + 1):
        name = gb.banded((cap,), np.uint8, 1, what="%s name, name_cap = %d" % (entry, cap))
        outs = tail()
        assert gb.call(lib, entry, h, 0, name, cap, *outs) == 0
        got = name.bytes()
        assert got[cap - 1] == 0 and got[:cap - 1].tobytes() == raw[:cap - 1]
        assert all(b.written() for b in outs)


def test_stage_and_kernel_names_stay_inside_name_cap(engines, plain128):
    eng = engines("fp32", 1, 2)
    stage, kernel = eng.stage_times()[0]["name"], eng.kernel_stats()[0]["name"]
    assert len(stage) > 2 and len(kernel) > 2
    _name_extents(eng._lib, eng._h, "ds_get_stage", stage,
                  lambda: [gb.scalar(np.int32), gb.scalar(np.float64), gb.scalar(np.int64), gb.scalar(np.float64)])
    _name_extents(eng._lib, eng._h, "ds_get_kernel_stat", kernel, lambda: [gb.scalar(np.int64), gb.scalar(np.float64), gb.scalar(np.float64)])


def test_alloc_host_writes_one_pointer():
    lib = E.load_library()
    out = gb.scalar(np.uint64, "out")
    assert gb.call(lib, "ds_alloc_host", 4096, out) == 0
    p = int(out.view[0])
    assert p != 0 and p != int.from_bytes(bytes([gb.PREFILL]) * 8, "little")
    np.ctypeslib.as_array(ctypes.cast(ctypes.c_void_p(p), ctypes.POINTER(ctypes.c_uint8)), (4096,))[:] = 1      # the block is the caller's
    assert lib.ds_free_host(p) == 0
