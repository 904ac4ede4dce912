"""ctypes binding of libdeepsignal_hip.so — the MI355X engine behind `call_mods`.

`Engine` plays the role of the reference's `(Model, tf.Session)` pair
(/root/reference/deepsignal/call_modifications.py:203-212): construct, restore weights, then
`run(...)` == `tf_sess.run([model.activation_logits, model.prediction], feed_dict)`
(call_modifications.py:168-178).

There is NO CPU fallback: if the HIP library is missing or no GPU is visible, construction raises.
"""
from __future__ import annotations

import ctypes
import os
from typing import Dict, List, Optional, Tuple

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# DS_HIP_LIBRARY: developer override (kernel A/B builds under tools/). The product path is the in-tree library; an active
# override is announced on stderr when the library is loaded and shows up in bench.py's JSON ("library_override"), so a
# variable left over from an A/B session cannot silently change what a product run or a benchmark measures.
DEFAULT_LIB_PATH = os.path.join(_HERE, "libdeepsignal_hip.so")
LIB_PATH = os.environ.get("DS_HIP_LIBRARY") or DEFAULT_LIB_PATH
LIBRARY_OVERRIDE = LIB_PATH if os.path.abspath(LIB_PATH) != os.path.abspath(DEFAULT_LIB_PATH) else None

# every symbol include/deepsignal_hip.h declares
EXPORTED_SYMBOLS = (
    "ds_create", "ds_destroy", "ds_last_error", "ds_version", "ds_load_weights", "ds_set_tensor",
    "ds_finalize_weights", "ds_forward", "ds_forward_device", "ds_sync", "ds_alloc_host", "ds_free_host",
    "ds_get_intermediate", "ds_set_profiling", "ds_num_stages", "ds_get_stage", "ds_reset_stage_times",
    "ds_set_graph", "ds_num_kernels", "ds_get_kernel_stat", "ds_submit", "ds_submit_parts", "ds_wait", "ds_num_slots",
    # scope row f1 (host I/O)
    "ds_tsv_open", "ds_tsv_close", "ds_tsv_error", "ds_tsv_next", "ds_tsv_kmer", "ds_tsv_means", "ds_tsv_stds",
    "ds_tsv_lens", "ds_tsv_signals", "ds_tsv_labels", "ds_tsv_info", "ds_tsv_info_offsets", "ds_format_rows",
    "ds_tsv_size", "ds_tsv_align", "ds_tsv_set_range", "ds_tsv_locate", "ds_tsv_parse_into",
    # scope row f3 (TF checkpoint import)
    "ds_crc32c",
    # scope row f2 on the device (fast5 feature extraction)
    "ds_extract", "ds_submit_reads", "ds_extract_reference",
    # feature rows on the device (the text half of `extract`)
    "ds_submit_rows", "ds_wait_rows", "ds_extract_rows", "ds_extract_rows_reference", "ds_format_values", "ds_get_rows_times",
    # cascaded precision (a fine handle rechecks the near-threshold sites of a coarse one)
    "ds_set_recheck", "ds_get_recheck_stats", "ds_get_recheck_times", "ds_recheck_select",
    # feature-TSV rows parsed on the device (call_mods --parse_on gpu)
    "ds_submit_text", "ds_wait_text", "ds_parse_text", "ds_parse_text_reference", "ds_get_text_stats", "ds_get_text_times",
    "ds_tsv_take_lines", "ds_tsv_data",
    # per-site modification frequency on the device (call_freq --on gpu)
    "ds_freq_locate", "ds_freq_begin", "ds_freq_parse", "ds_freq_accumulate", "ds_freq_result", "ds_freq_end",
    "ds_freq_reference", "ds_get_freq_times",
    # ... and straight from the forward's results (call_mods --freq_file)
    "ds_freq_begin_stream", "ds_freq_push", "ds_freq_keys", "ds_freq_values", "ds_freq_values_reference", "ds_get_freq_stream_times",
    # both strands of a CpG table combined on the device (combine_strands --on gpu)
    "ds_fasta_locate", "ds_combine_begin", "ds_combine_genome", "ds_combine_bitmap", "ds_combine_parse", "ds_combine_accumulate",
    "ds_combine_result", "ds_combine_end", "ds_motif_reference", "ds_combine_reference", "ds_get_combine_times",
    # call accuracy and AUROC of labelled call rows on the device (evaluate --on gpu)
    "ds_eval_locate", "ds_eval_begin", "ds_eval_parse", "ds_eval_accumulate", "ds_eval_result", "ds_eval_end", "ds_eval_reference",
    "ds_get_eval_times",
    # training step of the RNN-only model (denoise)
    "ds_train_begin", "ds_train_set_tensor", "ds_train_step", "ds_train_sync_weights", "ds_train_get_tensor", "ds_train_get_grad",
    "ds_train_get_mask", "ds_train_end", "ds_train_mask_reference", "ds_get_train_times",
    # ... with the embedding trained too, and the evaluation pass (train)
    "ds_train_begin_base", "ds_train_step_base", "ds_train_eval",
    # the signal-only model's training step (train --is_cnn yes --is_rnn no)
    "ds_train_begin_signal", "ds_train_step_signal", "ds_train_eval_signal", "ds_train_get_tap", "ds_train_mask_reference_wide",
)


class DsConfig(ctypes.Structure):
    _fields_ = [
        ("kmer_len", ctypes.c_int32), ("signal_len", ctypes.c_int32), ("class_num", ctypes.c_int32),
        ("is_cnn", ctypes.c_int32), ("is_rnn", ctypes.c_int32), ("is_base", ctypes.c_int32),
        ("device", ctypes.c_int32), ("precision", ctypes.c_int32), ("max_batch", ctypes.c_int32),
        ("reserved", ctypes.c_int32 * 7),
    ]


class DsReads(ctypes.Structure):
    """include/deepsignal_hip.h ds_reads"""
    _fields_ = [
        ("nreads", ctypes.c_int32), ("raw", ctypes.c_void_p), ("raw_off", ctypes.c_void_p), ("start", ctypes.c_void_p),
        ("length", ctypes.c_void_p), ("base", ctypes.c_void_p), ("base_off", ctypes.c_void_p), ("scaling", ctypes.c_void_p),
        ("offset", ctypes.c_void_p), ("key", ctypes.c_void_p), ("nsites", ctypes.c_int32), ("site_read", ctypes.c_void_p),
        ("site_loc", ctypes.c_void_p), ("norm", ctypes.c_int32), ("seed", ctypes.c_uint64),
    ]


class DsTrainConfig(ctypes.Structure):
    """include/deepsignal_hip.h ds_train_config"""
    _fields_ = [
        ("keep_prob", ctypes.c_float), ("pos_weight", ctypes.c_float), ("beta1", ctypes.c_float), ("beta2", ctypes.c_float),
        ("epsilon", ctypes.c_float), ("seed", ctypes.c_uint64),
    ]


NORMS = {"mad": 0, "zscore": 1}       # DS_NORM_MAD, DS_NORM_ZSCORE
_BASE_CODES = np.full(256, -1, np.int8)
for _i, _b in enumerate(b"ACGTN"):
    _BASE_CODES[_b] = _i


def base_codes(bases: str) -> np.ndarray:
    """'ACGTN' text -> int8 codes 0 .. 4 (base2code_dna); any other letter -> -1, which ds_reads validation refuses."""
    return _BASE_CODES[np.frombuffer(bases.encode("latin-1"), np.uint8)]


class ReadBatch:
    """Packed reads and the sites to extract from them: the ds_reads of ds_extract / ds_submit_reads / ds_extract_reference.

    `reads`: sequence of (raw int16[n], starts[nbases] (read_start_rel_to_raw applied), lengths[nbases], base codes int8[nbases]
    (base_codes), scaling, offset) tuples, optionally with a 7th entry, the read's subsample key (default: its index here).
    `site_read[i]` / `site_loc[i]`: the read and the index of the targeted base of site i. The arrays stay referenced here."""

    def __init__(self, reads, site_read, site_loc, norm: str = "mad", seed: int = 0):
        if norm not in NORMS:
            raise ValueError("norm must be one of %s" % (sorted(NORMS),))
        raws = [np.asarray(r[0]) for r in reads]
        if any(x.dtype != np.int16 for x in raws):
            raise ValueError("raw signals must be int16")
        self.raw = np.ascontiguousarray(np.concatenate(raws) if raws else np.zeros(0, np.int16))
        self.raw_off = np.zeros(len(raws) + 1, np.int64)
        self.raw_off[1:] = np.cumsum([len(x) for x in raws])
        self.start = np.ascontiguousarray(np.concatenate([np.asarray(r[1], np.int64) for r in reads]), np.int64)
        self.length = np.ascontiguousarray(np.concatenate([np.asarray(r[2], np.int64) for r in reads]).astype(np.int32))
        self.base = np.ascontiguousarray(np.concatenate([np.asarray(r[3], np.int8) for r in reads]), np.int8)
        self.base_off = np.zeros(len(raws) + 1, np.int64)
        self.base_off[1:] = np.cumsum([len(r[3]) for r in reads])
        self.scaling = np.array([r[4] for r in reads], np.float64)
        self.offset = np.array([r[5] for r in reads], np.float64)
        self.key = np.array([r[6] if len(r) > 6 else i for i, r in enumerate(reads)], np.uint64)
        self.site_read = np.ascontiguousarray(site_read, np.int32)
        self.site_loc = np.ascontiguousarray(site_loc, np.int32)
        self.nsites = int(self.site_read.shape[0])
        self.desc = DsReads(len(raws), self.raw.ctypes.data, self.raw_off.ctypes.data, self.start.ctypes.data,
                            self.length.ctypes.data, self.base.ctypes.data, self.base_off.ctypes.data, self.scaling.ctypes.data,
                            self.offset.ctypes.data, self.key.ctypes.data, self.nsites, self.site_read.ctypes.data,
                            self.site_loc.ctypes.data, NORMS[norm], seed)


def _feature_arrays(n: int, kmer_len: int, signal_len: int):
    return {"kmer": np.empty((n, kmer_len), np.int32), "means": np.empty((n, kmer_len), np.float32),
            "stds": np.empty((n, kmer_len), np.float32), "sanums": np.empty((n, kmer_len), np.float32),
            "signals": np.empty((n, signal_len), np.float32)}


def extract_reference(batch: ReadBatch, kmer_len: int = 17, signal_len: int = 360) -> Dict[str, np.ndarray]:
    """ds_extract_reference: the device route's features computed on the CPU from the same arithmetic. A checker for the
    tests (no GPU needed), not a fall-back: inference has no CPU path."""
    lib = load_library()
    out = _feature_arrays(batch.nsites, kmer_len, signal_len)
    rc = lib.ds_extract_reference(ctypes.byref(batch.desc), kmer_len, signal_len,
                                  *(out[k].ctypes.data for k in ("kmer", "means", "stds", "sanums", "signals")))
    if rc != 0:
        raise RuntimeError("ds_extract_reference failed (%d): %s" % (rc, lib.ds_last_error(None).decode()))
    return out


def pack_info(info_rows):
    """The six leading columns of each row (bytes, tab-joined, no newline) -> (uint8 blob, int64 offsets[n + 1]): the info /
    info_off layout of ds_format_rows and the rows entry points."""
    off = np.zeros(len(info_rows) + 1, np.int64)
    off[1:] = np.cumsum([len(r) for r in info_rows])
    return np.frombuffer(b"".join(info_rows), np.uint8), off


def _rows_call(call, nsites: int, buf: Optional[np.ndarray] = None):
    """Run call(out pointer, capacity, row_off pointer) -> bytes written or -(bytes needed), growing the buffer when asked."""
    if buf is None:
        buf = np.empty(max(4096, nsites * 4096), np.uint8)
    row_off = np.empty(nsites + 1, np.int64)
    got = int(call(buf.ctypes.data, buf.size, row_off.ctypes.data))
    if got < -5:                    # -(bytes needed): a row is longer than that; the error codes are -1 .. -5
        buf = np.empty(-got, np.uint8)
        got = int(call(buf.ctypes.data, buf.size, row_off.ctypes.data))
    return got, buf, row_off


def extract_rows_reference(batch: ReadBatch, info, info_off, label: int, kmer_len: int = 17, signal_len: int = 360):
    """ds_extract_rows_reference: the feature rows of `batch` on the CPU -> (bytes, int64 row offsets[nsites + 1]). A checker
    for the tests, as extract_reference."""
    lib = load_library()
    info = np.ascontiguousarray(info, np.uint8)
    info_off = np.ascontiguousarray(info_off, np.int64)
    got, buf, row_off = _rows_call(lambda o, c, ro: lib.ds_extract_rows_reference(
        ctypes.byref(batch.desc), kmer_len, signal_len, info.ctypes.data, info_off.ctypes.data, label, o, c, ro), batch.nsites)
    if got < 0:
        raise RuntimeError("ds_extract_rows_reference failed (%d): %s" % (got, lib.ds_last_error(None).decode()))
    return buf[:got].tobytes(), row_off


def format_values(values, engine: Optional["Engine"] = None, cap: Optional[int] = None) -> bytes:
    """ds_format_values: the comma-joined row text of float64 values, by the host code (engine None) or the device routine.
    cap: the output capacity to offer (default: enough); a short one raises with the bytes needed in the message."""
    lib = load_library()
    v = np.ascontiguousarray(values, np.float64)
    buf = np.empty(28 * max(1, v.size) if cap is None else cap, np.uint8)
    h = engine._h if engine is not None else None
    got = int(lib.ds_format_values(h, v.size, v.ctypes.data, buf.ctypes.data, buf.size))
    if got < 0:
        raise RuntimeError("ds_format_values failed (%d)%s" % (got, ": " + lib.ds_last_error(h).decode() if got >= -5 else
                                                               ": %d bytes needed" % -got))
    return buf[:got].tobytes()


TEXT_ROW_OK, TEXT_ROW_HOST = 0, 1      # DS_TEXT_ROW_*: per-row status of the device's TSV parser


class TextRowError(ValueError):
    """wait_text: a row the device left to the host parser is malformed; `row` = its index within the ticket."""

    def __init__(self, row: int, message: str):
        ValueError.__init__(self, message)
        self.row = row


def _text_args(text, begin, end):
    """(keep-alive object, address) of a text buffer given as bytes / a uint8 array / a raw address, and the int64 span arrays."""
    begin = np.ascontiguousarray(begin, np.int64)
    end = np.ascontiguousarray(end, np.int64)
    if begin.ndim != 1 or begin.shape != end.shape:
        raise ValueError("begin / end must be 1-d arrays of one length")
    if isinstance(text, (int, np.integer)):
        return None, int(text), begin, end
    if isinstance(text, (bytes, bytearray)):
        text = np.frombuffer(text, np.uint8)
    text = np.ascontiguousarray(text, np.uint8)
    if begin.size and (int(begin.min()) < 0 or int(end.max()) > text.size or bool((end < begin).any())):
        raise ValueError("row spans outside the text")
    return text, text.ctypes.data, begin, end


def _batch_rows_args(text, begin, end, chrom, flags, batch_rows: int):
    """The arguments of freq_parse / combine_parse: (keep-alive object, address, begin, end, chrom, flags) of a batch's rows."""
    keep, addr, begin, end = _text_args(text, begin, end)
    chrom = np.ascontiguousarray(chrom, np.int32)
    flags = np.ascontiguousarray(flags, np.uint8)
    n = int(begin.size)
    if chrom.shape != (n,) or flags.shape != (n,):
        raise ValueError("chrom / flags must have one entry per row")
    if not 1 <= n <= batch_rows:
        raise ValueError("a batch holds 1 .. batch_rows rows of an open run")
    if n > 1 and bool((begin[1:] < end[:-1]).any()):
        raise ValueError("the rows of a batch must be ascending and disjoint")
    return keep, addr, begin, end, chrom, flags


def _check_override_rows(rows: np.ndarray, n: int) -> None:
    """freq_accumulate / combine_accumulate: the caller's rows are ascending indices of a batch of n rows."""
    if rows.size and (int(rows.min()) < 0 or int(rows.max()) >= n or bool((np.diff(rows) <= 0).any())):
        raise ValueError("override rows must be ascending indices of the batch")


def _text_arrays(n: int, kmer_len: int, signal_len: int):
    out = _feature_arrays(n, kmer_len, signal_len)
    out["lens"] = out.pop("sanums")
    out.update(labels=np.empty(n, np.int32), info_len=np.empty(n, np.int32), status=np.empty(n, np.int32))
    return out


_TEXT_ORDER = ("kmer", "means", "stds", "lens", "signals", "labels", "info_len", "status")


def parse_text_reference(text, begin, end, kmer_len: int = 17, signal_len: int = 360) -> Dict[str, np.ndarray]:
    """ds_parse_text_reference: the device's TSV row parser on the CPU, from the same token routines -> kmer, means, stds, lens,
    signals, labels, info_len, status (TEXT_ROW_OK / TEXT_ROW_HOST; the values of a HOST row are unspecified). A checker for
    the tests (no GPU needed), not a fall-back."""
    lib = load_library()
    keep, addr, begin, end = _text_args(text, begin, end)
    out = _text_arrays(begin.size, kmer_len, signal_len)
    rc = lib.ds_parse_text_reference(kmer_len, signal_len, addr, begin.size, begin.ctypes.data, end.ctypes.data,
                                     *(out[k].ctypes.data for k in _TEXT_ORDER))
    if rc != 0:
        raise RuntimeError("ds_parse_text_reference failed (%d): %s" % (rc, lib.ds_last_error(None).decode()))
    return out


FREQ_ROW_GIVEN = 2                     # DS_FREQ_ROW_GIVEN: freq_reference takes this row's values from the caller
FREQ_POS_LIMIT, FREQ_CHROM_LIMIT = 1 << 40, 1 << 23      # a site key is chrom_id << 40 | pos
FREQ_MAX_BATCH, FREQ_MAX_ROWS = 1 << 24, 1 << 30


class FreqNoMemory(RuntimeError):
    """freq_begin: the site table or the batch buffers do not fit the device."""


class _TableRun:
    """What Engine keeps of one table route's run (freq, combine, eval): batch = the batch_rows of the open run (0: none), pending =
    the rows parsed or pushed and not yet accumulated (-1: none), and the route's extras."""

    def __init__(self, **extras):
        self.begin(0, **extras)

    def begin(self, batch_rows: int, **extras) -> None:
        self.batch, self.pending = batch_rows, -1
        self.__dict__.update(extras)

    def end(self) -> None:
        self.begin(0)


def _run_sizes(total_rows, batch_rows, min_total: int = 1) -> Tuple[int, int]:
    """The total_rows / batch_rows of a *_begin, as ints in their ranges."""
    total_rows, batch_rows = int(total_rows), int(batch_rows)
    if not min_total <= total_rows <= FREQ_MAX_ROWS:
        raise ValueError("total_rows must be in [%d, 2^30]" % min_total)
    if not 1 <= batch_rows <= FREQ_MAX_BATCH:
        raise ValueError("batch_rows must be in [1, 2^24]")
    return total_rows, batch_rows


def freq_locate(text):
    """ds_freq_locate: the rows of a call_mods result buffer (bytes, or a uint8 array such as a memory map) -> (row_begin int64[n],
    row_end int64[n], chrom int32[n], flags uint8[n], names): chrom = the row's chromosome id, an index into `names` (bytes, in
    first-appearance order); flags 1 = a row Python strips or decodes differently from its raw bytes (chrom -1)."""
    lib = load_library()
    if isinstance(text, (bytes, bytearray)):
        text = np.frombuffer(text, np.uint8)
    text = np.ascontiguousarray(text, np.uint8)
    if text.ndim != 1:
        raise ValueError("text must be a flat byte buffer")
    nb, nn = ctypes.c_int64(), ctypes.c_int32()
    cap, names_cap = text.size // 32 + 1, 1 << 16      # a result row is ~100 bytes: one pass over the buffer in the common case
    while True:
        begin, end = np.empty(cap, np.int64), np.empty(cap, np.int64)
        chrom, flags = np.empty(cap, np.int32), np.empty(cap, np.uint8)
        names = np.empty(names_cap, np.uint8)
        n = int(lib.ds_freq_locate(text.ctypes.data if text.size else None, text.size, cap, begin.ctypes.data, end.ctypes.data,
                                   chrom.ctypes.data, flags.ctypes.data, names.ctypes.data, names_cap, ctypes.byref(nb),
                                   ctypes.byref(nn)))
        if n < 0:
            raise RuntimeError("ds_freq_locate failed (%d)" % n)
        if n <= cap and nb.value <= names_cap:
            blob = names[:nb.value].tobytes()
            return begin[:n], end[:n], chrom[:n], flags[:n], blob.split(b"\n")[:nn.value]
        cap, names_cap = max(cap, n), max(names_cap, int(nb.value))


_FREQ_SITE_FIELDS = (("first_row", np.int64), ("chrom", np.int32), ("pos", np.int64), ("sum0", np.float64), ("sum1", np.float64),
                     ("met", np.int32), ("unmet", np.int32))


def freq_reference(text, begin, end, chrom, flags, prob_cf: float = 0.0, given=None) -> Dict[str, np.ndarray]:
    """ds_freq_reference: the device route's aggregation on the CPU from the same row routine, one pass in row order. A checker
    for the tests (no GPU needed), not a fall-back. `given`: {row index: (chrom id, pos, p0, p1, met)} for rows whose values
    the caller supplies (what the device route does with the rows it leaves to Python). Returns the per-row status / pos / p0 /
    p1 / met and the sites in the order of their first used row (first_row, chrom, pos, sum0, sum1, met, unmet), plus `used`."""
    lib = load_library()
    keep, addr, begin, end = _text_args(text, begin, end)
    n = int(begin.size)
    chrom = np.array(chrom, np.int32)              # a copy: the given rows' ids go in
    flags = np.ascontiguousarray(flags, np.uint8)
    if chrom.shape != (n,) or flags.shape != (n,):
        raise ValueError("chrom / flags must have one entry per row")
    status = np.zeros(n, np.int32)
    pos, p0, p1, met = np.zeros(n, np.int64), np.zeros(n, np.float64), np.zeros(n, np.float64), np.zeros(n, np.int32)
    for i, (c, q, a, b, m) in (given or {}).items():
        status[i], chrom[i], pos[i], p0[i], p1[i], met[i] = FREQ_ROW_GIVEN, c, q, a, b, m
    sites = {k: np.empty(n, dt) for k, dt in _FREQ_SITE_FIELDS}
    used = ctypes.c_int64()
    got = int(lib.ds_freq_reference(addr, n, begin.ctypes.data, end.ctypes.data, chrom.ctypes.data, flags.ctypes.data, float(prob_cf),
                                    status.ctypes.data, pos.ctypes.data, p0.ctypes.data, p1.ctypes.data, met.ctypes.data, n,
                                    *(sites[k].ctypes.data for k, _ in _FREQ_SITE_FIELDS), ctypes.byref(used)))
    if got < 0:
        raise RuntimeError("ds_freq_reference failed (%d): %s" % (got, lib.ds_last_error(None).decode()))
    out = {k: v[:got] for k, v in sites.items()}
    out.update(status=status, row_pos=pos, row_p0=p0, row_p1=p1, row_met=met, used=int(used.value))
    return out


def freq_keys(info, info_off):
    """ds_freq_keys: the site keys of n sampleinfo strings (info: a flat byte buffer, info_off int64[n + 1]) -> (chrom int32[n],
    pos int64[n], flags uint8[n], names): chrom indexes `names` (bytes, first-appearance order within this call); flags 1 = a row to
    format and let Python read (chrom -1)."""
    lib = load_library()
    info = np.ascontiguousarray(info, np.uint8)
    off = np.ascontiguousarray(info_off, np.int64)
    n = int(off.size) - 1
    if info.ndim != 1 or off.ndim != 1 or n < 0:
        raise ValueError("info must be a flat byte buffer and info_off hold n + 1 offsets")
    if n and (int(off[0]) < 0 or int(off[-1]) > info.size or bool((np.diff(off) < 0).any())):
        raise ValueError("info_off must ascend inside info")
    chrom, pos, flags = np.empty(n, np.int32), np.empty(n, np.int64), np.empty(n, np.uint8)
    nb, nn = ctypes.c_int64(), ctypes.c_int32()
    names_cap = 1 << 12
    while True:
        names = np.empty(names_cap, np.uint8)
        got = int(lib.ds_freq_keys(n, info.ctypes.data if info.size else None, off.ctypes.data, chrom.ctypes.data, pos.ctypes.data,
                                   flags.ctypes.data, names.ctypes.data, names_cap, ctypes.byref(nb), ctypes.byref(nn)))
        if got != n:
            raise RuntimeError("ds_freq_keys failed (%d)" % got)
        if nb.value <= names_cap:
            return chrom, pos, flags, names[:nb.value].tobytes().split(b"\n")[:nn.value]
        names_cap = int(nb.value)


def _act_rows(act):
    act = np.ascontiguousarray(act, np.float32)
    if act.ndim != 2 or act.shape[1] < 2:
        raise ValueError("act must be [n, class_num >= 2] float32")
    return act


def freq_values_reference(act) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """ds_freq_values_reference: per act row the two doubles call_freq reads from the row call_mods prints for it, and the status
    (TEXT_ROW_OK / TEXT_ROW_HOST), by the routine freq_values_kernel runs -- on the CPU. A checker for the tests, not a fall-back."""
    lib = load_library()
    act = _act_rows(act)
    n = act.shape[0]
    p0, p1, status = np.zeros(n, np.float64), np.zeros(n, np.float64), np.zeros(n, np.int32)
    rc = lib.ds_freq_values_reference(n, act.ctypes.data, act.shape[1], p0.ctypes.data, p1.ctypes.data, status.ctypes.data)
    if rc != 0:
        raise RuntimeError("ds_freq_values_reference failed (%d)" % rc)
    return p0, p1, status


EVAL_BARE_CR = 1                       # DS_EVAL_BARE_CR: eval_locate's word on the buffer
EVAL_ROW_GIVEN = 2                     # DS_EVAL_ROW_GIVEN: eval_reference takes this row's values from the caller
EVAL_SET_SAMPLE, EVAL_SET_ALL, EVAL_TRUTH = 1, 2, 4      # DS_EVAL_SET_* / DS_EVAL_TRUTH: the bits of a row's byte
EVAL_MAX_CF = 32


def eval_locate(text):
    """ds_eval_locate: the rows of a call_mods result buffer (bytes, or a uint8 array such as a memory map) for a reader that cuts
    them with line.rstrip().split() -> (row_begin int64[n], row_end int64[n], flags uint8[n], file_flags): flags 1 = a row Python
    tokenises or decodes differently from fields between runs of space or tab; file_flags & EVAL_BARE_CR = a bare carriage return."""
    lib = load_library()
    if isinstance(text, (bytes, bytearray)):
        text = np.frombuffer(text, np.uint8)
    text = np.ascontiguousarray(text, np.uint8)
    if text.ndim != 1:
        raise ValueError("text must be a flat byte buffer")
    ff = ctypes.c_int32()
    cap = text.size // 32 + 1
    while True:
        begin, end, flags = np.empty(cap, np.int64), np.empty(cap, np.int64), np.empty(cap, np.uint8)
        n = int(lib.ds_eval_locate(text.ctypes.data if text.size else None, text.size, cap, begin.ctypes.data, end.ctypes.data,
                                   flags.ctypes.data, ctypes.byref(ff)))
        if n < 0:
            raise RuntimeError("ds_eval_locate failed (%d)" % n)
        if n <= cap:
            return begin[:n], end[:n], flags[:n], int(ff.value)
        cap = n


def _eval_cutoffs(cf) -> np.ndarray:
    cf = np.ascontiguousarray(cf, np.float64)
    if cf.ndim != 1 or not 1 <= cf.size <= EVAL_MAX_CF:
        raise ValueError("1 .. 32 cut-offs")
    return cf


def _eval_mask(mask, n: int) -> np.ndarray:
    mask = np.ascontiguousarray(mask, np.uint8)
    if mask.shape != (n,):
        raise ValueError("mask must have one byte per row")
    if n and int(mask.max()) > (EVAL_SET_SAMPLE | EVAL_SET_ALL | EVAL_TRUTH):
        raise ValueError("a row's byte holds bits 0 .. 2 only")
    return mask


def _eval_result(ncf: int):
    return np.zeros((2, 4 + 2 * ncf), np.int64), np.zeros(2, np.uint64), np.zeros(2, np.int64), np.zeros(2, np.int64)


def eval_reference(text, begin, end, flags, mask, cf, given=None) -> Dict[str, np.ndarray]:
    """ds_eval_reference: the device route's counts on the CPU from the same row routines, one pass. A checker for the tests (no
    GPU needed), not a fall-back. mask: a byte per row (EVAL_SET_SAMPLE | EVAL_SET_ALL | EVAL_TRUTH). `given`: {row index: (p0, p1,
    called)} for rows whose values the caller supplies. Returns the per-row status / p0 / p1 / called, counts int64[2, 4 + 2 ncf]
    (tp, fp, tn, fn, called per cut-off, correct per cut-off; set 0 the sample, set 1 all) and per set u2 / p / n."""
    lib = load_library()
    keep, addr, begin, end = _text_args(text, begin, end)
    n = int(begin.size)
    flags = np.ascontiguousarray(flags, np.uint8)
    if flags.shape != (n,):
        raise ValueError("flags must have one entry per row")
    mask, cf = _eval_mask(mask, n), _eval_cutoffs(cf)
    status = np.zeros(n, np.int32)
    p0, p1, called = np.zeros(n, np.float64), np.zeros(n, np.float64), np.zeros(n, np.int32)
    for i, (a, b, c) in (given or {}).items():
        status[i], p0[i], p1[i], called[i] = EVAL_ROW_GIVEN, a, b, int(c != 0)
    counts, u2, pn, nn = _eval_result(cf.size)
    rc = lib.ds_eval_reference(addr, n, begin.ctypes.data, end.ctypes.data, flags.ctypes.data, mask.ctypes.data, cf.size, cf.ctypes.data,
                               status.ctypes.data, p0.ctypes.data, p1.ctypes.data, called.ctypes.data, counts.ctypes.data, u2.ctypes.data,
                               pn.ctypes.data, nn.ctypes.data)
    if rc != 0:
        raise RuntimeError("ds_eval_reference failed (%d): %s" % (rc, lib.ds_last_error(None).decode()))
    return dict(status=status, p0=p0, p1=p1, called=called, counts=counts, u2=[int(v) for v in u2], p=[int(v) for v in pn],
                n=[int(v) for v in nn])


COMBINE_TABLE, COMBINE_BED = 0, 1      # DS_COMBINE_TABLE / DS_COMBINE_BED: the form of the rows
COMBINE_ROW_SKIP, COMBINE_ROW_GIVEN, COMBINE_ROW_GIVEN_SKIP = 2, 3, 4      # DS_COMBINE_ROW_*
COMBINE_COUNT_LIMIT = 1 << 32          # a count the caller gives for a row stays below this in magnitude
COMBINE_MAX_CHUNK = 1 << 30            # bytes one genome chunk may span
FASTA_NON_ASCII, FASTA_BARE_CR = 1, 2  # ds_fasta_locate's flags


def fasta_locate(text) -> Dict[str, np.ndarray]:
    """ds_fasta_locate: the sequence lines and records of a FASTA buffer (bytes, or a uint8 array such as a memory map) ->
    line_begin / line_end (stripped byte spans), line_rec, line_off (offset inside the record's sequence), name_begin / name_end,
    rec_len (record 0 = what lies in front of the first header), and `flags` (FASTA_NON_ASCII | FASTA_BARE_CR)."""
    lib = load_library()
    if isinstance(text, (bytes, bytearray)):
        text = np.frombuffer(text, np.uint8)
    text = np.ascontiguousarray(text, np.uint8)
    if text.ndim != 1:
        raise ValueError("text must be a flat byte buffer")
    nrec, flags = ctypes.c_int64(), ctypes.c_int32()
    cap, cap_recs = text.size // 48 + 16, 1 << 10
    while True:
        lines = {"line_begin": np.empty(cap, np.int64), "line_end": np.empty(cap, np.int64), "line_rec": np.empty(cap, np.int32),
                 "line_off": np.empty(cap, np.int64)}
        recs = {"name_begin": np.empty(cap_recs, np.int64), "name_end": np.empty(cap_recs, np.int64), "rec_len": np.empty(cap_recs, np.int64)}
        n = int(lib.ds_fasta_locate(text.ctypes.data if text.size else None, text.size, cap, *(v.ctypes.data for v in lines.values()),
                                    cap_recs, *(v.ctypes.data for v in recs.values()), ctypes.byref(nrec), ctypes.byref(flags)))
        if n < 0:
            raise RuntimeError("ds_fasta_locate failed (%d)" % n)
        if n <= cap and nrec.value <= cap_recs:
            out = {k: v[:n] for k, v in lines.items()}
            out.update({k: v[:nrec.value] for k, v in recs.items()})
            out["flags"] = int(flags.value)
            return out
        cap, cap_recs = max(cap, n), max(cap_recs, int(nrec.value))


def _segment_args(text, seg_begin, seg_end, seg_bit, seg_carry):
    keep, addr, seg_begin, seg_end = _text_args(text, seg_begin, seg_end)
    seg_bit = np.ascontiguousarray(seg_bit, np.int64)
    seg_carry = np.ascontiguousarray(seg_carry, np.uint8)
    if seg_bit.shape != seg_begin.shape or seg_carry.shape != seg_begin.shape:
        raise ValueError("seg_bit / seg_carry must have one entry per segment")
    return keep, addr, seg_begin, seg_end, seg_bit, seg_carry


def motif_reference(text, seg_begin, seg_end, seg_bit, seg_carry, nbits: int, bitmap: Optional[np.ndarray] = None) -> np.ndarray:
    """ds_motif_reference: the genome scan of motif_bitmap_kernel on the CPU, from the same routine -> the bitmap, uint32[(nbits + 31)
    // 32] (ORed into `bitmap` when given). A checker for the tests (no GPU needed), not a fall-back."""
    lib = load_library()
    keep, addr, seg_begin, seg_end, seg_bit, seg_carry = _segment_args(text, seg_begin, seg_end, seg_bit, seg_carry)
    if bitmap is None:
        bitmap = np.zeros((int(nbits) + 31) // 32, np.uint32)
    if bitmap.dtype != np.uint32 or bitmap.size < (int(nbits) + 31) // 32 or not bitmap.flags.c_contiguous:
        raise ValueError("bitmap must be a contiguous uint32 array of (nbits + 31) // 32 words")
    rc = lib.ds_motif_reference(addr, seg_begin.size, seg_begin.ctypes.data, seg_end.ctypes.data, seg_bit.ctypes.data, seg_carry.ctypes.data,
                                int(nbits), bitmap.ctypes.data if bitmap.size else None)
    if rc != 0:
        raise RuntimeError("ds_motif_reference failed (%d): %s" % (rc, lib.ds_last_error(None).decode()))
    return bitmap


_COMBINE_ROW_FIELDS = (("pos", np.int64), ("plus", np.int32), ("a", np.float64), ("b", np.float64), ("met", np.int64), ("unmet", np.int64),
                       ("cov", np.int64))
_COMBINE_SITE_FIELDS = (("chrom", np.int32), ("pos", np.int64), ("sum0", np.float64), ("sum1", np.float64), ("met", np.int64),
                        ("unmet", np.int64), ("cov", np.int64), ("last_plus", np.int64))


def combine_reference(form: int, text, begin, end, chrom, flags, rec_len, bitmap, given=None, sites: bool = True) -> Dict[str, np.ndarray]:
    """ds_combine_reference: the device route's row grammar and aggregation on the CPU from the same routines, one pass in row order.
    A checker for the tests (no GPU needed), not a fall-back. `given`: {row index: None (the caller found the key to be no CG) or
    (record, pos, plus, a, b, met, unmet, cov)} for the rows whose values the caller supplies. Returns the per-row status and values
    (row_*) and, with `sites`, the sites in the order of their first row (chrom, pos, sum0, sum1, met, unmet, cov, last_plus)."""
    lib = load_library()
    keep, addr, begin, end = _text_args(text, begin, end)
    n = int(begin.size)
    chrom = np.array(chrom, np.int32)              # a copy: the given rows' records go in
    flags = np.ascontiguousarray(flags, np.uint8)
    rec_len = np.ascontiguousarray(rec_len, np.int64)
    bitmap = np.ascontiguousarray(bitmap, np.uint32)
    if chrom.shape != (n,) or flags.shape != (n,):
        raise ValueError("chrom / flags must have one entry per row")
    if bitmap.size < (int(rec_len.sum()) + 31) // 32:
        raise ValueError("the bitmap is shorter than the records")
    if bitmap.size == 0:
        bitmap = np.zeros(1, np.uint32)
    status = np.zeros(n, np.int32)
    rows = {k: np.zeros(n, dt) for k, dt in _COMBINE_ROW_FIELDS}
    for i, v in (given or {}).items():
        if v is None:
            status[i] = COMBINE_ROW_GIVEN_SKIP
        else:
            status[i], chrom[i] = COMBINE_ROW_GIVEN, v[0]
            for (k, _), x in zip(_COMBINE_ROW_FIELDS, v[1:]):
                rows[k][i] = x
    cap = n if sites else 0
    out = {k: np.empty(cap, dt) for k, dt in _COMBINE_SITE_FIELDS}
    got = int(lib.ds_combine_reference(int(form), addr, n, begin.ctypes.data, end.ctypes.data, chrom.ctypes.data, flags.ctypes.data,
                                       rec_len.size, rec_len.ctypes.data, bitmap.ctypes.data, status.ctypes.data,
                                       *(rows[k].ctypes.data for k, _ in _COMBINE_ROW_FIELDS), cap,
                                       *(out[k].ctypes.data for k, _ in _COMBINE_SITE_FIELDS)))
    if got < 0:
        raise RuntimeError("ds_combine_reference failed (%d): %s" % (got, lib.ds_last_error(None).decode()))
    out = {k: v[:got] for k, v in out.items()}
    out.update({"row_" + k: v for k, v in rows.items()})
    out.update(status=status, row_chrom=chrom)
    return out


# ds_config.precision (include/deepsignal_hip.h): "bf16" = bf16 conv + FC operands with fp32 accumulation, fp32 BiLSTM;
# "bf16_all" = also bf16 h / weight operands in the LSTM matmuls (fp32 accumulate, gates, cell state)
PRECISIONS = {"fp32": 0, "bf16": 1, "bf16_all": 2, "bf16x3": 3, "fp16x2": 4}
TUNE_NO_FUSED, TUNE_SERIAL, TUNE_DEBUG_STAMPS, TUNE_NO_FOLD_FC, TUNE_NO_CHAIN, TUNE_SHARED_EVENT_STREAM, TUNE_SPLIT_DENSE_NARROW, TUNE_NO_LSTM_XPROJ, TUNE_LSTM_XPROJ_ALL = 1, 2, 4, 8, 16, 32, 64, 128, 256     # ds_config.reserved[2]
LSTM_TILINGS = {"auto": 0, "narrow": 1, "wide": 2, "lds1": 3, "lds2": 4, "wide8": 5}     # ds_config.reserved[3]

_lib: Optional[ctypes.CDLL] = None


def _share_hip_runtime_with_torch() -> None:
    """One HIP runtime per process. PyTorch-ROCm wheels bundle their own libamdhip64.so (SONAME
    libamdhip64.so.7) and ask for it by file name, so if this library pulls in /opt/rocm's copy first, a later
    `import torch` loads a SECOND runtime that cannot see the GPU ("No HIP GPUs are available"). Mapping
    torch's copy first (no torch import needed) lets both resolve to the same runtime in either import order.
    Processes without torch installed simply use the system ROCm runtime."""
    import importlib.util
    import sys
    if "torch" in sys.modules:
        return
    try:
        spec = importlib.util.find_spec("torch")
    except (ImportError, ValueError):
        spec = None
    if spec is None or not spec.submodule_search_locations:
        return
    cand = os.path.join(list(spec.submodule_search_locations)[0], "lib", "libamdhip64.so")
    if os.path.exists(cand):
        try:
            ctypes.CDLL(cand, mode=ctypes.RTLD_GLOBAL)
        except OSError:
            pass


def load_library() -> ctypes.CDLL:
    """Load the in-tree HIP library; raise (never fall back) when it is absent."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            "%s not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(or `make -C deepsignal_amd/csrc`). There is no CPU fallback." % LIB_PATH)
    _share_hip_runtime_with_torch()
    if LIBRARY_OVERRIDE:
        import sys
        print("deepsignal_amd: DS_HIP_LIBRARY is set -- loading %s instead of the in-tree library" % LIBRARY_OVERRIDE, file=sys.stderr)
    lib = ctypes.CDLL(LIB_PATH)
    vp, i32, i64 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64
    lib.ds_create.argtypes = [ctypes.POINTER(DsConfig), ctypes.POINTER(vp)]
    lib.ds_create.restype = ctypes.c_int
    lib.ds_destroy.argtypes = [vp]
    lib.ds_destroy.restype = None
    lib.ds_last_error.argtypes = [vp]
    lib.ds_last_error.restype = ctypes.c_char_p
    lib.ds_version.restype = ctypes.c_char_p
    lib.ds_load_weights.argtypes = [vp, ctypes.c_char_p]
    lib.ds_set_tensor.argtypes = [vp, ctypes.c_char_p, vp, ctypes.POINTER(i64), i32]
    lib.ds_finalize_weights.argtypes = [vp]
    lib.ds_forward.argtypes = [vp, i32, vp, vp, vp, vp, vp, vp, vp]
    lib.ds_forward_device.argtypes = [vp, i32, vp, vp, vp, vp, vp, vp, vp]
    lib.ds_sync.argtypes = [vp]
    lib.ds_submit.argtypes = [vp, i32, vp, vp, vp, vp, vp, ctypes.POINTER(i32)]
    lib.ds_submit_parts.argtypes = [vp, i32, vp, vp, vp, vp, vp, vp, ctypes.POINTER(i32)]
    lib.ds_wait.argtypes = [vp, i32, vp, vp]
    lib.ds_num_slots.argtypes = [vp]
    lib.ds_alloc_host.argtypes = [ctypes.c_size_t, ctypes.POINTER(vp)]
    lib.ds_free_host.argtypes = [vp]
    lib.ds_get_intermediate.argtypes = [vp, ctypes.c_char_p, vp, i64]
    lib.ds_get_intermediate.restype = i64
    lib.ds_set_profiling.argtypes = [vp, i32]
    lib.ds_num_stages.argtypes = [vp]
    lib.ds_get_stage.argtypes = [vp, i32, ctypes.c_char_p, i32, ctypes.POINTER(i32), ctypes.POINTER(ctypes.c_double),
                                 ctypes.POINTER(i64), ctypes.POINTER(ctypes.c_double)]
    lib.ds_reset_stage_times.argtypes = [vp]
    lib.ds_set_graph.argtypes = [vp, i32]
    lib.ds_num_kernels.argtypes = [vp]
    lib.ds_extract.argtypes = [vp, ctypes.POINTER(DsReads), vp, vp, vp, vp, vp]
    lib.ds_submit_reads.argtypes = [vp, ctypes.POINTER(DsReads), ctypes.POINTER(i32)]
    lib.ds_extract_reference.argtypes = [ctypes.POINTER(DsReads), i32, i32, vp, vp, vp, vp, vp]
    lib.ds_submit_rows.argtypes = [vp, ctypes.POINTER(DsReads), vp, vp, i32, ctypes.POINTER(i32)]
    lib.ds_wait_rows.argtypes = [vp, i32, vp, i64, vp]
    lib.ds_wait_rows.restype = i64
    lib.ds_extract_rows.argtypes = [vp, ctypes.POINTER(DsReads), vp, vp, i32, vp, i64, vp]
    lib.ds_extract_rows.restype = i64
    lib.ds_extract_rows_reference.argtypes = [ctypes.POINTER(DsReads), i32, i32, vp, vp, i32, vp, i64, vp]
    lib.ds_extract_rows_reference.restype = i64
    lib.ds_format_values.argtypes = [vp, i64, vp, vp, i64]
    lib.ds_format_values.restype = i64
    lib.ds_get_rows_times.argtypes = [vp, i32, ctypes.POINTER(i64), ctypes.POINTER(ctypes.c_double)]
    lib.ds_set_recheck.argtypes = [vp, vp, ctypes.c_float]
    lib.ds_set_recheck.restype = ctypes.c_int
    lib.ds_get_recheck_stats.argtypes = [vp, ctypes.POINTER(i64), ctypes.POINTER(i64), ctypes.POINTER(i64)]
    lib.ds_get_recheck_stats.restype = ctypes.c_int
    lib.ds_get_recheck_times.argtypes = [vp, i32, ctypes.POINTER(i64), ctypes.POINTER(ctypes.c_double)]
    lib.ds_recheck_select.argtypes = [vp, i32, vp, ctypes.c_float, ctypes.POINTER(i32), vp]
    lib.ds_get_kernel_stat.argtypes = [vp, i32, ctypes.c_char_p, i32, ctypes.POINTER(i64),
                                       ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_double)]
    lib.ds_submit_text.argtypes = [vp, vp, i32, vp, vp, ctypes.POINTER(i32)]
    lib.ds_wait_text.argtypes = [vp, i32, vp, vp, vp, vp, vp, i64, vp]
    lib.ds_parse_text.argtypes = [vp, vp, i32, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp]
    lib.ds_parse_text_reference.argtypes = [i32, i32, vp, i32, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp]
    lib.ds_get_text_stats.argtypes = [vp, ctypes.POINTER(i64), ctypes.POINTER(i64)]
    lib.ds_get_text_times.argtypes = [vp, i32, ctypes.POINTER(i64), ctypes.POINTER(ctypes.c_double)]
    f64 = ctypes.c_double
    lib.ds_freq_locate.argtypes = [vp, i64, i64, vp, vp, vp, vp, vp, i64, ctypes.POINTER(i64), ctypes.POINTER(i32)]
    lib.ds_freq_locate.restype = i64
    lib.ds_freq_begin.argtypes = [vp, i64, i32, f64]
    lib.ds_freq_parse.argtypes = [vp, vp, i32, vp, vp, vp, vp, vp]
    lib.ds_freq_accumulate.argtypes = [vp, i32, vp, vp, vp, vp, vp, vp]
    lib.ds_freq_result.argtypes = [vp, i64, vp, vp, vp, vp, vp, vp, vp, ctypes.POINTER(i64), ctypes.POINTER(i64)]
    lib.ds_freq_result.restype = i64
    lib.ds_freq_end.argtypes = [vp]
    lib.ds_freq_reference.argtypes = [vp, i64, vp, vp, vp, vp, f64, vp, vp, vp, vp, vp, i64, vp, vp, vp, vp, vp, vp, vp,
                                      ctypes.POINTER(i64)]
    lib.ds_freq_reference.restype = i64
    lib.ds_get_freq_times.argtypes = [vp, i32, ctypes.POINTER(i64), ctypes.POINTER(f64)]
    lib.ds_eval_locate.argtypes = [vp, i64, i64, vp, vp, vp, ctypes.POINTER(i32)]
    lib.ds_eval_locate.restype = i64
    lib.ds_eval_begin.argtypes = [vp, i64, i32, i32, vp]
    lib.ds_eval_parse.argtypes = [vp, vp, i32, vp, vp, vp, vp]
    lib.ds_eval_accumulate.argtypes = [vp, vp, i32, vp, vp, vp, vp]
    lib.ds_eval_result.argtypes = [vp, vp, vp, vp, vp, ctypes.POINTER(i64), ctypes.POINTER(i64)]
    lib.ds_eval_end.argtypes = [vp]
    lib.ds_eval_reference.argtypes = [vp, i64, vp, vp, vp, vp, i32, vp, vp, vp, vp, vp, vp, vp, vp, vp]
    lib.ds_get_eval_times.argtypes = [vp, i32, ctypes.POINTER(i64), ctypes.POINTER(f64)]
    lib.ds_freq_begin_stream.argtypes = [vp, i64, i32, f64]
    lib.ds_freq_push.argtypes = [vp, i32, vp, vp, vp, i32, vp, vp, vp]
    lib.ds_freq_keys.argtypes = [i64, vp, vp, vp, vp, vp, vp, i64, ctypes.POINTER(i64), ctypes.POINTER(i32)]
    lib.ds_freq_keys.restype = i64
    lib.ds_freq_values.argtypes = [vp, i64, vp, i32, vp, vp, vp]
    lib.ds_freq_values_reference.argtypes = [i64, vp, i32, vp, vp, vp]
    lib.ds_get_freq_stream_times.argtypes = [vp, i32, ctypes.POINTER(i64), ctypes.POINTER(f64)]
    u8p = vp
    lib.ds_fasta_locate.argtypes = [vp, i64, i64, vp, vp, vp, vp, i64, vp, vp, vp, ctypes.POINTER(i64), ctypes.POINTER(i32)]
    lib.ds_fasta_locate.restype = i64
    lib.ds_combine_begin.argtypes = [vp, i32, i32, vp, i64, i32]
    lib.ds_combine_genome.argtypes = [vp, vp, i64, vp, vp, vp, u8p]
    lib.ds_combine_bitmap.argtypes = [vp, i64, vp]
    lib.ds_combine_parse.argtypes = [vp, vp, i32, vp, vp, vp, vp, vp]
    lib.ds_combine_accumulate.argtypes = [vp, i32, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp]
    lib.ds_combine_result.argtypes = [vp, i64, vp, vp, vp, vp, vp, vp, vp, vp, ctypes.POINTER(i64)]
    lib.ds_combine_result.restype = i64
    lib.ds_combine_end.argtypes = [vp]
    lib.ds_motif_reference.argtypes = [vp, i64, vp, vp, vp, u8p, i64, vp]
    lib.ds_combine_reference.argtypes = [i32, vp, i64, vp, vp, vp, vp, i32, vp, vp] + [vp] * 8 + [i64] + [vp] * 8
    lib.ds_combine_reference.restype = i64
    lib.ds_get_combine_times.argtypes = [vp, i32, ctypes.POINTER(i64), ctypes.POINTER(i64), ctypes.POINTER(f64)]
    lib.ds_train_begin.argtypes = [vp, ctypes.POINTER(DsTrainConfig)]
    lib.ds_train_set_tensor.argtypes = [vp, ctypes.c_char_p, vp, i64]
    lib.ds_train_step.argtypes = [vp, i32, vp, vp, vp, vp, ctypes.c_float, ctypes.POINTER(ctypes.c_float), vp]
    lib.ds_train_sync_weights.argtypes = [vp]
    lib.ds_train_begin_base.argtypes = [vp, ctypes.POINTER(DsTrainConfig)]
    lib.ds_train_step_base.argtypes = [vp, i32, vp, vp, vp, vp, vp, ctypes.c_float, ctypes.POINTER(ctypes.c_float), vp]
    lib.ds_train_eval.argtypes = [vp, i32, vp, vp, vp, vp, vp, ctypes.POINTER(ctypes.c_float), vp, vp]
    lib.ds_train_begin_signal.argtypes = [vp, ctypes.POINTER(DsTrainConfig)]
    lib.ds_train_step_signal.argtypes = [vp, i32, vp, vp, ctypes.c_float, ctypes.POINTER(ctypes.c_float), vp]
    lib.ds_train_eval_signal.argtypes = [vp, i32, vp, vp, ctypes.POINTER(ctypes.c_float), vp, vp]
    lib.ds_train_mask_reference_wide.argtypes = [ctypes.c_uint64, i64, ctypes.c_char_p, i32, i32, ctypes.c_float, vp]
    for fn in (lib.ds_train_get_tensor, lib.ds_train_get_grad, lib.ds_train_get_mask, lib.ds_train_get_tap):
        fn.argtypes = [vp, ctypes.c_char_p, vp, i64]
        fn.restype = i64
    lib.ds_train_end.argtypes = [vp]
    lib.ds_train_mask_reference.argtypes = [ctypes.c_uint64, i64, ctypes.c_char_p, i32, i32, ctypes.c_float, vp]
    lib.ds_get_train_times.argtypes = [vp, i32, ctypes.POINTER(i64), ctypes.POINTER(f64)]
    _lib = lib
    return lib


# ---- training step of the RNN-only model (include/deepsignal_hip.h, "training step") --------------------------------------------
MASK_STREAMS = ("fw_l0", "fw_l1", "fw_l2", "bw_l0", "bw_l1", "bw_l2", "fc1", "fc2")
TRAIN_PHASES = ("forward_sweep", "backward_sweep", "weight_gradients", "head", "adam")


def mask_shape(stream: str, n: int, kmer_len: int) -> Tuple[int, ...]:
    if stream not in MASK_STREAMS:
        raise ValueError("mask stream must be one of %s" % (MASK_STREAMS,))
    return (n, kmer_len, 256) if stream[2] == "_" else (n, 512 if stream == "fc1" else 2)


def train_mask_reference(seed: int, step: int, stream: str, n: int, kmer_len: int, keep_prob: float) -> np.ndarray:
    """The dropout mask of `stream` for rows 0 .. n - 1 of step `step` (counted from 0), computed on the CPU by the function
    the kernels run: a checker, no handle, no GPU."""
    out = np.empty(mask_shape(stream, n, kmer_len), np.uint8)
    rc = load_library().ds_train_mask_reference(seed, step, stream.encode(), n, kmer_len, keep_prob, out.ctypes.data)
    if rc != 0:
        raise ValueError("ds_train_mask_reference failed (%d): bad stream, size or keep_prob" % rc)
    return out


def trainable_names(is_base: bool = False) -> List[str]:
    """TF names of the tensors the RNN-only model trains, in the order of `spec.tensor_table`: 14, and `modelembedding` before
    them with is_base."""
    from . import spec
    return [name for name, _ in spec.tensor_table(17, 360, 2, is_cnn=False, is_rnn=True, is_base=is_base)]


# ---- ... of the signal-only model (is_cnn, not is_rnn; include/deepsignal_hip.h, "training step of the signal-only model") ---------
SIGNAL_MASK_STREAMS = ("fc1", "fc2")
SIGNAL_TRAIN_PHASES = ("forward", "backward", "weight_gradients", "joint_layers", "adam")


def train_mask_reference_wide(seed: int, step: int, stream: str, n: int, width: int, keep_prob: float) -> np.ndarray:
    """train_mask_reference for a joint-layer stream ("fc1", "fc2") whose rows are `width` units wide (fc1 of the signal-only
    model: J = w_c x 240): uint8 [n, width]."""
    if stream not in SIGNAL_MASK_STREAMS:
        raise ValueError("mask stream must be one of %s" % (SIGNAL_MASK_STREAMS,))
    out = np.empty((n, width), np.uint8)
    rc = load_library().ds_train_mask_reference_wide(seed, step, stream.encode(), n, width, keep_prob, out.ctypes.data)
    if rc != 0:
        raise ValueError("ds_train_mask_reference_wide failed (%d): bad stream, size (width 1 .. 65535) or keep_prob" % rc)
    return out


def signal_tensor_names(signal_len: int = 360) -> List[str]:
    """TF names of every tensor of the signal-only model, moving statistics included, in the order of `spec.tensor_table`."""
    from . import spec
    return [name for name, _ in spec.tensor_table(17, signal_len, 2, is_cnn=True, is_rnn=False)]


def signal_trainable_names(signal_len: int = 360) -> List[str]:
    """... of the 341 it trains: 113 kernels, 113 beta, 113 gamma, the two dense kernels."""
    return [name for name in signal_tensor_names(signal_len) if not name.endswith(("/moving_mean", "/moving_variance"))]


def signal_tap_names() -> List[str]:
    """What Engine.train_tap takes: every conv + BN (+ ReLU) output, each module's b5 after the add, feat and logits."""
    from . import spec
    names = ["stem1", "stem2", "stem3"]
    for m in range(1, spec.N_INCEPTION + 1):
        names += ["m%d.%s" % (m, key) for key in spec.INCEPTION_KEYS] + ["m%d.b5" % m]
    return names + ["feat", "logits"]


class Engine:
    """One handle == one GPU == one full weight replica."""

    def __init__(self, kmer_len: int = 17, signal_len: int = 360, class_num: int = 2, device: int = 0,
                 max_batch: int = 512, is_cnn: bool = True, is_rnn: bool = True, is_base: bool = True,
                 debug: bool = False, slots: int = 0, precision: str = "fp32", serial: bool = False,
                 no_fused: bool = False, debug_stamps: bool = False, fold_fc: bool = True, lstm_tiling: str = "auto",
                 fuse_max_spt: int = 0, fuse_min_tiles: int = 0, chain_modules: bool = True, shared_event_stream: bool = False,
                 split_dense_min_n: int = 0, split_dense_narrow: bool = False, lstm_xproj=True):
        self._lib = load_library()
        self._h = ctypes.c_void_p()
        # opened: the array of a freq_push, alive until the library has filled it; words: the combine run's bitmap
        self._freq, self._combine, self._eval = _TableRun(opened=None), _TableRun(words=0), _TableRun(ncf=1)
        if precision not in PRECISIONS:
            raise ValueError("precision must be one of %s" % (sorted(PRECISIONS),))
        self.precision = precision
        cfg = DsConfig(kmer_len, signal_len, class_num, int(is_cnn), int(is_rnn), int(is_base), device,
                       PRECISIONS[precision], max_batch)
        cfg.reserved[0] = 1 if debug else 0
        cfg.reserved[1] = slots          # forwards in flight for run_device (0 = engine default)
        # per-handle diagnostics / tuning (include/deepsignal_hip.h: DS_TUNE_*, DS_LSTM_TILING_*); the library reads
        # no environment variables
        cfg.reserved[2] = (TUNE_NO_FUSED if no_fused else 0) | (TUNE_SERIAL if serial else 0) | \
                          (TUNE_DEBUG_STAMPS if debug_stamps else 0) | (0 if fold_fc else TUNE_NO_FOLD_FC) | \
                          (0 if chain_modules else TUNE_NO_CHAIN) | (TUNE_SHARED_EVENT_STREAM if shared_event_stream else 0) | \
                          (TUNE_SPLIT_DENSE_NARROW if split_dense_narrow else 0) | \
                          (0 if lstm_xproj else TUNE_NO_LSTM_XPROJ) | (TUNE_LSTM_XPROJ_ALL if lstm_xproj == "all" else 0)
        if lstm_tiling not in LSTM_TILINGS:
            raise ValueError("lstm_tiling must be one of %s" % (sorted(LSTM_TILINGS),))
        cfg.reserved[3] = LSTM_TILINGS[lstm_tiling]
        cfg.reserved[4] = fuse_max_spt
        cfg.reserved[5] = fuse_min_tiles
        cfg.reserved[6] = split_dense_min_n
        rc = self._lib.ds_create(ctypes.byref(cfg), ctypes.byref(self._h))
        if rc != 0:
            msg = self._lib.ds_last_error(None).decode()
            self._h = ctypes.c_void_p()
            raise RuntimeError("ds_create failed (%d): %s" % (rc, msg))
        self.kmer_len, self.signal_len, self.class_num = kmer_len, signal_len, class_num
        self._slots = int(self._lib.ds_num_slots(self._h))
        self.device, self.max_batch = device, max_batch
        self.is_base = bool(is_base)
        self.is_cnn, self.is_rnn = bool(is_cnn), bool(is_rnn)
        self.signal_only = self.is_cnn and not self.is_rnn      # the variant ds_train_begin_signal trains
        self._fine: Optional["Engine"] = None      # set_recheck: the attached engine stays referenced here
        self._owns_fine = False

    # -- lifecycle -----------------------------------------------------------------------------
    def close(self) -> None:
        if getattr(self, "_h", None) and self._h.value:
            fine, owned = getattr(self, "_fine", None), getattr(self, "_owns_fine", False)
            if fine is not None:                   # detach first: the library must not keep a handle that may go away
                self._lib.ds_set_recheck(self._h, None, 0.0)
                self._fine, self._owns_fine = None, False
            self._lib.ds_destroy(self._h)
            self._h = ctypes.c_void_p()
            if fine is not None and owned:
                fine.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc: int, what: str) -> None:
        if rc < 0:
            raise RuntimeError("%s failed (%d): %s" % (what, rc, self._lib.ds_last_error(self._h).decode()))

    def _check_memory(self, rc: int, what: str) -> None:
        """_check for the calls that allocate for a site-table run: DS_ERR_NOMEM is FreqNoMemory."""
        if rc == -5:
            raise FreqNoMemory(self._lib.ds_last_error(self._h).decode())
        self._check(rc, what)

    def _times(self, fn, what: str, names, counters=("batches",), reset: bool = False) -> dict:
        """A ds_get_*_times getter: the summed device milliseconds under `names` and the counts under `counters`."""
        counts = [ctypes.c_int64() for _ in counters]
        ms = (ctypes.c_double * len(names))()
        self._check(fn(self._h, int(reset), *(ctypes.byref(c) for c in counts), ms), what)
        return dict(zip(names, ms), **{k: int(c.value) for k, c in zip(counters, counts)})

    def _run_parse(self, run: _TableRun, fn, what: str, text, begin, end, chrom, flags) -> np.ndarray:
        """A *_parse: the batch's rows to the library (chrom None: the route's rows name no chromosome) -> the per-row status."""
        keep, addr, begin, end, ids, flags = _batch_rows_args(text, begin, end, np.zeros(len(begin), np.int32) if chrom is None else chrom,
                                                              flags, run.batch)
        n = int(begin.size)
        status = np.empty(n, np.int32)
        cols = (flags,) if chrom is None else (ids, flags)
        self._check(fn(self._h, addr, n, begin.ctypes.data, end.ctypes.data, *(c.ctypes.data for c in cols), status.ctypes.data), what)
        run.pending = n
        return status

    @staticmethod
    def _run_batch(run: _TableRun, route: str, rows: np.ndarray) -> int:
        """The head of a *_accumulate: the rows of the batch parsed last, of which `rows` must be ascending indices."""
        if run.pending < 0:
            raise ValueError("%s_accumulate needs a batch from %s_parse" % (route, route))
        _check_override_rows(rows, run.pending)
        return run.pending

    def _sites_result(self, fn, what: str, fields, *scalars) -> Dict[str, np.ndarray]:
        """The two calls of ds_freq_result / ds_combine_result: the number of sites, then arrays of that size filled."""
        nulls = (None,) * len(fields)
        tail = [ctypes.byref(v) for v in scalars]
        n = int(fn(self._h, 0, *nulls, *tail))
        self._check(n, what)
        out = {k: np.empty(n, dt) for k, dt in fields}
        if n:
            got = int(fn(self._h, n, *(out[k].ctypes.data for k, _ in fields), *tail))
            self._check(got, what)
            if got != n:
                raise RuntimeError("%s: %d sites announced, %d returned" % (what, n, got))
        return out

    # -- weights (Saver.restore, call_modifications.py:210-211) --------------------------------
    def load_weights_file(self, path: str) -> None:
        self._check(self._lib.ds_load_weights(self._h, path.encode()), "ds_load_weights")

    def load_weights(self, weights: Dict[str, np.ndarray]) -> None:
        for name, arr in weights.items():
            a = np.ascontiguousarray(arr, dtype=np.float32)
            shape = (ctypes.c_int64 * a.ndim)(*a.shape)
            self._check(self._lib.ds_set_tensor(self._h, name.encode(), a.ctypes.data, shape, a.ndim), "ds_set_tensor")
        self._check(self._lib.ds_finalize_weights(self._h), "ds_finalize_weights")

    # -- training step of the RNN-only model (denoise.py:97-110) -------------------------------
    def train_begin(self, keep_prob: float = 0.5, pos_weight: float = 1.0, seed: int = 0, beta1: float = 0.0, beta2: float = 0.0,
                    epsilon: float = 0.0, weights: Optional[Dict[str, np.ndarray]] = None, base: bool = False) -> None:
        """Start (or start over) from the loaded weights, or from `weights` installed in their place: fp32 master
        parameters, zero Adam moments, step 0. beta1 / beta2 / epsilon 0 = TF's defaults. base=True opens the run through
        ds_train_begin_base, which also takes an is_base handle (the embedding is trained; train_step then needs `kmer`)."""
        if weights is not None:
            for name, arr in weights.items():
                a = np.ascontiguousarray(arr, dtype=np.float32)
                self._check(self._lib.ds_train_set_tensor(self._h, name.encode(), a.ctypes.data, a.size), "ds_train_set_tensor")
        cfg = DsTrainConfig(keep_prob, pos_weight, beta1, beta2, epsilon, seed & 0xFFFFFFFFFFFFFFFF)
        if self.signal_only:
            self._check(self._lib.ds_train_begin_signal(self._h, ctypes.byref(cfg)), "ds_train_begin_signal")
        elif base:
            self._check(self._lib.ds_train_begin_base(self._h, ctypes.byref(cfg)), "ds_train_begin_base")
        else:
            self._check(self._lib.ds_train_begin(self._h, ctypes.byref(cfg)), "ds_train_begin")

    def _train_arrays(self, means, stds, sanums, labels, kmer):
        means = np.ascontiguousarray(means, dtype=np.float32)
        stds = np.ascontiguousarray(stds, dtype=np.float32)
        sanums = np.ascontiguousarray(sanums, dtype=np.float32)
        labels = np.ascontiguousarray(labels, dtype=np.int32)
        n = int(labels.shape[0]) if labels.ndim == 1 else -1
        if means.ndim != 2 or means.shape != (n, self.kmer_len) or stds.shape != means.shape or sanums.shape != means.shape:
            raise ValueError("training arrays have inconsistent shapes")
        if kmer is not None:
            kmer = np.ascontiguousarray(kmer, dtype=np.int32)
            if kmer.shape != means.shape:
                raise ValueError("training arrays have inconsistent shapes")
        return n, means, stds, sanums, labels, kmer

    def _train_call(self, what: str, n: int, *args, lr: Optional[float] = None):
        """One step (`lr` given) or evaluation entry `what` on n rows: makes the loss, prediction and, for an evaluation, logits
        buffers, calls it with the inputs `args` in front and checks the return code."""
        loss = ctypes.c_float()
        pred = np.empty((n,), np.int32)
        fn = getattr(self._lib, what)
        if lr is not None:
            self._check(fn(self._h, n, *args, lr, ctypes.byref(loss), pred.ctypes.data), what)
            return float(loss.value), pred
        logits = np.empty((n, 2), np.float32)
        self._check(fn(self._h, n, *args, ctypes.byref(loss), pred.ctypes.data, logits.ctypes.data), what)
        return float(loss.value), pred, logits

    def train_step(self, means, stds, sanums, labels, lr: float, kmer=None) -> Tuple[float, np.ndarray]:
        """One step on these rows: (cost, prediction int32[n]). `kmer` int32[n, kmer_len]: the codes, which a run that trains
        the embedding needs (without them it is refused); given, the step goes through ds_train_step_base."""
        n, means, stds, sanums, labels, kmer = self._train_arrays(means, stds, sanums, labels, kmer)
        rows = (means.ctypes.data, stds.ctypes.data, sanums.ctypes.data, labels.ctypes.data)
        if kmer is not None:
            return self._train_call("ds_train_step_base", n, kmer.ctypes.data, *rows, lr=lr)
        return self._train_call("ds_train_step", n, *rows, lr=lr)

    def train_eval(self, means, stds, sanums, labels, kmer=None) -> Tuple[float, np.ndarray, np.ndarray]:
        """The training forward on the current parameters with keep_prob 1 and nothing changed: (cost, prediction int32[n],
        logits float32[n, 2])."""
        n, means, stds, sanums, labels, kmer = self._train_arrays(means, stds, sanums, labels, kmer)
        return self._train_call("ds_train_eval", n, None if kmer is None else kmer.ctypes.data, means.ctypes.data, stds.ctypes.data,
                                sanums.ctypes.data, labels.ctypes.data)

    # -- ... of the signal-only model (train_model.py with --is_cnn yes --is_rnn no) --------------
    def _signal_arrays(self, signals, labels):
        signals = np.ascontiguousarray(signals, dtype=np.float32)
        labels = np.ascontiguousarray(labels, dtype=np.int32)
        n = int(labels.shape[0]) if labels.ndim == 1 else -1
        if signals.shape != (n, self.signal_len):
            raise ValueError("training arrays have inconsistent shapes")
        return n, signals, labels

    def train_step_signal(self, signals, labels, lr: float) -> Tuple[float, np.ndarray]:
        """One step of a signal run on signals float32[n, signal_len]: (cost, prediction int32[n])."""
        n, signals, labels = self._signal_arrays(signals, labels)
        return self._train_call("ds_train_step_signal", n, signals.ctypes.data, labels.ctypes.data, lr=lr)

    def train_eval_signal(self, signals, labels) -> Tuple[float, np.ndarray, np.ndarray]:
        """training = False, keep_prob = 1: the forward on the current parameters with the moving statistics, nothing changed:
        (cost, prediction int32[n], logits float32[n, 2])."""
        n, signals, labels = self._signal_arrays(signals, labels)
        return self._train_call("ds_train_eval_signal", n, signals.ctypes.data, labels.ctypes.data)

    def train_tap(self, name: str, n: int) -> np.ndarray:
        """A layer output of the last step of a signal run (`signal_tap_names`), float32 [n, W, C] ([n, C] for feat and logits)."""
        from . import spec
        d = spec.net_dims(self.kmer_len, self.signal_len, self.class_num, True, False)
        if name in ("feat", "logits"):
            shape = (n, d.joint if name == "feat" else 2)
        elif name == "stem1":
            shape = (n, d.w_conv1, 64)
        elif name in ("stem2", "stem3"):
            shape = (n, d.w_a, 128 if name == "stem2" else 256)
        else:
            m, _, key = name.partition(".")
            if name not in signal_tap_names():
                raise KeyError(name)
            k = int(m[1:])
            shape = (n, d.module_width(k), 48 if key == "b5" else spec.inception_convs(k, d.module_cin(k))[key].cout)
        out = np.empty(shape, np.float32)
        got = int(self._lib.ds_train_get_tap(self._h, name.encode(), out.ctypes.data, out.size))
        self._check(got, "ds_train_get_tap")
        if got != out.size:
            raise RuntimeError("ds_train_get_tap: the last step had %d elements of %s, %d asked for" % (got, name, out.size))
        return out

    def train_sync_weights(self) -> None:
        self._check(self._lib.ds_train_sync_weights(self._h), "ds_train_sync_weights")

    def _train_tensor(self, fn, what: str, name: str) -> np.ndarray:
        from . import spec
        shapes = dict(spec.tensor_table(self.kmer_len, self.signal_len, self.class_num, is_cnn=self.signal_only, is_rnn=not self.signal_only,
                                        is_base=self.is_base))
        if name not in shapes:
            raise KeyError(name)
        out = np.empty(shapes[name], np.float32)
        got = int(fn(self._h, name.encode(), out.ctypes.data, out.size))
        self._check(got, what)
        if got != out.size:
            raise RuntimeError("%s: %d floats expected, %d returned" % (what, out.size, got))
        return out

    def train_tensor(self, name: str) -> np.ndarray:
        return self._train_tensor(self._lib.ds_train_get_tensor, "ds_train_get_tensor", name)

    def train_grad(self, name: str) -> np.ndarray:
        return self._train_tensor(self._lib.ds_train_get_grad, "ds_train_get_grad", name)

    def train_tensors(self) -> Dict[str, np.ndarray]:
        """Every current tensor of the run by name (a signal run: the moving statistics too)."""
        names = signal_tensor_names(self.signal_len) if self.signal_only else trainable_names(self.is_base)
        return {name: self.train_tensor(name) for name in names}

    def train_grads(self) -> Dict[str, np.ndarray]:
        names = signal_trainable_names(self.signal_len) if self.signal_only else trainable_names(self.is_base)
        return {name: self.train_grad(name) for name in names}

    def train_mask(self, stream: str, n: int) -> np.ndarray:
        if self.signal_only:
            from . import spec
            if stream not in SIGNAL_MASK_STREAMS:
                raise ValueError("mask stream must be one of %s" % (SIGNAL_MASK_STREAMS,))
            out = np.empty((n, spec.net_dims(self.kmer_len, self.signal_len, self.class_num, True, False).joint if stream == "fc1" else 2), np.uint8)
        else:
            out = np.empty(mask_shape(stream, n, self.kmer_len), np.uint8)
        got = int(self._lib.ds_train_get_mask(self._h, stream.encode(), out.ctypes.data, out.size))
        self._check(got, "ds_train_get_mask")
        if got != out.size:
            raise RuntimeError("ds_train_get_mask: the last step had %d mask elements, %d asked for" % (got, out.size))
        return out

    def train_end(self) -> None:
        self._check(self._lib.ds_train_end(self._h), "ds_train_end")

    def train_times(self, reset: bool = False) -> dict:
        steps = ctypes.c_int64()
        ms = (ctypes.c_double * len(TRAIN_PHASES))()
        self._check(self._lib.ds_get_train_times(self._h, int(reset), ctypes.byref(steps), ms), "ds_get_train_times")
        return {"steps": int(steps.value), "ms": dict(zip(SIGNAL_TRAIN_PHASES if self.signal_only else TRAIN_PHASES, (float(v) for v in ms)))}

    # -- forward (sess.run, call_modifications.py:177-178) -------------------------------------
    def run(self, kmer, means, stds, sanums, signals) -> Tuple[np.ndarray, np.ndarray]:
        """Host arrays in, (activation_logits float32[n,class_num], prediction int32[n]) out."""
        kmer = np.ascontiguousarray(kmer, dtype=np.int32)
        n = kmer.shape[0] if kmer.ndim == 2 else 0
        means = np.ascontiguousarray(means, dtype=np.float32)
        stds = np.ascontiguousarray(stds, dtype=np.float32)
        sanums = np.ascontiguousarray(sanums, dtype=np.float32)     # int -> float cast as the TF feed does
        signals = np.ascontiguousarray(signals, dtype=np.float32)
        act = np.empty((n, self.class_num), np.float32)
        pred = np.empty((n,), np.int32)
        if n == 0:
            return act, pred
        if kmer.shape != (n, self.kmer_len) or means.shape != kmer.shape or stds.shape != kmer.shape \
                or sanums.shape != kmer.shape or signals.shape != (n, self.signal_len):
            raise ValueError("feature arrays have inconsistent shapes")
        rc = self._lib.ds_forward(self._h, n, kmer.ctypes.data, means.ctypes.data, stds.ctypes.data,
                                  sanums.ctypes.data, signals.ctypes.data, act.ctypes.data, pred.ctypes.data)
        self._check(rc, "ds_forward")
        return act, pred

    def run_device(self, n: int, d_kmer: int, d_means: int, d_stds: int, d_sanums: int, d_signals: int,
                   d_act: int, d_pred: int) -> None:
        """Raw device pointers (e.g. torch tensors' data_ptr()); asynchronous, call sync()."""
        rc = self._lib.ds_forward_device(self._h, n, d_kmer, d_means, d_stds, d_sanums, d_signals, d_act, d_pred)
        self._check(rc, "ds_forward_device")

    def sync(self) -> None:
        self._check(self._lib.ds_sync(self._h), "ds_sync")

    def submit(self, kmer, means, stds, sanums, signals) -> Tuple[int, int]:
        """Asynchronous run() of one batch (n <= max_batch): returns a ticket for wait(). Up to `slots` batches may be
        in flight; wait() them in submission order."""
        kmer = np.ascontiguousarray(kmer, dtype=np.int32)
        n = int(kmer.shape[0])
        arrs = [np.ascontiguousarray(a, dtype=np.float32) for a in (means, stds, sanums, signals)]
        t = ctypes.c_int32()
        self._check(self._lib.ds_submit(self._h, n, kmer.ctypes.data, *(a.ctypes.data for a in arrs), ctypes.byref(t)),
                    "ds_submit")
        return (int(t.value), n)

    def submit_parts(self, parts) -> Tuple[int, int]:
        """submit() of one batch given as row segments: `parts` is a sequence of (kmer, means, stds, sanums, signals)
        array tuples; the rows are gathered into the pinned staging buffer by the library (no concatenated copy)."""
        k = len(parts)
        keep = [(np.ascontiguousarray(p[0], dtype=np.int32),) + tuple(np.ascontiguousarray(a, dtype=np.float32) for a in p[1:5])
                for p in parts]
        counts = (ctypes.c_int32 * k)(*[int(p[0].shape[0]) for p in keep])
        ptrs = [(ctypes.c_void_p * k)(*[p[j].ctypes.data for p in keep]) for j in range(5)]
        n = int(sum(counts))
        t = ctypes.c_int32()
        self._check(self._lib.ds_submit_parts(self._h, k, counts, *ptrs, ctypes.byref(t)), "ds_submit_parts")
        return (int(t.value), n)

    def wait(self, ticket: Tuple[int, int]) -> Tuple[np.ndarray, np.ndarray]:
        slot, n = ticket
        act = np.empty((n, self.class_num), np.float32)
        pred = np.empty((n,), np.int32)
        self._check(self._lib.ds_wait(self._h, slot, act.ctypes.data, pred.ctypes.data), "ds_wait")
        return act, pred

    def extract(self, batch: ReadBatch) -> Dict[str, np.ndarray]:
        """ds_extract: the features of every site of `batch` (nsites <= max_batch), computed on the GPU, as host arrays
        kmer / means / stds / sanums / signals (the inputs of run())."""
        out = _feature_arrays(batch.nsites, self.kmer_len, self.signal_len)
        self._check(self._lib.ds_extract(self._h, ctypes.byref(batch.desc),
                                         *(out[k].ctypes.data for k in ("kmer", "means", "stds", "sanums", "signals"))),
                    "ds_extract")
        return out

    def submit_reads(self, batch: ReadBatch) -> Tuple[int, int]:
        """ds_submit_reads: features extracted on the GPU straight into the forward's inputs; a ticket for wait(), as submit()."""
        t = ctypes.c_int32()
        self._check(self._lib.ds_submit_reads(self._h, ctypes.byref(batch.desc), ctypes.byref(t)), "ds_submit_reads")
        return (int(t.value), batch.nsites)

    def submit_rows(self, batch: ReadBatch, info, info_off, label: int) -> Tuple[int, int]:
        """ds_submit_rows: the feature rows of `batch` (nsites <= max_batch) formatted on the GPU; a ticket for wait_rows().
        info / info_off: the rows' six leading columns (pack_info). Needs no weights."""
        info = np.ascontiguousarray(info, np.uint8)
        info_off = np.ascontiguousarray(info_off, np.int64)
        if info_off.shape[0] != batch.nsites + 1:
            raise ValueError("info_off must have nsites + 1 entries")
        t = ctypes.c_int32()
        self._check(self._lib.ds_submit_rows(self._h, ctypes.byref(batch.desc), info.ctypes.data, info_off.ctypes.data, label,
                                             ctypes.byref(t)), "ds_submit_rows")
        return (int(t.value), batch.nsites)

    def wait_rows(self, ticket: Tuple[int, int]):
        """ds_wait_rows -> (the rows' bytes, int64 row offsets[nsites + 1])."""
        slot, n = ticket
        got, self._rows_buf, row_off = _rows_call(lambda o, c, ro: self._lib.ds_wait_rows(self._h, slot, o, c, ro), n,
                                                  getattr(self, "_rows_buf", None))
        self._check(got, "ds_wait_rows")
        return self._rows_buf[:got].tobytes(), row_off

    def extract_rows(self, batch: ReadBatch, info, info_off, label: int):
        """ds_extract_rows: the blocking form of submit_rows() + wait_rows()."""
        info = np.ascontiguousarray(info, np.uint8)
        info_off = np.ascontiguousarray(info_off, np.int64)
        if info_off.shape[0] != batch.nsites + 1:
            raise ValueError("info_off must have nsites + 1 entries")
        got, self._rows_buf, row_off = _rows_call(lambda o, c, ro: self._lib.ds_extract_rows(
            self._h, ctypes.byref(batch.desc), info.ctypes.data, info_off.ctypes.data, label, o, c, ro), batch.nsites,
            getattr(self, "_rows_buf", None))
        self._check(got, "ds_extract_rows")
        return self._rows_buf[:got].tobytes(), row_off

    # -- feature-TSV rows parsed on the device (ds_submit_text / ds_wait_text) -------------------
    def submit_text(self, text, begin, end):
        """ds_submit_text: the rows text[begin[i]:end[i]] (bytes, a uint8 array, or the address of a buffer such as
        FeatureReader.data) parsed on the GPU straight into a forward's inputs; a ticket for wait_text(). The text must stay
        alive and unchanged until then (an array given here is kept referenced by the ticket)."""
        keep, addr, begin, end = _text_args(text, begin, end)
        t = ctypes.c_int32()
        self._check(self._lib.ds_submit_text(self._h, addr, begin.size, begin.ctypes.data, end.ctypes.data, ctypes.byref(t)),
                    "ds_submit_text")
        return (int(t.value), int(begin.size), int((end - begin).sum()), keep)

    def wait_text(self, ticket):
        """ds_wait_text -> (act, pred, kmer, labels, info uint8 blob, info_off int64[n + 1]): wait()'s results plus what
        fastio.format_rows needs. Rows outside the device's grammar were parsed by the host parser and forwarded again; a
        malformed one raises TextRowError (its .row = the index within the ticket)."""
        slot, n, nbytes = ticket[0], ticket[1], ticket[2]
        act = np.empty((n, self.class_num), np.float32)
        pred, labels = np.empty((n,), np.int32), np.empty((n,), np.int32)
        kmer = np.empty((n, self.kmer_len), np.int32)
        info = np.empty(max(1, nbytes), np.uint8)
        info_off = np.empty(n + 1, np.int64)
        rc = self._lib.ds_wait_text(self._h, slot, act.ctypes.data, pred.ctypes.data, kmer.ctypes.data, labels.ctypes.data,
                                    info.ctypes.data, info.size, info_off.ctypes.data)
        if rc == -3:
            import re
            msg = self._lib.ds_last_error(self._h).decode()
            m = re.search(r"row (\d+) of the ticket", msg)
            raise TextRowError(int(m.group(1)) if m else -1, msg)
        self._check(rc, "ds_wait_text")
        return act, pred, kmer, labels, info[:int(info_off[n])], info_off

    def parse_text(self, text, begin, end) -> Dict[str, np.ndarray]:
        """ds_parse_text (diagnostic, needs no weights): the device parser's arrays and per-row status, as parse_text_reference."""
        keep, addr, begin, end = _text_args(text, begin, end)
        out = _text_arrays(begin.size, self.kmer_len, self.signal_len)
        self._check(self._lib.ds_parse_text(self._h, addr, begin.size, begin.ctypes.data, end.ctypes.data,
                                            *(out[k].ctypes.data for k in _TEXT_ORDER)), "ds_parse_text")
        return out

    def text_stats(self) -> dict:
        """ds_get_text_stats: rows through submit_text / wait_text since construction, and those the host parser took."""
        a, b = ctypes.c_int64(), ctypes.c_int64()
        self._check(self._lib.ds_get_text_stats(self._h, ctypes.byref(a), ctypes.byref(b)), "ds_get_text_stats")
        return {"rows": int(a.value), "host_rows": int(b.value)}

    def text_times(self, reset: bool = False) -> dict:
        """ds_get_text_times: device milliseconds of the text batches so far (H2D of the text, the parse kernel, D2H)."""
        return self._times(self._lib.ds_get_text_times, "ds_get_text_times", ("h2d_ms", "kernel_ms", "d2h_ms"), reset=reset)

    # -- per-site modification frequency on the device (ds_freq_*; call_freq --on gpu) ----------
    def freq_begin(self, total_rows: int, batch_rows: int, prob_cf: float = 0.0) -> None:
        """ds_freq_begin: open a run whose batches hold at most batch_rows rows and total_rows rows in all (the site table is
        sized from it, at most half full). FreqNoMemory when the table or the buffers do not fit the device. Needs no weights."""
        (total_rows, batch_rows), prob_cf = _run_sizes(total_rows, batch_rows), float(prob_cf)
        if prob_cf != prob_cf:
            raise ValueError("prob_cf must not be NaN")
        rc = self._lib.ds_freq_begin(self._h, total_rows, batch_rows, prob_cf)
        self._check_memory(rc, "ds_freq_begin")
        self._freq.begin(batch_rows)

    def freq_begin_stream(self, initial_slots: int, batch_rows: int, prob_cf: float = 0.0) -> None:
        """ds_freq_begin_stream: open a run whose number of rows is not known: the site table starts with initial_slots slots and
        doubles as sites arrive; batches come through freq_push. FreqNoMemory when the table or the buffers do not fit the device."""
        initial_slots, batch_rows, prob_cf = int(initial_slots), int(batch_rows), float(prob_cf)
        if not 1 <= initial_slots <= 2 * FREQ_MAX_ROWS:
            raise ValueError("initial_slots must be in [1, 2^31]")
        if not 1 <= batch_rows <= FREQ_MAX_BATCH:
            raise ValueError("batch_rows must be in [1, 2^24]")
        if prob_cf != prob_cf:
            raise ValueError("prob_cf must not be NaN")
        rc = self._lib.ds_freq_begin_stream(self._h, initial_slots, batch_rows, prob_cf)
        self._check_memory(rc, "ds_freq_begin_stream")
        self._freq.begin(batch_rows, opened=None)

    def freq_push(self, chrom, pos, act, pred) -> np.ndarray:
        """ds_freq_push: one batch of a streaming run -- chromosome ids, positions (freq_keys, the ids mapped to one numbering for
        the run; -1 = a row for Python), the forward's act rows and pred -> the per-row status (TEXT_ROW_OK / TEXT_ROW_HOST).
        freq_accumulate completes the batch and returns which rows opened a site. FreqNoMemory: the table could not grow."""
        chrom, pred = np.ascontiguousarray(chrom, np.int32), np.ascontiguousarray(pred, np.int32)
        pos = np.ascontiguousarray(pos, np.int64)
        act = _act_rows(act)
        n = act.shape[0]
        if chrom.shape != (n,) or pos.shape != (n,) or pred.shape != (n,):
            raise ValueError("chrom / pos / pred must have one entry per act row")
        if not 1 <= n <= self._freq.batch:
            raise ValueError("a batch holds 1 .. batch_rows rows of an open run")
        status, opened = np.empty(n, np.int32), np.zeros(n, np.int32)
        rc = self._lib.ds_freq_push(self._h, n, chrom.ctypes.data, pos.ctypes.data, act.ctypes.data, act.shape[1], pred.ctypes.data,
                                    status.ctypes.data, opened.ctypes.data)
        self._check_memory(rc, "ds_freq_push")
        self._freq.pending, self._freq.opened = n, opened        # the library fills `opened` when the batch is accumulated
        return status

    def freq_values(self, act) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
        """ds_freq_values: freq_values_kernel alone over act rows -> (p0, p1, status); what freq_values_reference gives on the CPU."""
        act = _act_rows(act)
        n = act.shape[0]
        p0, p1, status = np.zeros(n, np.float64), np.zeros(n, np.float64), np.zeros(n, np.int32)
        self._check(self._lib.ds_freq_values(self._h, n, act.ctypes.data, act.shape[1], p0.ctypes.data, p1.ctypes.data,
                                             status.ctypes.data), "ds_freq_values")
        return p0, p1, status

    def freq_stream_times(self, reset: bool = False) -> dict:
        """ds_get_freq_stream_times: device milliseconds of freq_values_kernel and of the table growths, and their number."""
        return self._times(self._lib.ds_get_freq_stream_times, "ds_get_freq_stream_times", ("values_ms", "rehash_ms"), ("growths",), reset)

    def freq_parse(self, text, begin, end, chrom, flags) -> np.ndarray:
        """ds_freq_parse: one batch of rows (ascending spans of one buffer; chrom / flags per row as freq_locate gives them, the
        ids mapped to one numbering for the whole run) parsed on the GPU -> the per-row status (TEXT_ROW_OK / TEXT_ROW_HOST)."""
        return self._run_parse(self._freq, self._lib.ds_freq_parse, "ds_freq_parse", text, begin, end, chrom, flags)

    def freq_accumulate(self, rows=(), chrom=(), pos=(), p0=(), p1=(), met=()) -> Optional[np.ndarray]:
        """ds_freq_accumulate: add the batch just parsed (or pushed) to the run. rows .. met: the caller's values for the batch's
        TEXT_ROW_HOST rows (ascending batch row indices, every such row; 0 <= chrom < 2^23, 0 <= pos < 2^40). After freq_push:
        returns int32[n], 1 where the row is the first used row of a new site."""
        rows, chrom, met = (np.ascontiguousarray(a, np.int32) for a in (rows, chrom, met))
        pos = np.ascontiguousarray(pos, np.int64)
        p0, p1 = np.ascontiguousarray(p0, np.float64), np.ascontiguousarray(p1, np.float64)
        m = int(rows.size)
        if any(a.shape != (m,) for a in (chrom, pos, p0, p1, met)):
            raise ValueError("the override arrays must have one length")
        self._run_batch(self._freq, "freq", rows)
        if m and (int(chrom.min()) < 0 or int(chrom.max()) >= FREQ_CHROM_LIMIT or int(pos.min()) < 0 or int(pos.max()) >= FREQ_POS_LIMIT):
            raise ValueError("override chromosome ids / positions must fit the key (2^23 ids, pos < 2^40)")
        self._freq.pending = -1
        # the library holds the address of `opened` until it has accumulated the batch or the run ends: so does this object
        opened = self._freq.opened
        self._check(self._lib.ds_freq_accumulate(self._h, m, rows.ctypes.data, chrom.ctypes.data, pos.ctypes.data, p0.ctypes.data,
                                                 p1.ctypes.data, met.ctypes.data), "ds_freq_accumulate")
        self._freq.opened = None
        return opened

    def freq_result(self) -> Dict[str, np.ndarray]:
        """ds_freq_result: the sites of the run so far, in no particular order -> first_row, chrom, pos, sum0, sum1, met, unmet
        arrays, and the scalars rows (accumulated) and used (rows that passed the threshold)."""
        rows, used = ctypes.c_int64(), ctypes.c_int64()
        out = self._sites_result(self._lib.ds_freq_result, "ds_freq_result", _FREQ_SITE_FIELDS, rows, used)
        out.update(rows=int(rows.value), used=int(used.value))
        return out

    def freq_end(self) -> None:
        self._freq.end()
        self._check(self._lib.ds_freq_end(self._h), "ds_freq_end")
        self._freq.opened = None

    def freq_times(self, reset: bool = False) -> dict:
        """ds_get_freq_times: device milliseconds of the frequency batches so far (copies, parse kernel, sort, insert + accumulate)."""
        return self._times(self._lib.ds_get_freq_times, "ds_get_freq_times", ("copy_ms", "parse_ms", "sort_ms", "accumulate_ms"), reset=reset)

    # -- both strands of a CpG table combined on the device (ds_combine_*; combine_strands --on gpu) ----------
    def combine_begin(self, form: int, rec_len, total_rows: int, batch_rows: int) -> None:
        """ds_combine_begin: open a run over the records whose lengths are rec_len (the bitmap holds one bit per base), with
        total_rows rows in all in batches of at most batch_rows. FreqNoMemory when the bitmap, the table or the buffers do not fit
        the device. Needs no weights."""
        rec_len = np.ascontiguousarray(rec_len, np.int64)
        form = int(form)
        if form not in (COMBINE_TABLE, COMBINE_BED):
            raise ValueError("form must be COMBINE_TABLE or COMBINE_BED")
        if rec_len.ndim != 1 or not 1 <= rec_len.size <= FREQ_CHROM_LIMIT or int(rec_len.min()) < 0 or int(rec_len.max()) > FREQ_POS_LIMIT:
            raise ValueError("rec_len must hold 1 .. 2^23 lengths in [0, 2^40]")
        total_rows, batch_rows = _run_sizes(total_rows, batch_rows, 0)
        rc = self._lib.ds_combine_begin(self._h, form, rec_len.size, rec_len.ctypes.data, total_rows, batch_rows)
        self._check_memory(rc, "ds_combine_begin")
        self._combine.begin(batch_rows, words=(int(rec_len.sum()) + 31) // 32)

    def combine_genome(self, text, seg_begin, seg_end, seg_bit, seg_carry) -> None:
        """ds_combine_genome: one chunk of the FASTA (segments ascending and disjoint, at most 2^30 bytes from the first begin to the
        last end) through motif_bitmap_kernel into the run's bitmap."""
        keep, addr, seg_begin, seg_end, seg_bit, seg_carry = _segment_args(text, seg_begin, seg_end, seg_bit, seg_carry)
        if seg_begin.size < 1:
            raise ValueError("a chunk holds at least one segment")
        rc = self._lib.ds_combine_genome(self._h, addr, seg_begin.size, seg_begin.ctypes.data, seg_end.ctypes.data, seg_bit.ctypes.data,
                                         seg_carry.ctypes.data)
        self._check_memory(rc, "ds_combine_genome")

    def combine_bitmap(self) -> np.ndarray:
        """ds_combine_bitmap: the run's bitmap, uint32[(bases + 31) // 32]; what motif_reference gives on the CPU."""
        out = np.zeros(self._combine.words, np.uint32)
        self._check(self._lib.ds_combine_bitmap(self._h, out.size, out.ctypes.data if out.size else None), "ds_combine_bitmap")
        return out

    def combine_parse(self, text, begin, end, chrom, flags) -> np.ndarray:
        """ds_combine_parse: one batch of rows (ascending spans of one buffer; chrom = the record column 0 names, -1 for none; flags
        as freq_locate gives them) -> the per-row status (TEXT_ROW_OK / TEXT_ROW_HOST / COMBINE_ROW_SKIP)."""
        return self._run_parse(self._combine, self._lib.ds_combine_parse, "ds_combine_parse", text, begin, end, chrom, flags)

    def combine_accumulate(self, rows=(), given=()) -> None:
        """ds_combine_accumulate: add the batch just parsed to the run. rows: the ascending batch indices of every TEXT_ROW_HOST
        row; given: per such row None (its key is no CG) or (record, pos, plus, a, b, met, unmet, cov)."""
        rows = np.ascontiguousarray(rows, np.int32)
        m = int(rows.size)
        if len(given) != m:
            raise ValueError("one entry of `given` per override row")
        self._run_batch(self._combine, "combine", rows)
        status = np.array([COMBINE_ROW_SKIP if v is None else TEXT_ROW_OK for v in given], np.int32)
        vals = [(0, 0, 0, 0.0, 0.0, 0, 0, 0) if v is None else v for v in given]
        if any(abs(int(c)) >= COMBINE_COUNT_LIMIT for v in vals for c in v[5:8]):
            raise ValueError("override counts must be below 2^32 in magnitude")
        cols = [np.ascontiguousarray([v[k] for v in vals], dt) for k, dt in enumerate((np.int32, np.int64, np.int32, np.float64, np.float64,
                                                                                         np.int64, np.int64, np.int64))]
        self._combine.pending = -1
        self._check(self._lib.ds_combine_accumulate(self._h, m, rows.ctypes.data, status.ctypes.data, *(c.ctypes.data for c in cols)),
                    "ds_combine_accumulate")

    def combine_result(self) -> Dict[str, np.ndarray]:
        """ds_combine_result: the sites of the run so far, in no particular order -> chrom, pos, sum0, sum1, met, unmet, cov,
        last_plus arrays, and the scalar rows (accumulated)."""
        rows = ctypes.c_int64()
        out = self._sites_result(self._lib.ds_combine_result, "ds_combine_result", _COMBINE_SITE_FIELDS, rows)
        out.update(rows=int(rows.value))
        return out

    def combine_end(self) -> None:
        self._combine.end()
        self._check(self._lib.ds_combine_end(self._h), "ds_combine_end")

    def combine_times(self, reset: bool = False) -> dict:
        """ds_get_combine_times: device milliseconds of the combine runs so far (copies, motif kernel, parse kernel, sort, insert +
        accumulate), the genome chunks and the batches."""
        return self._times(self._lib.ds_get_combine_times, "ds_get_combine_times", ("copy_ms", "motif_ms", "parse_ms", "sort_ms", "accumulate_ms"),
                           ("chunks", "batches"), reset)

    # -- call accuracy and AUROC of labelled call rows on the device (ds_eval_*; evaluate --on gpu) ----------
    def eval_begin(self, total_rows: int, batch_rows: int, cf) -> None:
        """ds_eval_begin: open a run of total_rows rows in all in batches of at most batch_rows, with the cut-offs cf (1 .. 32
        doubles). FreqNoMemory when the score table or the buffers do not fit the device. Needs no weights."""
        cf = _eval_cutoffs(cf)
        total_rows, batch_rows = _run_sizes(total_rows, batch_rows)
        rc = self._lib.ds_eval_begin(self._h, total_rows, batch_rows, cf.size, cf.ctypes.data)
        self._check_memory(rc, "ds_eval_begin")
        self._eval.begin(batch_rows, ncf=int(cf.size))

    def eval_parse(self, text, begin, end, flags) -> np.ndarray:
        """ds_eval_parse: one batch of rows (ascending spans of one buffer; flags as eval_locate gives them) -> the per-row status
        (TEXT_ROW_OK / TEXT_ROW_HOST)."""
        return self._run_parse(self._eval, self._lib.ds_eval_parse, "ds_eval_parse", text, begin, end, None, flags)

    def eval_accumulate(self, mask, rows=(), p0=(), p1=(), called=()) -> None:
        """ds_eval_accumulate: add the batch just parsed to the run. mask: a byte per row of the batch (EVAL_SET_SAMPLE |
        EVAL_SET_ALL | EVAL_TRUTH). rows .. called: the caller's values for the batch's TEXT_ROW_HOST rows (ascending batch row
        indices, every such row; called = a non-zero label)."""
        rows = np.ascontiguousarray(rows, np.int32)
        mask = _eval_mask(mask, self._run_batch(self._eval, "eval", rows))
        p0, p1 = np.ascontiguousarray(p0, np.float64), np.ascontiguousarray(p1, np.float64)
        called = np.ascontiguousarray(np.asarray(called) != 0, np.int32)
        m = int(rows.size)
        if not (p0.shape == p1.shape == called.shape == (m,)):
            raise ValueError("one value of each kind per override row")
        self._eval.pending = -1
        self._check(self._lib.ds_eval_accumulate(self._h, mask.ctypes.data, m, rows.ctypes.data, p0.ctypes.data, p1.ctypes.data,
                                                 called.ctypes.data), "ds_eval_accumulate")

    def eval_result(self) -> dict:
        """ds_eval_result: counts int64[2, 4 + 2 ncf] (tp, fp, tn, fn, called per cut-off, correct per cut-off; set 0 the sample, set 1
        all), per set u2 / p / n over the rows with a finite prob_1, and the scalars rows (accumulated) and distinct (scores)."""
        counts, u2, pn, nn = _eval_result(self._eval.ncf)
        rows, distinct = ctypes.c_int64(), ctypes.c_int64()
        self._check(self._lib.ds_eval_result(self._h, counts.ctypes.data, u2.ctypes.data, pn.ctypes.data, nn.ctypes.data, ctypes.byref(rows),
                                             ctypes.byref(distinct)), "ds_eval_result")
        return dict(counts=counts, u2=[int(v) for v in u2], p=[int(v) for v in pn], n=[int(v) for v in nn], rows=int(rows.value),
                    distinct=int(distinct.value))

    def eval_end(self) -> None:
        self._eval.end()
        self._check(self._lib.ds_eval_end(self._h), "ds_eval_end")

    def eval_times(self, reset: bool = False) -> dict:
        """ds_get_eval_times: device milliseconds of the evaluate runs so far (copies, parse kernel, count + insert kernels, the
        result's sort / scan / reduction) and the batches."""
        return self._times(self._lib.ds_get_eval_times, "ds_get_eval_times", ("copy_ms", "parse_ms", "count_ms", "result_ms"), reset=reset)

    def rows_times(self, reset: bool = False) -> dict:
        """ds_get_rows_times: device milliseconds of the extract_rows() calls made while profiling was on."""
        return self._times(self._lib.ds_get_rows_times, "ds_get_rows_times", ("stats_ms", "values_ms", "length_ms", "format_ms", "d2h_ms"), reset=reset)

    # -- cascaded precision (ds_set_recheck) ---------------------------------------------------
    def set_recheck(self, fine: Optional["Engine"], margin: float, own: bool = False) -> None:
        """Attach `fine` (same geometry and device, weights loaded): every site whose result here falls within `margin` of the
        threshold -- |p1 - p0| < margin on the normalised probabilities, or a non-finite result -- is run again on `fine`,
        whose act / pred replace this engine's for that site. run(), submit() / submit_parts() / wait() and submit_reads()
        honour it; run_device() raises while it is attached. `fine` must not be used directly while attached. fine None or
        margin <= 0 detaches. own=True: close() of this engine closes `fine` too."""
        if fine is not None and not isinstance(fine, Engine):
            raise TypeError("fine must be an Engine or None")
        h = fine._h if fine is not None else None
        self._check(self._lib.ds_set_recheck(self._h, h, float(margin)), "ds_set_recheck")
        attached = fine is not None and margin > 0
        self._fine, self._owns_fine = (fine, bool(own)) if attached else (None, False)

    def recheck_stats(self) -> dict:
        """ds_get_recheck_stats since the attachment: sites through this engine, sites rechecked, forwards of the fine engine."""
        a, b, c = ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int64()
        self._check(self._lib.ds_get_recheck_stats(self._h, ctypes.byref(a), ctypes.byref(b), ctypes.byref(c)),
                    "ds_get_recheck_stats")
        return {"sites": int(a.value), "rechecked": int(b.value), "fine_forwards": int(c.value)}

    def recheck_times(self, reset: bool = False) -> dict:
        """ds_get_recheck_times: device milliseconds of the selection kernel over the run() calls made while profiling was on."""
        return self._times(self._lib.ds_get_recheck_times, "ds_get_recheck_times", ("select_ms",), ("launches",), reset)

    def recheck_select(self, act, margin: float) -> np.ndarray:
        """ds_recheck_select (diagnostic): the ascending indices the selection kernel picks for the given act rows."""
        act = np.ascontiguousarray(act, np.float32)
        n = int(act.shape[0])
        count = ctypes.c_int32()
        index = np.empty(n, np.int32)
        self._check(self._lib.ds_recheck_select(self._h, n, act.ctypes.data, float(margin), ctypes.byref(count), index.ctypes.data),
                    "ds_recheck_select")
        return index[:count.value].copy()

    @property
    def slots(self) -> int:
        return self._slots

    # -- diagnostics ---------------------------------------------------------------------------
    def intermediate(self, name: str, shape) -> np.ndarray:
        out = np.empty(shape, np.float32)
        got = self._lib.ds_get_intermediate(self._h, name.encode(), out.ctypes.data, out.size)
        self._check(int(got), "ds_get_intermediate(%s)" % name)
        if got != out.size:
            raise RuntimeError("intermediate %s: expected %d floats, got %d" % (name, out.size, got))
        return out

    def set_profiling(self, mode) -> None:
        """0/False off, 1 per-kernel runs, 2/True per launch (see include/deepsignal_hip.h)."""
        mode = 2 if mode is True else int(mode)
        self._check(self._lib.ds_set_profiling(self._h, mode), "ds_set_profiling")

    def set_graph(self, enable: bool) -> None:
        self._check(self._lib.ds_set_graph(self._h, int(enable)), "ds_set_graph")

    def reset_stage_times(self) -> None:
        self._check(self._lib.ds_reset_stage_times(self._h), "ds_reset_stage_times")

    def stage_times(self) -> List[dict]:
        out = []
        for i in range(self._lib.ds_num_stages(self._h)):
            name = ctypes.create_string_buffer(64)
            launches = ctypes.c_int32()
            ms = ctypes.c_double()
            calls = ctypes.c_int64()
            flops = ctypes.c_double()
            self._check(self._lib.ds_get_stage(self._h, i, name, 64, ctypes.byref(launches), ctypes.byref(ms),
                                               ctypes.byref(calls), ctypes.byref(flops)), "ds_get_stage")
            out.append({"name": name.value.decode(), "launches": launches.value, "total_ms": ms.value,
                        "calls": calls.value, "flops_per_site": flops.value})
        return out

    def kernel_stats(self) -> List[dict]:
        out = []
        for i in range(self._lib.ds_num_kernels(self._h)):
            name = ctypes.create_string_buffer(96)
            launches = ctypes.c_int64()
            ms = ctypes.c_double()
            flops = ctypes.c_double()
            self._check(self._lib.ds_get_kernel_stat(self._h, i, name, 96, ctypes.byref(launches), ctypes.byref(ms),
                                                     ctypes.byref(flops)), "ds_get_kernel_stat")
            out.append({"name": name.value.decode(), "launches": launches.value, "total_ms": ms.value,
                        "flops": flops.value})
        return out
