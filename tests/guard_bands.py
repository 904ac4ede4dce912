"""Guard bands around every caller-owned output of the C ABI (tests/test_gpu_output_extents.py on the GPU,
tests/test_output_extents_host.py on the CPU, tests/test_output_extents_table.py for completeness).

An output buffer is carved out of one allocation of the test's own, laid out

    front band | extent | back band

with every band byte 0xA5 and every extent byte prefilled with 0x5A. A library write outside the stated extent changes a band
byte inside that allocation -- a failed assertion, never a fault -- and an element the contract says is written but is not
keeps its prefill. The bands hold at least `rows_per_band` rows of the output (the tests pass max_batch, so a "max_batch rows
written for n" bug stays inside them) and at least 4096 bytes; the extent starts 256-byte aligned.

`call(lib, "ds_x", ...)` is how the tests reach an entry: it holds the call to EXTENTS, the table of every output parameter
of include/deepsignal_hip.h -- each output named there must be given as a Banded (or None where the header makes it
optional) -- converts the arguments, runs the entry and checks every band.
"""
from __future__ import annotations

import ctypes
import os
import re

import numpy as np

BAND, PREFILL = 0xA5, 0x5A
MIN_BAND_BYTES, ALIGN = 4096, 256
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class Banded:
    """front band | extent | back band inside one allocation. ptr = the address of the extent, view = the extent as an array of
    the asked shape and dtype (numpy on the host, torch on the device), check() = both bands are intact."""

    def __init__(self, shape, dtype, rows_per_band, device=None, what=""):
        shape = (int(shape),) if np.isscalar(shape) else tuple(int(s) for s in shape)
        self.shape, self.dtype, self.device, self.what = shape, np.dtype(dtype), device, what
        row_bytes = self.dtype.itemsize * int(np.prod(shape[1:], dtype=np.int64)) if len(shape) else self.dtype.itemsize
        self.nbytes = self.dtype.itemsize * int(np.prod(shape, dtype=np.int64))
        band = max(int(rows_per_band) * row_bytes, MIN_BAND_BYTES)
        self.band = band = (band + ALIGN - 1) // ALIGN * ALIGN
        total = 2 * band + self.nbytes + ALIGN
        if device is None:
            self._raw = np.empty(total, np.uint8)
            base = self._raw.ctypes.data
        else:
            import torch
            self._raw = torch.empty(total, dtype=torch.uint8, device=device)
            base = self._raw.data_ptr()
        self._lo = (-base) % ALIGN                       # first byte of the front band: the extent then starts aligned
        self._at = self._lo + band
        self.ptr = base + self._at
        assert self.ptr % ALIGN == 0
        self._raw[:] = BAND
        self.refill()
        ext = self._raw[self._at:self._at + self.nbytes]
        if device is None:
            self.view = ext.view(self.dtype).reshape(shape)
        else:
            import torch
            tdt = {"float32": torch.float32, "int32": torch.int32, "uint8": torch.uint8, "int64": torch.int64}[self.dtype.name]
            self.view = ext.view(tdt).reshape(shape)

    def refill(self):
        self._raw[self._at:self._at + self.nbytes] = PREFILL

    def _bytes(self, a, b) -> np.ndarray:
        part = self._raw[a:b]
        return part if self.device is None else part.cpu().numpy()

    def check(self, what=""):
        """Both bands byte for byte intact."""
        what = what or self.what
        for side, a in (("front", self._lo), ("back", self._at + self.nbytes)):
            got = self._bytes(a, a + self.band)
            bad = np.nonzero(got != BAND)[0]
            assert bad.size == 0, "%s: the %s band changed: %d bytes, the first at byte %d of the band (extent %s %s)" % (
                what, side, bad.size, int(bad[0]), self.shape, self.dtype.name)

    def bytes(self) -> np.ndarray:
        """The extent's bytes, on the host."""
        return self._bytes(self._at, self._at + self.nbytes).copy()

    def array(self) -> np.ndarray:
        """The extent as a host numpy array (a copy)."""
        return self.bytes().view(self.dtype).reshape(self.shape)

    def untouched(self) -> bool:
        return bool((self.bytes() == PREFILL).all())

    def written(self, count=None) -> bool:
        """No element of the first `count` (default: all) still holds the prefill pattern in every byte."""
        a = self.bytes().reshape(-1, self.dtype.itemsize)
        a = a if count is None else a[:count]
        return not bool((a == PREFILL).all(axis=1).any())


def banded(shape, dtype, rows_per_band, device=None, what="") -> Banded:
    return Banded(shape, dtype, rows_per_band, device, what)


def scalar(dtype, what="") -> Banded:
    """A scalar out parameter: an extent of one element."""
    return Banded((1,), dtype, 1, None, what)


def same_bytes(b: Banded, want, what="") -> None:
    """The extent equals `want` (what the engine wrapper returned for the same inputs on the same handle) byte for byte."""
    want = np.ascontiguousarray(want)
    got = b.bytes()
    w = want.reshape(-1).view(np.uint8)
    assert got.size == w.size, "%s: extent of %d bytes, reference of %d" % (what or b.what, got.size, w.size)
    bad = np.nonzero(got != w)[0]
    assert bad.size == 0, "%s: the extent differs from the wrapper's result in %d bytes, the first at byte %d" % (
        what or b.what, bad.size, int(bad[0]))


# ---- the header, parsed the way tests/test_abi.py does ---------------------------------------------------------------------------
HANDLE_TYPES = ("ds_handle", "ds_tsv")


def declared_functions():
    """{function: [(parameter name, its text)]} of include/deepsignal_hip.h, comments stripped."""
    text = open(os.path.join(ROOT, "include", "deepsignal_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    out = {}
    for name, params in re.findall(r"\b(ds_[a-z_0-9]+)\s*\(([^()]*)\)\s*;", text):
        plist = []
        for p in params.split(","):
            p = " ".join(p.split())
            if p in ("", "void"):
                continue
            plist.append((re.findall(r"[A-Za-z_][A-Za-z_0-9]*", p)[-1], p))
        out[name] = plist
    return out


def output_params(plist):
    """The non-const pointer parameters of a declaration that are no handle: [(name, text, is a handle out-pointer)]."""
    out = []
    for name, p in plist:
        if "*" not in p or "const" in p.split():
            continue
        stars = p.count("*")
        handle = any(p.startswith(t + " ") for t in HANDLE_TYPES)
        if handle and stars == 1:
            continue                                    # the handle an entry works on
        out.append((name, p, handle and stars == 2))
    return out


# ---- the table: every output parameter of the ABI, and where its extent is held ----------------------------------------------------
GPU, HOST = "tests/test_gpu_output_extents.py", "tests/test_output_extents_host.py"
_HANDLE_OUT = "exempt: a handle out-pointer, one pointer written by the constructor"
# a non-const pointer that is no output, so no extent exists: the allocation ds_free_host releases
NOT_OUTPUTS = {("ds_free_host", "p"): "exempt: not an output, the pinned allocation being released"}


def _t(where, names):
    return {n: where for n in names.split()}


EXTENTS = {
    "ds_create": {"out": _HANDLE_OUT},
    "ds_tsv_open": {"out": _HANDLE_OUT},
    "ds_free_host": {"p": NOT_OUTPUTS[("ds_free_host", "p")]},
    # the forward
    "ds_forward": _t(GPU, "act pred"),
    "ds_forward_device": _t(GPU, "d_act d_pred"),
    "ds_submit": _t(GPU, "ticket"),
    "ds_wait": _t(GPU, "act pred"),
    "ds_submit_parts": _t(GPU, "ticket"),
    "ds_submit_reads": _t(GPU, "ticket"),
    "ds_alloc_host": _t(GPU, "out"),
    "ds_get_intermediate": _t(GPU, "out"),
    "ds_get_stage": _t(GPU, "name launches total_ms calls flops_per_site"),
    "ds_get_kernel_stat": _t(GPU, "name launches total_ms flops"),
    # extraction and rows
    "ds_extract": _t(GPU, "kmer means stds sanums signals"),
    "ds_submit_rows": _t(GPU, "ticket"),
    "ds_wait_rows": _t(GPU, "out row_off"),
    "ds_extract_rows": _t(GPU, "out row_off"),
    "ds_format_values": _t(GPU + " (device), " + HOST + " (h == NULL)", "out"),
    "ds_get_rows_times": _t(GPU, "batches ms"),
    "ds_extract_reference": _t(HOST, "kmer means stds sanums signals"),
    "ds_extract_rows_reference": _t(HOST, "out row_off"),
    "ds_format_rows": _t(HOST, "out"),
    "ds_tsv_parse_into": _t(HOST, "kmer means stds lens signals labels"),
    "ds_tsv_take_lines": _t(HOST, "begin end"),
    # recheck
    "ds_get_recheck_stats": _t(GPU, "sites rechecked fine_forwards"),
    "ds_get_recheck_times": _t(GPU, "launches ms"),
    "ds_recheck_select": _t(GPU, "count index"),
    # text
    "ds_submit_text": _t(GPU, "ticket"),
    "ds_wait_text": _t(GPU, "act pred kmer labels info info_off"),
    "ds_parse_text": _t(GPU, "kmer means stds lens signals labels info_len status"),
    "ds_parse_text_reference": _t(HOST, "kmer means stds lens signals labels info_len status"),
    "ds_get_text_stats": _t(GPU, "rows host_rows"),
    "ds_get_text_times": _t(GPU, "batches ms"),
    # frequency
    "ds_freq_locate": _t(HOST, "row_begin row_end chrom flags names names_bytes n_names"),
    "ds_freq_keys": _t(HOST, "chrom pos flags names names_bytes n_names"),
    "ds_freq_reference": _t(HOST, "status pos p0 p1 met first_row site_chrom site_pos sum0 sum1 site_met site_unmet used"),
    "ds_freq_values_reference": _t(HOST, "p0 p1 status"),
    "ds_freq_parse": _t(GPU, "status"),
    "ds_freq_result": _t(GPU, "first_row chrom pos sum0 sum1 met unmet rows used"),
    "ds_freq_push": _t(GPU, "status opened"),
    "ds_freq_values": _t(GPU, "p0 p1 status"),
    "ds_get_freq_times": _t(GPU, "batches ms"),
    "ds_get_freq_stream_times": _t(GPU, "growths ms"),
    # combine
    "ds_fasta_locate": _t(HOST, "line_begin line_end line_rec line_off name_begin name_end rec_len n_recs flags"),
    "ds_motif_reference": _t(HOST, "bitmap"),
    "ds_combine_reference": _t(HOST, "chrom status pos plus a b met unmet cov site_chrom site_pos sum0 sum1 site_met site_unmet site_cov "
                                     "last_plus"),
    "ds_combine_bitmap": _t(GPU, "bitmap"),
    "ds_combine_parse": _t(GPU, "status"),
    "ds_combine_result": _t(GPU, "chrom pos sum0 sum1 met unmet cov last_plus rows"),
    "ds_get_combine_times": _t(GPU, "chunks batches ms"),
    # evaluate
    "ds_eval_locate": _t(HOST, "row_begin row_end flags file_flags"),
    "ds_eval_reference": _t(HOST, "status p0 p1 called counts u2 pn nn"),
    "ds_eval_parse": _t(GPU, "status"),
    "ds_eval_result": _t(GPU, "counts u2 pn nn rows distinct"),
    "ds_get_eval_times": _t(GPU, "batches ms"),
    # training
    "ds_train_step": _t(GPU, "loss pred"),
    "ds_train_step_base": _t(GPU, "loss pred"),
    "ds_train_eval": _t(GPU, "loss pred logits"),
    "ds_train_step_signal": _t(GPU, "loss pred"),
    "ds_train_eval_signal": _t(GPU, "loss pred logits"),
    "ds_train_get_tensor": _t(GPU, "out"),
    "ds_train_get_grad": _t(GPU, "out"),
    "ds_train_get_mask": _t(GPU, "out"),
    "ds_train_get_tap": _t(GPU, "out"),
    "ds_get_train_times": _t(GPU, "steps ms"),
    "ds_train_mask_reference": _t(HOST, "out"),
    "ds_train_mask_reference_wide": _t(HOST, "out"),
}

_DECLARED = None


def _positions(name):
    """[(argument index, parameter name)] of the outputs EXTENTS lists for an entry."""
    global _DECLARED
    if _DECLARED is None:
        _DECLARED = declared_functions()
    plist = _DECLARED[name]
    return [(i, p) for i, (p, _) in enumerate(plist) if p in EXTENTS[name] and not EXTENTS[name][p].startswith("exempt")]


def call(lib, name, *args):
    """Run entry `name` with `args`; every output parameter of EXTENTS[name] must be a Banded, or None where the header makes
    the output optional. Every band is checked after the call. Returns the entry's return value."""
    fn = getattr(lib, name)
    argtypes = fn.argtypes
    assert argtypes is not None and len(argtypes) == len(args), "%s takes %d arguments" % (name, len(argtypes or ()))
    outs = dict(_positions(name))
    conv, bands = [], []
    for i, a in enumerate(args):
        if i in outs:
            assert a is None or isinstance(a, Banded), "%s: output %s must be banded" % (name, outs[i])
        if isinstance(a, Banded):
            assert i in outs, "%s: argument %d is no output in the table" % (name, i)
            a.what = a.what or "%s(%s)" % (name, outs[i])
            bands.append(a)
            t = argtypes[i]
            if t is ctypes.c_void_p:
                a = a.ptr
            elif t is ctypes.c_char_p:
                a = ctypes.cast(ctypes.c_void_p(a.ptr), ctypes.c_char_p)
            else:
                a = ctypes.cast(ctypes.c_void_p(a.ptr), t)
        conv.append(a)
    rc = fn(*conv)
    for b in bands:
        b.check()
    return rc
