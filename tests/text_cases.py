"""Shared by tests/test_text_parse_reference.py (CPU) and tests/test_gpu_text_parse.py: feature-TSV rows of any geometry, their
byte spans, the host reader's arrays for them, and the device parser's grammar restated in Python (regular expressions and
digit counts, independent of csrc/ds_tsv_device.h)."""
import os
import re

import numpy as np

ARRAYS = ("kmer", "means", "stds", "lens", "signals", "labels")
OK, HOST = 0, 1


def make_rows(n, K, S, seed, sites_per_read=3, fmt="%.6f", label=1):
    """n seeded rows of geometry (K, S) as bytes (no newline); reads of `sites_per_read` consecutive rows."""
    rng = np.random.default_rng(seed)
    rows = []
    for i in range(n):
        kmer = "".join("ACGTN"[c] for c in rng.integers(0, 5, K))
        means = ",".join(fmt % x for x in rng.normal(0, 1, K))
        stds = ",".join(fmt % abs(x) for x in rng.normal(0.2, 0.1, K))
        lens = ",".join(str(int(x)) for x in rng.integers(1, 120, K))
        sig = ",".join(fmt % x for x in rng.normal(0, 1.2, S))
        rows.append("\t".join(["chr%d" % (i % 5), str(1000 + 7 * i), "+-"[i % 2], str(99 - i), "read_%05d" % (i // sites_per_read), "tc"[i % 2],
                               kmer, means, stds, lens, sig, str(label if i % 4 else 1 - label)]).encode())
    return rows


def pack(rows, sep=b"\n"):
    """rows -> (blob, begin, end): the rows joined by `sep` and each row's span in the blob"""
    begin, end, pos = [], [], 0
    for r in rows:
        begin.append(pos)
        end.append(pos + len(r))
        pos += len(r) + len(sep)
    return sep.join(rows) + sep, np.asarray(begin, np.int64), np.asarray(end, np.int64)


def file_lines(data):
    """The rows the native reader hands out for a file's bytes: lines without their '\\r's at the end, blank ones skipped."""
    begin, end, pos = [], [], 0
    for line in data.split(b"\n"):
        e = pos + len(line)
        while e > pos and data[e - 1:e] == b"\r":
            e -= 1
        if e > pos:
            begin.append(pos)
            end.append(e)
        pos += len(line) + 1
    return np.asarray(begin, np.int64), np.asarray(end, np.int64)


def host_arrays(path, K, S):
    """The host reader's arrays of a whole file (+ info_len per row), or None when it refuses the file."""
    from deepsignal_amd import fastio
    rd = fastio.FeatureReader(path, K, S, nthreads=2)
    try:
        items = list(rd.items(1 << 30))
    except ValueError:
        return None
    finally:
        rd.close()
    if not items:
        out = {k: np.zeros((0,), np.float32) for k in ARRAYS}
        out["info_len"] = np.zeros(0, np.int64)
        return out
    out = {k: np.concatenate([getattr(it, k) for it in items]) for k in ARRAYS}
    out["info_len"] = np.concatenate([np.diff(it.info_off) for it in items])
    return out


def host_arrays_of(rows, K, S, tmpdir, name="host.tsv"):
    path = os.path.join(str(tmpdir), name)
    with open(path, "wb") as f:
        f.write(b"\n".join(rows) + b"\n")
    return host_arrays(path, K, S)


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def assert_rows_equal(got, want, rows=None, what=""):
    """Bit for bit (floats as uint32) on the given row indices (default: all)."""
    for k in ARRAYS:
        g, w = bits(got[k]), bits(want[k])
        if rows is not None:
            g, w = g[rows], w[rows]
        assert g.shape == w.shape and np.array_equal(g, w), "%s %s differs" % (what, k)


_FLOAT = re.compile(rb"^-?(?:(\d+)\.?(\d*)|\.(\d+))(?:[eE]([+-]?\d+))?$")
_INT = re.compile(rb"^-?\d{1,9}$")


def float_in_grammar(tok):
    m = _FLOAT.match(tok)
    if not m:
        return False
    ip, fp = (m.group(1), m.group(2)) if m.group(1) is not None else (b"", m.group(3))
    if len((ip + fp).lstrip(b"0")) > 15:
        return False
    ex = int(m.group(4)) if m.group(4) else 0
    return -22 <= ex - len(fp) <= 22


def row_in_grammar(row, K, S):
    """Does the device parse this row itself (status OK)? Otherwise it must flag it for the host (status HOST)."""
    cols = row.split(b"\t")
    if len(cols) < 12:
        return False
    if len(cols[6]) != K or any(c not in b"ACGTN" for c in cols[6]):
        return False
    for c, n, isint in ((7, K, False), (8, K, False), (9, K, True), (10, S, False)):
        toks = cols[c].split(b",")
        if len(toks) != n:
            return False
        if not all(bool(_INT.match(t)) if isint else float_in_grammar(t) for t in toks):
            return False
    return bool(_INT.match(cols[11].rstrip(b"\r ")))
