"""What the gpu routes of call_freq, combine_strands and evaluate share above the engine: a run on the device's site table is opened
on the smallest handle, the input's rows go to it batch by batch, the host gives its own values for the rows the device declines, and
the result is read once. A route keeps only what is its own: how a file is located, what one host row yields, what is printed and
when, and how the result becomes the tool's output."""
from __future__ import annotations

import contextlib
import gzip
import io
import mmap
import os
from typing import Callable, List


class _CpuRoute(Exception):
    """--on gpu cannot take this input as it is; the message says why and the cpu route runs instead (never a truncated table)."""


def map_file(path: str, gunzip: bool = False):
    """(keep-alive object, uint8 array) of a file's bytes: a read-only memory map, or an empty array; gunzip: a path ending in .gz
    is read and decompressed instead."""
    import numpy as np
    if gunzip and path.endswith(".gz"):
        with gzip.open(path, "rb") as f:
            return None, np.frombuffer(f.read(), np.uint8)
    with open(path, "rb") as f:
        if os.fstat(f.fileno()).st_size:
            keep = mmap.mmap(f.fileno(), 0, access=mmap.ACCESS_READ)
            return keep, np.frombuffer(keep, np.uint8)
    return None, np.zeros(0, np.uint8)


class RowFile:
    """One input file of a gpu route: its bytes and, once the route has located them, the row spans and the per-row flags."""

    def __init__(self, path: str, gunzip: bool = False):
        self.keep, self.data = map_file(path, gunzip)

    def set_rows(self, begin, end, flags) -> None:
        self.begin, self.end, self.flags, self.n = begin, end, flags, int(begin.size)

    def row_bytes(self, i: int) -> bytes:
        return self.data[int(self.begin[i]):int(self.end[i])].tobytes()


def python_row(raw: bytes) -> List[str]:
    """A row's bytes -> the `w` of the cpu route: decoded and split into lines by the very text layer open(path, "r") uses, then
    line.strip().split("\\t"). A row that holds a line break of its own (a bare carriage return) is more than one line there."""
    lines = list(io.TextIOWrapper(io.BytesIO(raw + b"\n")))
    if len(lines) != 1:
        raise _CpuRoute("a row holds a bare carriage return, which ends a line in Python's text mode")
    return lines[0].strip().split("\t")


def check_batch_rows(batch_rows: int) -> None:
    from . import engine as eng
    if not 1 <= batch_rows <= eng.FREQ_MAX_BATCH:
        raise ValueError("batch_rows must be in [1, 2^24]")


def open_engine(make_engine, device: int):
    """What provides the run's calls: make_engine(), or an Engine on `device`. The calls need no weights, but they hang off a handle,
    and a handle carries the forward's workspace and streams: the smallest one (64 sites, one slot) keeps that cost to a few MB, as
    `extract --extract_on gpu` does."""
    from . import engine as eng
    return make_engine() if make_engine is not None else eng.Engine(device=device, max_batch=64, slots=1)


@contextlib.contextmanager
def small_engine(make_engine, device: int):
    """open_engine(), closed whatever happens."""
    e = open_engine(make_engine, device)
    try:
        yield e
    finally:
        e.close()


@contextlib.contextmanager
def fits(what: str):
    """The calls that allocate on the device: FreqNoMemory -> _CpuRoute("<what> (<the library's message>)")."""
    from . import engine as eng
    try:
        yield
    except eng.FreqNoMemory as exc:
        raise _CpuRoute("%s (%s)" % (what, exc))


NO_HOST_ROW = object()       # a host_row's answer for a row that is not the host's after all: it is left out


def host_values(status, host_row: Callable):
    """The rows of a batch whose status is not TEXT_ROW_OK, ascending, and host_row(i, status[i]) of each -> (rows, values)."""
    import numpy as np
    from . import engine as eng
    rows, values = [], []
    for i in np.flatnonzero(status != eng.TEXT_ROW_OK).tolist():
        v = host_row(i, int(status[i]))
        if v is not NO_HOST_ROW:
            rows.append(i)
            values.append(v)
    return rows, values


def columns(values: list, k: int) -> List[list]:
    """Tuples of k values each -> k lists."""
    return [list(c) for c in zip(*values)] if values else [[] for _ in range(k)]


def walk(n: int, batch_rows: int, parse: Callable, host_row: Callable, accumulate: Callable) -> int:
    """n rows in batches s:t of at most batch_rows: parse(s, t) -> the batch's statuses, host_row(row, status) for each row (counted
    from the first of the n) the device left to the host, accumulate(s, t, rows, values) with those rows as indices of the batch.
    Returns the number of host rows."""
    host_rows = 0
    for s in range(0, n, batch_rows):
        t = min(n, s + batch_rows)
        rows, values = host_values(parse(s, t), lambda i, st: host_row(s + i, st))
        accumulate(s, t, rows, values)
        host_rows += len(rows)
    return host_rows


def finish(e, route: str):
    """<route>_result, <route>_times and <route>_end of `e` -> (the result, the times)."""
    res, times = getattr(e, route + "_result")(), getattr(e, route + "_times")()
    getattr(e, route + "_end")()
    return res, times


def check_rows(res: dict, located: int) -> None:
    if res["rows"] != located:
        raise RuntimeError("gpu route: %d rows accumulated, %d located" % (res["rows"], located))
