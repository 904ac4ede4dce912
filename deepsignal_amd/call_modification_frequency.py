"""Per-site modification frequency from call_mods result files — scope row f4 (the step after the
path; what users actually consume). Same algorithm, flags and output formats as the reference script
(/root/reference/scripts/call_modification_frequency.py:16-78, scripts/txt_formater.py:8-46):
group calls by (chromosome, pos), keep a call if |prob_0 - prob_1| >= prob_cf, accumulate prob sums,
met / unmet counts and coverage, write the 11-column table or bedMethyl.

`--on gpu` (calculate_mods_frequency_gpu) computes the same SiteStats on the MI355X: the host only finds the rows and numbers
the chromosomes (ds_freq_locate), the device parses and aggregates them (csrc/ds_freq.hip), and the rows in a form the device
does not parse go through the expressions of the cpu route right here. The table is byte-identical to `--on cpu`.
"""
from __future__ import annotations

import argparse
import gzip
import io
import mmap
import os
import sys
from typing import Dict, Iterable, List, Tuple


class SiteStats:
    __slots__ = ("strand", "pos_in_strand", "kmer", "prob_0", "prob_1", "met", "unmet", "coverage")

    def __init__(self, strand: str, pos_in_strand: int, kmer: str):
        self.strand, self.pos_in_strand, self.kmer = strand, pos_in_strand, kmer
        self.prob_0 = 0.0
        self.prob_1 = 0.0
        self.met = self.unmet = self.coverage = 0


SiteKey = Tuple[str, int]


def calculate_mods_frequency(mods_files: Iterable[str], prob_cf: float = 0.0) -> Dict[SiteKey, SiteStats]:
    stats: Dict[SiteKey, SiteStats] = {}
    count = used = 0
    for path in mods_files:
        opener = gzip.open(path, "rt") if path.endswith(".gz") else open(path, "r")
        with opener as f:
            for line in f:
                w = line.strip().split("\t")
                prob_0, prob_1 = float(w[6]), float(w[7])
                count += 1
                if abs(prob_0 - prob_1) < prob_cf:
                    continue
                key = (w[0], int(w[1]))
                st = stats.get(key)
                if st is None:
                    st = stats[key] = SiteStats(w[2], int(w[3]), w[9])
                st.prob_0 += prob_0
                st.prob_1 += prob_1
                st.coverage += 1
                if int(w[8]) == 1:
                    st.met += 1
                else:
                    st.unmet += 1
                used += 1
    print("{:.2f}% ({} of {}) calls used..".format(used / float(count) * 100 if count else 0.0, used, count))
    return stats


class _CpuRoute(Exception):
    """--on gpu cannot take this input as it is; the message says why and the cpu route runs instead (never a truncated table)."""


class _CallFile:
    """One input file of the gpu route: its bytes (memory map, or the gunzipped text), row spans, chromosome ids, flags."""

    def __init__(self, path: str, chrom_id):
        from . import engine as eng
        import numpy as np
        self.keep = None
        if path.endswith(".gz"):
            with gzip.open(path, "rb") as f:
                self.data = np.frombuffer(f.read(), np.uint8)
        else:
            with open(path, "rb") as f:
                size = os.fstat(f.fileno()).st_size
                if size:
                    self.keep = mmap.mmap(f.fileno(), 0, access=mmap.ACCESS_READ)
                    self.data = np.frombuffer(self.keep, np.uint8)
                else:
                    self.data = np.zeros(0, np.uint8)
        self.begin, self.end, local, self.flags, names = eng.freq_locate(self.data)
        # the file's ids -> the run's (names of unflagged rows are ASCII)
        to_run = np.array([chrom_id(n.decode("ascii")) for n in names] + [-1], np.int32)
        self.chrom = to_run[local]               # -1 (a flagged row) picks the -1 at the end
        self.n = int(self.begin.size)

    def row_bytes(self, i: int) -> bytes:
        return self.data[int(self.begin[i]):int(self.end[i])].tobytes()


def _python_row(raw: bytes) -> List[str]:
    """A row's bytes -> the `w` of the cpu route: decoded and split into lines by the very text layer open(path, "r") uses, then
    line.strip().split("\t"). A row that holds a line break of its own (a bare carriage return) is more than one line there."""
    lines = list(io.TextIOWrapper(io.BytesIO(raw + b"\n")))
    if len(lines) != 1:
        raise _CpuRoute("a row holds a bare carriage return, which ends a line in Python's text mode")
    return lines[0].strip().split("\t")


def calculate_mods_frequency_gpu(mods_files: Iterable[str], prob_cf: float = 0.0, device: int = 0, batch_rows: int = 1 << 20,
                                 info: dict = None, make_engine=None) -> Dict[SiteKey, SiteStats]:
    """calculate_mods_frequency on the GPU: the same dict -- same keys in the same order, same doubles, same counts -- and the
    same "calls used" line. `info`, when given, receives host_rows (rows parsed here because the device does not take their form),
    rows, used, batches and the device times. Raises what the cpu route raises on a malformed row. _CpuRoute: see there.
    make_engine: what provides freq_begin .. freq_end (default: an Engine on `device`; the tests put the CPU checker behind it)."""
    import numpy as np
    from . import engine as eng
    mods_files = list(mods_files)
    if not 1 <= batch_rows <= eng.FREQ_MAX_BATCH:
        raise ValueError("batch_rows must be in [1, 2^24]")
    if prob_cf != prob_cf:
        raise ValueError("prob_cf must not be NaN")
    names: list = []                  # chromosome id -> its name, or (name, pos) for a site whose position does not fit the key
    ids: dict = {}

    def chrom_id(name):
        i = ids.get(name)
        if i is None:
            i = ids[name] = len(names)
            names.append(name)
            if i >= eng.FREQ_CHROM_LIMIT:
                raise _CpuRoute("more than 2^23 chromosome names")
        return i

    # host pass: every file's rows (the table is sized from their number). A file that cannot be read raises when its turn
    # comes, after the rows of the files in front of it, as on the cpu route.
    files: list = []
    for path in mods_files:
        try:
            files.append(_CallFile(path, chrom_id))
        except _CpuRoute:
            raise
        except Exception as exc:      # noqa: BLE001 -- re-raised below, in file order
            files.append(exc)
            break
    total = sum(f.n for f in files if isinstance(f, _CallFile))
    if total > eng.FREQ_MAX_ROWS:
        raise _CpuRoute("more than 2^30 rows")
    stats: Dict[SiteKey, SiteStats] = {}
    host_w: Dict[int, List[str]] = {}     # global row -> w, for the rows parsed here
    res = None
    times = {}
    host_rows = 0
    if total:
        # the ds_freq_* calls need no weights, but they hang off a handle, and a handle carries the forward's workspace and streams:
        # the smallest one (64 sites, one slot) keeps that cost to a few MB, as `extract --extract_on gpu` does
        e = make_engine() if make_engine is not None else eng.Engine(device=device, max_batch=64, slots=1)
        try:
            try:
                e.freq_begin(total, min(batch_rows, max(total, 1)), prob_cf)
            except eng.FreqNoMemory as exc:
                raise _CpuRoute("the site table of %d rows does not fit the device (%s)" % (total, exc))
            base = 0
            for f in files:
                if not isinstance(f, _CallFile):
                    raise f
                for s in range(0, f.n, batch_rows):
                    t = min(f.n, s + batch_rows)
                    status = e.freq_parse(f.data, f.begin[s:t], f.end[s:t], f.chrom[s:t], f.flags[s:t])
                    o_row, o_chrom, o_pos, o_p0, o_p1, o_met = [], [], [], [], [], []
                    for i in np.flatnonzero(status != eng.TEXT_ROW_OK).tolist():
                        w = _python_row(f.row_bytes(s + i))
                        prob_0, prob_1 = float(w[6]), float(w[7])
                        cid, pos, met = 0, 0, 0
                        if not abs(prob_0 - prob_1) < prob_cf:         # the device makes the same comparison on these doubles
                            name, pos = w[0], int(w[1])
                            if 0 <= pos < eng.FREQ_POS_LIMIT:
                                cid = chrom_id(name)
                            else:                                      # a position outside the key: a site under an id of its own
                                cid, pos = chrom_id((name, pos)), 0
                            met = 1 if int(w[8]) == 1 else 0
                            host_w[base + s + i] = w
                        o_row.append(i); o_chrom.append(cid); o_pos.append(pos); o_p0.append(prob_0); o_p1.append(prob_1); o_met.append(met)
                    e.freq_accumulate(o_row, o_chrom, o_pos, o_p0, o_p1, o_met)
                    host_rows += len(o_row)
                base += f.n
            res = e.freq_result()
            times = e.freq_times()
            e.freq_end()
        finally:
            e.close()
    else:
        for f in files:
            if not isinstance(f, _CallFile):
                raise f
    if res is not None:
        if res["rows"] != total:
            raise RuntimeError("gpu route: %d rows accumulated, %d located" % (res["rows"], total))
        bases = np.cumsum([0] + [f.n for f in files])
        for k in np.argsort(res["first_row"], kind="stable").tolist():
            row = int(res["first_row"][k])
            w = host_w.get(row)
            if w is None:
                fi = int(np.searchsorted(bases, row, side="right")) - 1
                w = files[fi].row_bytes(row - int(bases[fi])).decode("ascii").split("\t")
            name = names[int(res["chrom"][k])]
            key = name if isinstance(name, tuple) else (name, int(res["pos"][k]))
            st = stats[key] = SiteStats(w[2], int(w[3]), w[9])
            st.prob_0, st.prob_1 = float(res["sum0"][k]), float(res["sum1"][k])
            st.met, st.unmet = int(res["met"][k]), int(res["unmet"][k])
            st.coverage = st.met + st.unmet
    used = res["used"] if res is not None else 0
    if info is not None:
        info.update(host_rows=host_rows, rows=total, used=used, **times)
    if host_rows:
        print("{} row(s) parsed on the host (a form the device does not take)..".format(host_rows))
    print("{:.2f}% ({} of {}) calls used..".format(used / float(total) * 100 if total else 0.0, used, total))
    return stats


def write_sitekey2stats(stats: Dict[SiteKey, SiteStats], result_file: str, is_sort: bool, is_bed: bool) -> None:
    keys: List[SiteKey] = sorted(stats) if is_sort else list(stats)
    with open(result_file, "w") as wf:
        for chrom, pos in keys:
            st = stats[(chrom, pos)]
            assert st.coverage == st.met + st.unmet
            if st.coverage <= 0:
                print("{} {} has no coverage..".format(chrom, pos))
                continue
            rmet = float(st.met) / st.coverage
            if is_bed:
                wf.write("\t".join([chrom, str(pos), str(pos + 1), ".", str(st.coverage), st.strand, str(pos),
                                    str(pos + 1), "0,0,0", str(st.coverage), str(int(round(rmet * 100, 0)))]) + "\n")
            else:
                wf.write("%s\t%d\t%s\t%d\t%.3f\t%.3f\t%d\t%d\t%d\t%.4f\t%s\n" % (
                    chrom, pos, st.strand, st.pos_in_strand, st.prob_0, st.prob_1, st.met, st.unmet, st.coverage,
                    rmet, st.kmer))


def collect_input_files(input_paths: List[str], file_uid=None) -> List[str]:
    files = []
    for ipath in input_paths:
        p = os.path.abspath(ipath)
        if os.path.isdir(p):
            for name in os.listdir(p):
                if file_uid is None or name.find(file_uid) != -1:
                    files.append("/".join([p, name]))
        elif os.path.isfile(p):
            files.append(p)
        else:
            raise ValueError("%s is neither a file nor a directory" % ipath)
    return files


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description="calculate frequency of interested sites at genome level")
    ap.add_argument("--input_path", "-i", action="append", type=str, required=True)
    ap.add_argument("--result_file", "-o", type=str, required=True)
    ap.add_argument("--bed", action="store_true", default=False)
    ap.add_argument("--sort", action="store_true", default=False)
    ap.add_argument("--prob_cf", type=float, default=0.0)
    ap.add_argument("--file_uid", type=str, default=None)
    ap.add_argument("--on", default="cpu", choices=["cpu", "gpu"],
                    help="gpu: the rows are parsed and aggregated on the GPU (the host only finds them); the table is "
                         "byte-identical to the cpu route's")
    ap.add_argument("--device", type=int, default=None, help="GPU ordinal of --on gpu (default 0)")
    a = ap.parse_args(argv)
    if a.device is not None and a.on != "gpu":
        ap.error("--device needs --on gpu")
    if a.device is not None and a.device < 0:
        ap.error("--device must be >= 0")
    if a.on == "gpu" and a.prob_cf != a.prob_cf:
        ap.error("--prob_cf must be a number with --on gpu")
    files = collect_input_files(a.input_path, a.file_uid)
    print("get {} input file(s)..".format(len(files)))
    if a.on == "gpu":
        info: dict = {}
        try:
            stats = calculate_mods_frequency_gpu(files, a.prob_cf, a.device or 0, info=info)
        except _CpuRoute as exc:
            print("--on gpu: {}; running the cpu route..".format(exc))
            stats = calculate_mods_frequency(files, a.prob_cf)
    else:
        stats = calculate_mods_frequency(files, a.prob_cf)
    write_sitekey2stats(stats, a.result_file, a.sort, a.bed)
    return 0


if __name__ == "__main__":
    sys.exit(main())
