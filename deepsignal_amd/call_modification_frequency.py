"""Per-site modification frequency from call_mods result files — scope row f4 (the step after the
path; what users actually consume). Same algorithm, flags and output formats as the reference script
(/root/reference/scripts/call_modification_frequency.py:16-78, scripts/txt_formater.py:8-46):
group calls by (chromosome, pos), keep a call if |prob_0 - prob_1| >= prob_cf, accumulate prob sums,
met / unmet counts and coverage, write the 11-column table or bedMethyl.

`call_mods --freq_file` (FreqStream) computes the table from the forward's results as call_mods has them, with no result text
written or parsed in between; it shares the device kernels and the host-row expressions with `--on gpu`.

`--on gpu` (calculate_mods_frequency_gpu) computes the same SiteStats on the MI355X: the host only finds the rows and numbers
the chromosomes (ds_freq_locate), the device parses and aggregates them (csrc/ds_freq.hip), and the rows in a form the device
does not parse go through the expressions of the cpu route right here. The table is byte-identical to `--on cpu`.
"""
from __future__ import annotations

import argparse
import gzip
import os
import sys
from typing import Dict, Iterable, List, Tuple

from . import table_route as tr
from .table_route import _CpuRoute      # noqa: F401 -- the name call_modifications.py and the tests catch it under


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


class _CallFile(tr.RowFile):
    """One input file of the gpu route: its bytes (memory map, or the gunzipped text), row spans, chromosome ids, flags."""

    def __init__(self, path: str, chrom_id):
        from . import engine as eng
        import numpy as np
        tr.RowFile.__init__(self, path, gunzip=True)
        begin, end, local, flags, names = eng.freq_locate(self.data)
        self.set_rows(begin, end, flags)
        # the file's ids -> the run's (names of unflagged rows are ASCII)
        to_run = np.array([chrom_id(n.decode("ascii")) for n in names] + [-1], np.int32)
        self.chrom = to_run[local]               # -1 (a flagged row) picks the -1 at the end


def _host_row_values(w: List[str], prob_cf: float, chrom_id, used_w: dict, row: int):
    """One row `w` the device left to Python, through the expressions of the cpu route -> what ds_freq_accumulate takes for it:
    (chromosome id, pos, prob_0, prob_1, met). A row that passes the threshold (the device makes the same comparison on these
    doubles) is used: its key is looked up -- chrom_id(name), or chrom_id((name, pos)) with pos 0 for a position outside the key: a
    site under an id of its own -- and used_w[row] = w. Shared by `call_freq --on gpu` and `call_mods --freq_file`."""
    from . import engine as eng
    prob_0, prob_1 = float(w[6]), float(w[7])
    cid, pos, met = 0, 0, 0
    if not abs(prob_0 - prob_1) < prob_cf:
        name, pos = w[0], int(w[1])
        if 0 <= pos < eng.FREQ_POS_LIMIT:
            cid = chrom_id(name)
        else:
            cid, pos = chrom_id((name, pos)), 0
        met = 1 if int(w[8]) == 1 else 0
        used_w[row] = w
    return cid, pos, prob_0, prob_1, met


def _chrom_table():
    """names: chromosome id -> its name, or (name, pos) for a site whose position does not fit the key; chrom_id(name) numbers them
    in first-appearance order."""
    from . import engine as eng
    names: list = []
    ids: dict = {}

    def chrom_id(name):
        i = ids.get(name)
        if i is None:
            i = ids[name] = len(names)
            names.append(name)
            if i >= eng.FREQ_CHROM_LIMIT:
                raise _CpuRoute("more than 2^23 chromosome names")
        return i

    return names, chrom_id


def _print_used(host_rows: int, used: int, total: int) -> None:
    if host_rows:
        print("{} row(s) parsed on the host (a form the device does not take)..".format(host_rows))
    print("{:.2f}% ({} of {}) calls used..".format(used / float(total) * 100 if total else 0.0, used, total))


_KMER_BASES = b"ACGTN"


class FreqStream:
    """`call_mods --freq_file`: calculate_mods_frequency over the rows call_mods writes (or would write), fed with what the rows
    are made from -- sampleinfo, the forward's act rows, pred and the k-mer codes, exactly the arguments of fastio.format_rows --
    in result-file order. No row text is made or parsed: the keys come from ds_freq_keys, the two doubles float() would read from
    the printed probabilities from freq_values_kernel, the sums from the kernels of `call_freq --on gpu` on a table that grows. A row
    the device leaves to Python (a flagged sampleinfo, NaN, a probability below ~1e-14) is formatted on its own and read by the cpu
    route's expressions. finish() returns the dict calculate_mods_frequency gives on the text, in the same order.
    _CpuRoute: the stream cannot go on (the message says why); the caller runs the cpu route over the result file or gives up.
    make_engine: what provides freq_begin_stream .. freq_end (default: an Engine of its own on `device`, never the forward's)."""

    def __init__(self, prob_cf: float = 0.0, device: int = 0, batch_rows: int = 1 << 16, initial_slots: int = 1 << 16, make_engine=None):
        tr.check_batch_rows(batch_rows)
        if prob_cf != prob_cf:
            raise ValueError("prob_cf must not be NaN")
        self.prob_cf, self.batch_rows = prob_cf, batch_rows
        self.names, self.chrom_id = _chrom_table()
        self.rows = self.host_rows = 0
        self._buf, self._nbuf = [], 0                        # rows pushed, not yet on the device
        self.first: Dict[int, Tuple[str, int, str]] = {}     # a site's first used row -> its strand, pos_in_strand, k-mer
        self.info: dict = {}
        # a handle of its own, the smallest there is: the forward's handle is busy on another thread
        self.e = tr.open_engine(make_engine, device)
        try:
            with tr.fits("the site table does not fit the device"):
                self.e.freq_begin_stream(initial_slots, batch_rows, prob_cf)
        except BaseException:
            self.close()
            raise

    def push(self, info, info_off, act, pred, kmer) -> None:
        """The rows format_rows(info, info_off, act, pred, kmer) would print, in that order. They are copied and go to the device
        batch_rows at a time (the writer hands over a few thousand rows at once; a device batch of 65,536 rows costs a fixed ~140 kernel launches, 136 of them the bitonic network's)."""
        import numpy as np
        n = int(len(pred))
        if not n:
            return
        off = np.asarray(info_off, np.int64)
        self._buf.append((np.array(np.asarray(info, np.uint8)[int(off[0]):int(off[n])]), np.diff(off[:n + 1]), np.array(act, np.float32),
                          np.array(pred, np.int32), np.array(kmer, np.int32)))
        self._nbuf += n
        if self._nbuf >= self.batch_rows:
            self._flush(self.batch_rows)

    def _flush(self, full: int = 0) -> None:
        """Batches of `full` rows from the buffer while it holds that many; full == 0: everything."""
        import numpy as np
        if not self._nbuf:
            return
        info, lens, act, pred, kmer = (np.concatenate([b[j] for b in self._buf]) for j in range(5))
        off = np.zeros(self._nbuf + 1, np.int64)
        np.cumsum(lens, out=off[1:])
        self._buf, done = [], 0
        while self._nbuf - done >= max(full, 1):
            t = min(self._nbuf, done + (full or self.batch_rows))
            self._batch(info, off[done:t + 1], act[done:t], pred[done:t], kmer[done:t])
            done = t
        if done < self._nbuf:
            self._buf = [(info[int(off[done]):], lens[done:], act[done:], pred[done:], kmer[done:])]
        self._nbuf -= done

    def _batch(self, info, off, act, pred, kmer) -> None:
        import numpy as np
        from . import engine as eng
        from . import fastio
        n = int(len(pred))
        if self.rows + n > eng.FREQ_MAX_ROWS:
            raise _CpuRoute("more than 2^30 rows")
        local, pos, flags, names = eng.freq_keys(info, off)
        to_run = np.array([self.chrom_id(nm.decode("ascii")) for nm in names] + [-1], np.int32)
        with tr.fits("the site table cannot grow on the device"):
            status = self.e.freq_push(to_run[local], pos, act, pred)
        host_w: Dict[int, List[str]] = {}

        def host_row(i: int, _status: int):
            row = fastio.format_rows(info, off[i:i + 2], act[i:i + 1], pred[i:i + 1], kmer[i:i + 1])
            return _host_row_values(tr.python_row(row[:-1]), self.prob_cf, self.chrom_id, host_w, i)

        o_row, values = tr.host_values(status, host_row)
        opened = self.e.freq_accumulate(o_row, *tr.columns(values, 5))
        self.host_rows += len(o_row)
        # the rows that open a site: their strand, pos_in_strand and k-mer (codes -> letters as ds_format_rows writes them)
        idx = np.flatnonzero(opened)
        codes = np.asarray(kmer, np.int64)[idx]
        K = codes.shape[1] if codes.ndim == 2 else 0
        letters = np.frombuffer(_KMER_BASES, np.uint8)[np.where((codes >= 0) & (codes < 5), codes, 4)].tobytes().decode("ascii")
        base, blob, offs = int(off[0]), np.asarray(info, np.uint8)[int(off[0]):int(off[n])].tobytes(), off.tolist()
        for j, i in enumerate(idx.tolist()):
            w = host_w.get(i)
            if w is None:
                c = blob[offs[i] - base:offs[i + 1] - base].decode("ascii").split("\t")
                w2, w3, w9 = c[2], c[3], letters[j * K:(j + 1) * K]
            else:
                w2, w3, w9 = w[2], w[3], w[9]
            self.first[self.rows + i] = (w2, int(w3), w9)
        self.rows += n

    def finish(self) -> Dict[SiteKey, SiteStats]:
        """The sites in the order of their first used row, and the "calls used" line."""
        import numpy as np
        self._flush()
        stream_times = self.e.freq_stream_times() if hasattr(self.e, "freq_stream_times") else {}
        res, times = tr.finish(self.e, "freq")
        self.info.update(times, **stream_times)
        if res["rows"] != self.rows:
            raise RuntimeError("freq stream: %d rows accumulated, %d pushed" % (res["rows"], self.rows))
        stats: Dict[SiteKey, SiteStats] = {}
        for k in np.argsort(res["first_row"], kind="stable").tolist():
            strand, pis, kmer = self.first[int(res["first_row"][k])]
            name = self.names[int(res["chrom"][k])]
            key = name if isinstance(name, tuple) else (name, int(res["pos"][k]))
            st = stats[key] = SiteStats(strand, pis, kmer)
            st.prob_0, st.prob_1 = float(res["sum0"][k]), float(res["sum1"][k])
            st.met, st.unmet = int(res["met"][k]), int(res["unmet"][k])
            st.coverage = st.met + st.unmet
        self.info.update(host_rows=self.host_rows, rows=self.rows, used=res["used"])
        _print_used(self.host_rows, res["used"], self.rows)
        return stats

    def close(self) -> None:
        e, self.e = getattr(self, "e", None), None
        if e is not None:
            e.close()


def calculate_mods_frequency_gpu(mods_files: Iterable[str], prob_cf: float = 0.0, device: int = 0, batch_rows: int = 1 << 20,
                                 info: dict = None, make_engine=None) -> Dict[SiteKey, SiteStats]:
    """calculate_mods_frequency on the GPU: the same dict -- same keys in the same order, same doubles, same counts -- and the
    same "calls used" line. `info`, when given, receives host_rows (rows parsed here because the device does not take their form),
    rows, used, batches and the device times. Raises what the cpu route raises on a malformed row. _CpuRoute: see there.
    make_engine: what provides freq_begin .. freq_end (default: an Engine on `device`; the tests put the CPU checker behind it)."""
    import numpy as np
    from . import engine as eng
    mods_files = list(mods_files)
    tr.check_batch_rows(batch_rows)
    if prob_cf != prob_cf:
        raise ValueError("prob_cf must not be NaN")
    names, chrom_id = _chrom_table()

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
        with tr.small_engine(make_engine, device) as e:
            with tr.fits("the site table of %d rows does not fit the device" % total):
                e.freq_begin(total, min(batch_rows, max(total, 1)), prob_cf)
            base = 0
            for f in files:
                if not isinstance(f, _CallFile):
                    raise f
                host_rows += tr.walk(
                    f.n, batch_rows, lambda s, t: e.freq_parse(f.data, f.begin[s:t], f.end[s:t], f.chrom[s:t], f.flags[s:t]),
                    lambda row, _status: _host_row_values(tr.python_row(f.row_bytes(row)), prob_cf, chrom_id, host_w, base + row),
                    lambda s, t, rows, values: e.freq_accumulate(rows, *tr.columns(values, 5)))
                base += f.n
            res, times = tr.finish(e, "freq")
    else:
        for f in files:
            if not isinstance(f, _CallFile):
                raise f
    if res is not None:
        tr.check_rows(res, total)
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
    _print_used(host_rows, used, total)
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
    ap.add_argument("--combine_ref", type=str, default=None,
                    help="a genome reference (FASTA): after the result file is written, combine its two strands per CpG "
                         "(`combine_strands` on that file, honouring --on / --device) into <name>.fb_combined<ext>")
    ap.add_argument("--combine_contig", type=str, default=None, help="--combine_ref: only this contig (combine_strands --contig)")
    a = ap.parse_args(argv)
    if a.combine_contig is not None and a.combine_ref is None:
        ap.error("--combine_contig needs --combine_ref")
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
    if a.combine_ref is not None:
        from .combine_strands import combine_strands
        combine_strands(a.result_file, a.combine_ref, a.combine_contig or "", None, a.on, a.device or 0)
    return 0


if __name__ == "__main__":
    sys.exit(main())
