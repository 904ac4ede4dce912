"""Both strands of a CpG table combined — scope row f5, the last step of the workflow. Same algorithm, flags, output and stdout
as the reference script (/root/reference/scripts/combine_two_strands_frequency.py:6-182): the '-' strand row of each CpG is folded
onto the '+' strand cytosine one base upstream, only positions that are a CG of the reference genome are kept, per position the
sums are taken in row order, and the rows come out sorted by (name, position), every field through str().

`--on cpu` (combine_strands_cpu) keeps the genome as the script does -- one upper-cased string per contig, read through Python's
text layer -- and asks it directly whether a key is a CG (`seq[pos:pos + 2] == "CG"`): no loop over the bases, no entry per CG.

`--on gpu` (combine_strands_gpu) computes the same rows on the MI355X: the host only finds lines and rows (ds_fasta_locate,
ds_freq_locate) and decides which records count; the device scans the genome chunk by chunk into one bit per base, parses the rows,
tests their keys against the bitmap and adds each site's rows in row order (csrc/ds_combine.hip). Rows in a form the device does
not parse go through the expressions of the cpu route right here. File and stdout are byte-identical to `--on cpu`."""
from __future__ import annotations

import argparse
import os
import sys
from typing import Callable, Dict, List, Optional, Tuple

from . import table_route as tr
from .table_route import _CpuRoute

MOTIF = "CG"
MSG_GENOME = "start to get genome reference info.."
MSG_MOTIF = "start to get motif poses in genome reference.."
MSG_COMBINE = "start to combine forward backward strands.."
MSG_SKIP = "{}, not in selected motif poses of the genome"


def is_bed(report_fp: str) -> bool:
    """The reference's rule: the path ends in .bed (any case) -> bedMethyl, anything else -> the 11-column table."""
    return str(report_fp).lower().endswith(".bed")


def default_output(report_fp: str) -> str:
    fname, fext = os.path.splitext(report_fp)
    return fname + ".fb_combined" + fext


# ---- the cpu route ----------------------------------------------------------------------------------------------------------
def read_contigs(ref_fp: str) -> Dict[str, str]:
    """name -> upper-cased sequence, in the order and with the replacements of the script's DNAReference: a record with an empty
    name or an empty sequence is dropped unless it is the file's last, a later record of a name replaces the earlier one."""
    contigs: Dict[str, str] = {}
    name, parts = "", []
    with open(ref_fp, "r") as rf:
        for line in rf:
            if line.startswith(">"):
                seq = "".join(parts)
                if name != "" and seq != "":
                    contigs[name] = seq
                name, parts = line.strip()[1:].split(" ")[0], []
            else:
                parts.append(line.strip().upper())
    contigs[name] = "".join(parts)
    return contigs


def _select(contigs: dict, contig: str) -> dict:
    """--contig NAME: that contig alone (KeyError when the genome has none of that name); '' = all."""
    return contigs if contig == "" else {contig: contigs[contig]}


def _table_values(w: List[str]):
    return float(w[4]), float(w[5]), int(w[6]), int(w[7]), int(w[8])


def _bed_values(w: List[str]):
    return int(w[9]), float(w[10]) / 100 * int(w[9])


def _read_row(w: List[str], bed: bool, in_motif: Callable[[str, int], bool]):
    """One row `w` in the script's order of evaluation -> None (its key is no CG of the genome: the caller prints the script's
    line) or (name, pos, plus, values); raises what the script raises on a malformed row. Shared by the cpu route and the gpu
    route's host rows."""
    name, pos = w[0], int(w[1])
    minus = w[5 if bed else 2] == "-"
    if minus:
        pos -= 1
    if not in_motif(name, pos):
        return None
    if bed:
        return name, pos, not minus, _bed_values(w)
    kmer = None if minus else w[10]
    return name, pos, not minus, _table_values(w) + (kmer,)


def _finish_table(info: Dict[Tuple[str, int], list]) -> list:
    rows = []
    for (name, pos), (p0, p1, met, unmet, cov, kmer) in info.items():
        if cov == 0:
            continue
        rows.append([name, pos, "+", pos, p0, p1, met, unmet, cov, float(met) / cov, kmer])
    return sorted(rows, key=lambda x: (x[0], x[1]))


def _finish_bed(info: Dict[Tuple[str, int], list]) -> list:
    rows = []
    for (name, pos), (cov, met) in info.items():
        if cov == 0:
            continue
        rmet = float(met) / cov
        rows.append([name, pos, pos + 1, ".", cov, "+", pos, pos + 1, "0,0,0", cov, int(round(rmet, 2) * 100)])
    return sorted(rows, key=lambda x: (x[0], x[1]))


def combine_strands_cpu(report_fp: str, ref_fp: str, contig: str = "") -> list:
    """The rows of the combined table, and the script's stdout."""
    print(MSG_GENOME)
    contigs = read_contigs(ref_fp)
    print(MSG_MOTIF)
    contigs = _select(contigs, contig)

    def in_motif(name: str, pos: int) -> bool:
        seq = contigs.get(name)
        return seq is not None and pos >= 0 and seq[pos:pos + 2] == MOTIF

    print(MSG_COMBINE)
    bed = is_bed(report_fp)
    info: Dict[Tuple[str, int], list] = {}
    with open(report_fp, "r") as rf:
        for line in rf:
            w = line.strip().split("\t")
            got = _read_row(w, bed, in_motif)
            if got is None:
                print(MSG_SKIP.format(w))
                continue
            name, pos, plus, v = got
            if bed:
                st = info.setdefault((name, pos), [0, 0.0])
                st[0] += v[0]
                st[1] += v[1]
            else:
                st = info.setdefault((name, pos), [0.0, 0.0, 0, 0, 0, "-"])
                if plus:
                    st[5] = v[5]
                for k in range(5):
                    st[k] += v[k]
    return _finish_bed(info) if bed else _finish_table(info)


def write_rows(rows: list, out_fp: str) -> None:
    with open(out_fp, "w") as wf:
        for r in rows:
            wf.write("\t".join(map(str, r)) + "\n")


# ---- the gpu route ----------------------------------------------------------------------------------------------------------
class _Genome:
    """The host's view of a FASTA for the gpu route: which records count, their lines, and the bases of a few positions (the rows
    the device leaves to Python). Nothing here looks at every base: that is the device's part."""

    def __init__(self, ref_fp: str):
        import numpy as np
        from . import engine as eng
        self.keep, self.data = tr.map_file(ref_fp)
        loc = eng.fasta_locate(self.data)
        if loc["flags"] & eng.FASTA_NON_ASCII:
            raise _CpuRoute("the FASTA holds a byte >= 0x80, which Python's text layer may read as another character")
        if loc["flags"] & eng.FASTA_BARE_CR:
            raise _CpuRoute("the FASTA holds a bare carriage return, which ends a line in Python's text mode")
        self.loc = loc
        nrec = len(loc["rec_len"])
        blob = self.data
        # the dict the script builds: name -> raw record, a later record of a name takes the place (not the position) of the earlier
        self.by_name: Dict[str, int] = {}
        for k in range(nrec):
            name = blob[int(loc["name_begin"][k]):int(loc["name_end"][k])].tobytes().decode("ascii")
            if (name != "" and int(loc["rec_len"][k]) > 0) or k == nrec - 1:
                self.by_name[name] = k
        self.np = np

    def select(self, contig: str) -> None:
        """Number the surviving records 0 .. n - 1 in dict order and keep their lines; --contig NAME keeps that one (KeyError)."""
        from . import engine as eng
        np, loc = self.np, self.loc
        if contig != "":
            self.by_name = {contig: self.by_name[contig]}
        raw = np.array(list(self.by_name.values()), np.int64)
        if raw.size > eng.FREQ_CHROM_LIMIT:
            raise _CpuRoute("more than 2^23 contigs")
        self.rec_len = loc["rec_len"][raw]
        if int(self.rec_len.max()) > eng.FREQ_POS_LIMIT:
            raise _CpuRoute("a contig longer than 2^40")
        self.rec_id = {name: i for i, name in enumerate(self.by_name)}
        to_id = np.full(len(loc["rec_len"]), -1, np.int64)
        to_id[raw] = np.arange(raw.size)
        rec_base = np.zeros(raw.size, np.int64)
        np.cumsum(self.rec_len[:-1], out=rec_base[1:])
        line_id = to_id[loc["line_rec"]]
        keep = line_id >= 0
        self.line_id = line_id[keep]
        self.line_begin, self.line_end, self.line_off = loc["line_begin"][keep], loc["line_end"][keep], loc["line_off"][keep]
        self.line_bit = rec_base[self.line_id] + self.line_off
        # the lines of record i are line_first[i] .. line_first[i + 1] (a record's lines lie together, in file order)
        order = np.argsort(self.line_id, kind="stable")
        for a in ("line_id", "line_begin", "line_end", "line_off", "line_bit"):
            setattr(self, a, getattr(self, a)[order])
        self.line_first = np.searchsorted(self.line_id, np.arange(raw.size + 1))

    def base(self, rec: int, pos: int) -> str:
        """Base `pos` of record `rec`, upper-cased; '' outside the record."""
        if not 0 <= pos < int(self.rec_len[rec]):
            return ""
        lo, hi = int(self.line_first[rec]), int(self.line_first[rec + 1])
        k = lo + int(self.np.searchsorted(self.line_off[lo:hi], pos, side="right")) - 1
        return chr(int(self.data[int(self.line_begin[k]) + pos - int(self.line_off[k])])).upper()

    def in_motif(self, name: str, pos: int) -> bool:
        rec = self.rec_id.get(name)
        return rec is not None and self.base(rec, pos) == "C" and self.base(rec, pos + 1) == "G"

    def chunks(self, chunk_bytes: int):
        """The genome as ds_combine_genome takes it: per chunk the segments (begin, end, bit, carry). A line longer than a chunk is
        cut into pieces; a chunk spans at most chunk_bytes bytes of the file. The base in front of a segment is carried in."""
        np = self.np
        order = np.argsort(self.line_begin, kind="stable")           # file order (select() grouped the lines by record)
        lb, le, lbit, loff = self.line_begin[order], self.line_end[order], self.line_bit[order], self.line_off[order]
        if lb.size == 0:
            return
        # the base in front of a line: the last base of the line before it in the file, which is of the same record when line_off > 0
        carry = np.zeros(lb.size, np.uint8)
        carry[1:] = self.data[le[:-1] - 1]
        carry[loff == 0] = 0
        pieces = (le - lb + chunk_bytes - 1) // chunk_bytes
        if int(pieces.max()) > 1:
            idx = np.repeat(np.arange(lb.size), pieces)
            k = np.arange(idx.size) - np.repeat(np.cumsum(pieces) - pieces, pieces)
            sb = lb[idx] + k * chunk_bytes
            se = np.minimum(sb + chunk_bytes, le[idx])
            sbit = lbit[idx] + k * chunk_bytes
            scarry = np.where(k == 0, carry[idx], self.data[np.maximum(sb - 1, 0)])
        else:
            sb, se, sbit, scarry = lb, le, lbit, carry
        s = 0
        while s < sb.size:
            t = max(int(np.searchsorted(se, int(sb[s]) + chunk_bytes, side="right")), s + 1)
            yield sb[s:t], se[s:t], sbit[s:t], np.ascontiguousarray(scarry[s:t], np.uint8)
            s = t


class _Rows(tr.RowFile):
    """The rows of the input table for the gpu route: bytes, spans, flags, and per row the record its column 0 names (-1: none)."""

    def __init__(self, report_fp: str, rec_id: Dict[str, int]):
        import numpy as np
        from . import engine as eng
        tr.RowFile.__init__(self, report_fp)
        begin, end, local, flags, names = eng.freq_locate(self.data)
        self.set_rows(begin, end, flags)
        to_rec = np.array([rec_id.get(n.decode("ascii"), -1) for n in names] + [-1], np.int32)
        self.chrom = to_rec[local]               # -1 (a flagged row) picks the -1 at the end


def combine_strands_gpu(report_fp: str, ref_fp: str, contig: str = "", device: int = 0, batch_rows: int = 1 << 20,
                        chunk_bytes: int = 1 << 26, info: Optional[dict] = None, make_engine=None) -> list:
    """combine_strands_cpu on the GPU: the same rows and the same stdout. The stdout is held back until the run can no longer turn
    to the cpu route, so that a run that does says so and prints nothing twice. `info`, when given, receives host_rows, skipped,
    rows and the device times. Raises what the cpu route raises on a malformed row. _CpuRoute: the input cannot be taken as it
    is; the message says why. make_engine: what provides combine_begin .. combine_end (default: an Engine on `device`; the tests put
    the CPU checkers behind it)."""
    from . import engine as eng
    tr.check_batch_rows(batch_rows)
    if not 1 <= chunk_bytes <= eng.COMBINE_MAX_CHUNK:
        raise ValueError("chunk_bytes must be in [1, 2^30]")
    out: List[str] = []          # the stdout so far
    try:
        rows = _combine_gpu(report_fp, ref_fp, contig, device, batch_rows, chunk_bytes, info, make_engine, out, eng)
    except _CpuRoute:
        raise
    except BaseException:
        _flush(out)
        raise
    _flush(out)
    return rows


def _flush(out: List[str]) -> None:
    if out:
        sys.stdout.write("\n".join(out) + "\n")


def _combine_gpu(report_fp, ref_fp, contig, device, batch_rows, chunk_bytes, info, make_engine, out, eng) -> list:
    bed = is_bed(report_fp)
    out.append(MSG_GENOME)
    genome = _Genome(ref_fp)
    out.append(MSG_MOTIF)
    genome.select(contig)
    out.append(MSG_COMBINE)
    rows = _Rows(report_fp, genome.rec_id)
    if rows.n > eng.FREQ_MAX_ROWS:
        raise _CpuRoute("more than 2^30 rows")
    names = list(genome.rec_id)
    host_w: Dict[int, List[str]] = {}     # global row -> w, for the '+' rows read here
    host_rows, skips = 0, len(out)        # every line of `out` from here on is a skipped row's
    res, times = None, {}

    def host_row(row: int, status: int):
        """What combine_accumulate takes for a row the device did not add: nothing for one it found to be no CG itself."""
        if status == eng.COMBINE_ROW_SKIP:
            out.append(MSG_SKIP.format(rows.row_bytes(row).decode("ascii").split("\t")))
            return tr.NO_HOST_ROW
        w = tr.python_row(rows.row_bytes(row))
        got = _read_row(w, bed, genome.in_motif)
        if got is None:
            out.append(MSG_SKIP.format(w))
            return None
        name, pos, plus, v = got
        counts = (0, 0, v[0]) if bed else v[2:5]
        if any(abs(c) >= eng.COMBINE_COUNT_LIMIT for c in counts):
            raise _CpuRoute("a count of row %d does not fit the device's 64-bit sums" % row)
        if plus and not bed:
            host_w[row] = w
        return (genome.rec_id[name], pos, int(plus)) + ((v[1], 0.0) if bed else v[0:2]) + tuple(counts)

    if rows.n:
        with tr.small_engine(make_engine, device) as e:
            with tr.fits("the genome's bitmap or the table of %d rows does not fit the device" % rows.n):
                e.combine_begin(eng.COMBINE_BED if bed else eng.COMBINE_TABLE, genome.rec_len, rows.n, min(batch_rows, rows.n))
                for sb, se, sbit, scarry in genome.chunks(chunk_bytes):
                    e.combine_genome(genome.data, sb, se, sbit, scarry)
            host_rows = tr.walk(rows.n, batch_rows,
                                lambda s, t: e.combine_parse(rows.data, rows.begin[s:t], rows.end[s:t], rows.chrom[s:t], rows.flags[s:t]),
                                host_row, lambda s, t, o_row, given: e.combine_accumulate(o_row, given))
            res, times = tr.finish(e, "combine")
    if info is not None:
        info.update(host_rows=host_rows, skipped=len(out) - skips, rows=rows.n, **times)
    if res is None:
        return []
    tr.check_rows(res, rows.n)
    table: Dict[Tuple[str, int], list] = {}
    for k in range(len(res["pos"])):
        key = (names[int(res["chrom"][k])], int(res["pos"][k]))
        if bed:
            table[key] = [int(res["cov"][k]), float(res["sum0"][k])]
            continue
        kmer, last = "-", int(res["last_plus"][k])
        if last >= 0:
            w = host_w.get(last)
            kmer = (w if w is not None else rows.row_bytes(last).decode("ascii").split("\t"))[10]
        table[key] = [float(res["sum0"][k]), float(res["sum1"][k]), int(res["met"][k]), int(res["unmet"][k]), int(res["cov"][k]), kmer]
    return _finish_bed(table) if bed else _finish_table(table)


def combine_strands(report_fp: str, ref_fp: str, contig: str = "", out_fp: Optional[str] = None, on: str = "cpu", device: int = 0,
                    info: Optional[dict] = None) -> str:
    """Combine `report_fp` against the genome `ref_fp` and write the table; returns the path written (default: the reference's
    <name>.fb_combined<ext>)."""
    rows = None
    if on == "gpu":
        try:
            rows = combine_strands_gpu(report_fp, ref_fp, contig, device, info=info)
        except _CpuRoute as exc:
            print("--on gpu: {}; running the cpu route..".format(exc))
    if rows is None:
        rows = combine_strands_cpu(report_fp, ref_fp, contig)
    out_fp = default_output(report_fp) if out_fp is None else out_fp
    write_rows(rows, out_fp)
    return out_fp


def add_arguments(ap) -> None:
    ap.add_argument("--frequency_fp", type=str, required=True,
                    help="the call_freq file, 11-column table or (path ending in .bed) bedMethyl")
    ap.add_argument("-r", "--ref_fp", type=str, required=True, help="the genome reference (FASTA)")
    ap.add_argument("--contig", type=str, required=False, default="", help="only this contig (default: all)")
    ap.add_argument("-o", "--result_file", type=str, default=None, help="default: <name>.fb_combined<ext> next to --frequency_fp")
    ap.add_argument("--on", default="cpu", choices=["cpu", "gpu"],
                    help="gpu: genome scan, row parsing and aggregation on the GPU (the host only finds lines and rows); same "
                         "output bytes")
    ap.add_argument("--device", type=int, default=None, help="GPU ordinal of --on gpu (default 0)")


def check_arguments(ap, a) -> None:
    if a.device is not None and a.on != "gpu":
        ap.error("--device needs --on gpu")
    if a.device is not None and a.device < 0:
        ap.error("--device must be >= 0")


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description="combine modification_frequency of CG in forward and backward strand")
    add_arguments(ap)
    a = ap.parse_args(argv)
    check_arguments(ap, a)
    combine_strands(a.frequency_fp, a.ref_fp, a.contig, a.result_file, a.on, a.device or 0)
    return 0


if __name__ == "__main__":
    sys.exit(main())
