"""CPU: the host half of `combine_strands --on gpu` held to Python -- ds_fasta_locate (lines, names, lengths, flags),
ds_motif_reference and ds_combine_reference (the routines the device kernels are built from), and the Python glue of the gpu route
run on top of the checkers. The reference script's own outputs (tests/golden/combine_golden.json) and the cpu route are the
yardsticks."""
import io

import numpy as np
import pytest

from deepsignal_amd import call_modification_frequency as cmf
from deepsignal_amd import combine_strands as cs
from deepsignal_amd import engine as eng

from combine_cases import (CheckerBackend, KMER, bed_row, fasta_text, load_gold, python_bitmap, random_fasta, random_table, run_route,
                           table_row, write_bytes, write_case)

OK, HOST, SKIP = eng.TEXT_ROW_OK, eng.TEXT_ROW_HOST, eng.COMBINE_ROW_SKIP


@pytest.fixture(scope="module")
def gold():
    return load_gold()


def python_records(data: bytes):
    """The script's reading of a FASTA, record by record as ds_fasta_locate numbers them: [(name, sequence)], from Python's own
    text layer, startswith, strip, split and upper."""
    recs = [["", ""]]
    for line in io.TextIOWrapper(io.BytesIO(data), encoding="utf-8"):
        if line.startswith(">"):
            recs.append([line.strip()[1:].split(" ")[0], ""])
        else:
            recs[-1][1] += line.strip().upper()
    return recs


def located_records(data: bytes):
    loc = eng.fasta_locate(data)
    recs = [[data[b:e].decode("ascii"), ""] for b, e in zip(loc["name_begin"], loc["name_end"])]
    for b, e, r, off in zip(loc["line_begin"], loc["line_end"], loc["line_rec"], loc["line_off"]):
        assert off == len(recs[r][1]) and e > b
        recs[r][1] += data[b:e].decode("ascii").upper()
    assert loc["rec_len"].tolist() == [len(s) for _, s in recs]
    return recs, loc["flags"]


@pytest.mark.parametrize("idx", [0, 1, 2, 3])
def test_goldens_through_the_checkers(gold, idx, tmp_path, capsys):
    case = gold["cases"][idx]
    inp, fa = write_case(tmp_path, gold, case)
    info = {}
    out, stdout = run_route(tmp_path, capsys, inp, fa, "gpu", case["contig"], batch_rows=64, chunk_bytes=64, info=info,
                            make_engine=CheckerBackend)
    assert out == ("\n".join(case["output"]) + "\n").encode() and stdout == case["stdout"]
    assert info["host_rows"] == 0 and info["rows"] == len(case["input_rows"]) and info["skipped"] == case["stdout"].count("\n") - 3


@pytest.mark.parametrize("seed,nbases,nrows,bed", [(1, 1, 1, False), (2, 70, 40, False), (3, 700, 500, True), (4, 2000, 2000, False),
                                                   (5, 2000, 2000, True), (6, 300, 2000, False)])
def test_random_pairs_gpu_route_equals_cpu_route(seed, nbases, nrows, bed, tmp_path, capsys):
    text, genome = random_fasta(seed, nbases)
    fa = write_bytes(tmp_path / "g.fa", text)
    inp = write_bytes(tmp_path / ("f.bed" if bed else "f.tsv"), ("\n".join(random_table(seed, genome, nrows, bed)) + "\n").encode())
    cpu = run_route(tmp_path, capsys, inp, fa, "cpu")
    for batch, chunk in ((256, 64), (1 << 20, 1 << 26), (7, 5)):
        assert run_route(tmp_path, capsys, inp, fa, "gpu", batch_rows=batch, chunk_bytes=chunk, make_engine=CheckerBackend) == cpu
    assert cpu[0].count(b"\n") > 0 or nrows < 10


def test_fasta_locate_follows_pythons_line_and_strip_rules():
    """Every byte value below 0x80 at the start, in the middle and at the end of a line, in a header and in a sequence line."""
    assert [c for c in range(128) if chr(c).isspace()] == [9, 10, 11, 12, 13, 28, 29, 30, 31, 32]      # what strip() removes
    for c in range(128):
        ch = bytes([c])
        for line in (ch + b"acGT", b"ac" + ch + b"GT", b"acGT" + ch, ch + b"ac" + ch + b"gt" + ch, ch):
            for data in (b">r1 d\nAC\n" + line + b"\ncg\n>r2\nG", b">r1 d\n" + line, line + b"\n>r1\nacg\n",
                         b">r" + line + b" x\nACG\n", b">" + line + b"\r\nC\r\n" + line + b"\r\n"):
                recs, flags = located_records(data)
                want = python_records(data)
                bare_cr = b"\r" in data.replace(b"\r\n", b"")
                assert bool(flags & eng.FASTA_BARE_CR) == bare_cr and not flags & eng.FASTA_NON_ASCII, (c, data)
                if not bare_cr:
                    assert recs == want, (c, data)
    for data, nrec in ((b"", 1), (b"\n", 1), (b">", 2), (b">\n>", 3), (b"ACG", 1), (b"\r\n\r\n", 1)):
        recs, flags = located_records(data)
        assert len(recs) == nrec and recs == python_records(data) and flags == 0
    assert eng.fasta_locate(">r\xc3\xa9\nACG\n".encode("latin-1"))["flags"] == eng.FASTA_NON_ASCII
    assert eng.fasta_locate(b">r\nAC\rG\n\xff")["flags"] == eng.FASTA_NON_ASCII | eng.FASTA_BARE_CR
    big = b">big\n" + b"ACG" * 40000 + b"\n" + b"\n".join([b"cg"] * 5000)          # more lines and records than the first guess
    recs, flags = located_records(big + b"\n" + b"".join(b">r%d\nC\n" % i for i in range(1500)))
    assert len(recs) == 1502 and recs[1][1] == "ACG" * 40000 + "CG" * 5000


def genome_of(tmp_path, data: bytes, contig=""):
    g = cs._Genome(write_bytes(tmp_path / "g.fa", data))
    g.select(contig)
    return g


def checker_bitmap(g, chunk_bytes):
    nbits = int(g.rec_len.sum())
    bitmap = np.zeros((nbits + 31) // 32, np.uint32)
    for sb, se, sbit, scarry in g.chunks(chunk_bytes):
        assert int(se[-1] - sb[0]) <= chunk_bytes
        eng.motif_reference(g.data, sb, se, sbit, scarry, nbits, bitmap)
    return bitmap


@pytest.mark.parametrize("width", [1, 7, 60])
def test_motif_checker_is_pythons_find(width, tmp_path):
    rng = np.random.default_rng(width)
    for newline in ("\n", "\r\n"):
        seqs = ["".join(rng.choice(list("CGcgAT"), n)) for n in (1, 2, 63, 64, 65, 129, 31, 1)]
        seqs[1], seqs[3] = "cG", seqs[3][:-1] + "C"                # a record that is one CG; a C at a record's end, a G behind it
        seqs[4] = "G" + seqs[4][1:]
        data = fasta_text([("r%d" % i, s) for i, s in enumerate(seqs)], width, newline, final_newline=width != 7)
        g = genome_of(tmp_path, data)
        want = python_bitmap([s.upper() for s in seqs])
        for chunk in (64, 5, 1 << 20):
            assert checker_bitmap(g, chunk).tolist() == want.tolist(), (width, newline, chunk)
        for name, s in zip(g.rec_id, seqs):
            for pos in range(-2, len(s) + 2):
                assert g.in_motif(name, pos) == (pos >= 0 and s.upper()[pos:pos + 2] == "CG")
    g = genome_of(tmp_path, b">a\nCG\n>b\nCGCG\n>a\nTTCG\n>e\n>c\nC", "")
    assert list(g.rec_id) == ["a", "b", "c"] and g.rec_len.tolist() == [4, 4, 1]
    assert checker_bitmap(g, 64).tolist() == python_bitmap(["TTCG", "CGCG", "C"]).tolist()
    assert genome_of(tmp_path, b">a\nCG\n>b\nCGCG\n", "b").rec_len.tolist() == [4]
    with pytest.raises(KeyError):
        genome_of(tmp_path, b">a\nCG\n>b\n>c\nCG", "b")
    with pytest.raises(RuntimeError):                              # a carried base in front of the bitmap's first bit
        eng.motif_reference(b"G", [0], [1], [0], [ord("C")], 8)
    with pytest.raises(RuntimeError):
        eng.motif_reference(b"CGCG", [0], [4], [6], [0], 8)


def rows_status(form, rows, genome_bytes, tmp_path):
    g = genome_of(tmp_path, genome_bytes)
    text = ("\n".join(rows) + "\n").encode()
    begin, end, local, flags, names = eng.freq_locate(text)
    chrom = np.array([g.rec_id.get(n.decode(), -1) for n in names] + [-1], np.int32)[local]
    return eng.combine_reference(form, text, begin, end, chrom, flags, g.rec_len, checker_bitmap(g, 64))


def test_row_grammar_of_the_checker(tmp_path):
    fa = b">c1\nACGTCGC\n>c2\nCG\n"
    good = [table_row("c1", 1, "+"), table_row("c1", 2, "-"), table_row("c1", "-0", "*"), table_row("c1", "01", "+", "1e-3", ".5", -1, 0, 123456789),
            "\t".join(table_row("c1", 5, "-").split("\t")[:9]), table_row("c2", 0, "+") + "\textra"]
    out = rows_status(eng.COMBINE_TABLE, good, fa, tmp_path)
    assert out["status"].tolist() == [OK, OK, SKIP, OK, OK, OK]
    assert out["row_pos"].tolist()[:2] == [1, 1] and out["row_plus"].tolist() == [1, 0, 0, 1, 0, 1]
    assert out["row_a"][3] == float("1e-3") and out["row_cov"][3] == 123456789 and out["row_met"][3] == -1
    skip = [table_row("c1", 0, "-"), table_row("c1", 6, "+"), table_row("c1", 7, "+"), table_row("c1", 1 << 40, "+"), table_row("c9", 1, "+"),
            "\t".join(["c1", "0", "+", "7", "x", "y", "z"]), table_row("c1", "9" * 18, "+", "nan")]
    assert rows_status(eng.COMBINE_TABLE, skip, fa, tmp_path)["status"].tolist() == [SKIP] * len(skip)
    host = [table_row("c1", "+1", "+"), table_row("c1", "1_0", "+"), table_row("c1", "9" * 19, "+"), table_row("c1", "", "+"), "c1\t1", "c1", "",
            " " + table_row("c1", 1, "+"), table_row("c1", 1, "+") + "\r", "\t".join(table_row("c1", 1, "+").split("\t")[:10]),
            "\t".join(table_row("c1", 2, "-").split("\t")[:8]), table_row("c1", 1, "+", "nan"), table_row("c1", 1, "+", "0.5", "1e-30"),
            table_row("c1", 1, "+", met="1234567890"), table_row("c1", 1, "+", unmet="+1"), table_row("c1", 1, "+", cov="1.0")]
    assert rows_status(eng.COMBINE_TABLE, host, fa, tmp_path)["status"].tolist() == [HOST] * len(host)
    bed = [bed_row("c1", 1, "+", 7, 33), bed_row("c1", 2, "-", 5, "12.5"), bed_row("c1", 2, "+"), bed_row("c1", 1, "+", "x", "y"),
           "\t".join(bed_row("c1", 1, "+").split("\t")[:10]), "\t".join(bed_row("c1", 0, "+").split("\t")[:5]), bed_row("c1", 1, "+", 1 << 53, 5)]
    out = rows_status(eng.COMBINE_BED, bed, fa, tmp_path)
    assert out["status"].tolist() == [OK, OK, SKIP, HOST, HOST, HOST, HOST]
    assert out["row_a"][0] == 33.0 / 100 * 7 and out["row_a"][1] == 12.5 / 100 * 5 and out["row_cov"].tolist()[:2] == [7, 5]
    assert out["sum0"].tolist() == [0.0 + 33.0 / 100 * 7 + 12.5 / 100 * 5] and out["cov"].tolist() == [12] and out["last_plus"].tolist() == [0]


def test_bed_met_is_two_roundings_not_a_fused_one(tmp_path):
    """percent / 100 * coverage, then the sum: pairs for which a fused multiply-add would give other bits."""
    rng = np.random.default_rng(3)
    rows, want, other = [], 0.0, False
    for _ in range(400):
        pct, cov = "%.4f" % rng.uniform(0, 100), int(rng.integers(1, 10 ** 9))
        rows.append(bed_row("c1", 1, "+", cov, pct))
        q = float(pct) / 100
        fused = float(np.longdouble(q) * np.longdouble(cov) + np.longdouble(want))      # one rounding at the end
        want += q * cov
        other = other or fused != want
    assert other                                                   # otherwise the input proves nothing
    out = rows_status(eng.COMBINE_BED, rows, b">c1\nACG\n", tmp_path)
    assert (out["status"] == OK).all() and out["sum0"].tolist() == [want]


def test_host_rows_take_the_cpu_routes_expressions(tmp_path, capsys):
    fa = write_bytes(tmp_path / "g.fa", b">c1\nACGTCGC\n>c2\nCG\n")
    rows = [table_row("c1", 1, "+", "0.1", "0.2", kmer="K0"), table_row("c1", "+1", "+", "nan", "1e-30", kmer="K1"),
            " " + table_row("c1", 2, "-", "inf", "0.25"), table_row("c1", 1, "+", "0.5", "0.5", met="1_0", kmer="K3") + "\r",
            table_row("c1", "1_0", "+"), table_row("c1", 2, "-", "0.3", "0.4"), table_row("c9", "+5", "+"), table_row("c1", "９", "+"),
            table_row("c2", 0, "+", "1e400", "0x", kmer="K8").replace("0x", "-0.0"), table_row("c1", "9" * 25, "-")]
    inp = write_bytes(tmp_path / "f.tsv", ("\n".join(rows) + "\n").encode())
    cpu = run_route(tmp_path, capsys, inp, fa, "cpu")
    for batch in (3, 64):
        info = {}
        assert run_route(tmp_path, capsys, inp, fa, "gpu", batch_rows=batch, info=info, make_engine=CheckerBackend) == cpu
        assert info["host_rows"] == 8 and info["skipped"] == 4
    assert b"\tK3\n" in cpu[0] and b"nan" in cpu[0] and b"c2\t0\t+\t0\tinf" in cpu[0]
    bed = write_bytes(tmp_path / "f.bed", ("\n".join([bed_row("c1", 1, "+", 7, 33), bed_row("c1", "+2", "-", "1_1", "+50.5"),
                                                      bed_row("c2", 0, "+", 3, "1e-30") + " ", bed_row("c1", " 7", "+")]) + "\n").encode())
    cpu = run_route(tmp_path, capsys, bed, fa, "cpu")
    assert run_route(tmp_path, capsys, bed, fa, "gpu", batch_rows=2, make_engine=CheckerBackend) == cpu


def test_malformed_rows_raise_as_the_cpu_route(tmp_path, capsys):
    fa = write_bytes(tmp_path / "g.fa", b">c1\nACGTCGC\n")
    good, skipped = table_row("c1", 1, "+"), table_row("c1", 0, "+")
    for bad, exc in (("\t".join(good.split("\t")[:10]), IndexError), ("", IndexError), ("c1\t1", IndexError), (table_row("c1", "x", "+"), ValueError),
                     (table_row("c1", 1, "+", "zero"), ValueError), (table_row("c1", 2, "-", cov="1.5"), ValueError)):
        inp = write_bytes(tmp_path / "f.tsv", ("\n".join([good, skipped, good, bad, skipped, good]) + "\n").encode())
        outs = []
        for route in (lambda: cs.combine_strands_cpu(inp, fa), lambda: cs.combine_strands_gpu(inp, fa, batch_rows=2, make_engine=CheckerBackend)):
            capsys.readouterr()
            with pytest.raises(exc):
                route()
            outs.append(capsys.readouterr().out)
        assert outs[0] == outs[1] and outs[0].count("not in selected") == 1      # what the script had printed when it raised


def test_inputs_that_go_the_cpu_route(tmp_path, capsys):
    good = table_row("c1", 1, "+")
    inp = write_bytes(tmp_path / "f.tsv", (good + "\n").encode())
    for data in (b">c1\nACG\n>c\xc3\xa9\nCG\n", b">c1\nAC\rG\n", b">c1\nACG\r"):
        fa = write_bytes(tmp_path / "g.fa", data)
        with pytest.raises(cmf._CpuRoute):
            cs.combine_strands_gpu(inp, fa, make_engine=CheckerBackend)
        assert capsys.readouterr().out == ""                       # nothing is printed twice
        out = str(tmp_path / "o.tsv")
        assert cs.combine_strands(inp, fa, out_fp=out, on="gpu") == out
        lines = capsys.readouterr().out.splitlines()
        assert lines[0].startswith("--on gpu: the FASTA holds") and lines[1:] == [cs.MSG_GENOME, cs.MSG_MOTIF, cs.MSG_COMBINE]
        assert open(out).read().startswith("c1\t1\t+\t1\t1.25\t2.75\t1\t3\t4\t0.25\t" + KMER)
    fa = write_bytes(tmp_path / "g.fa", b">c1\nACG\n")
    for rows in ([good, "a\rb", good], [good, table_row("c1", 1, "+", cov=str(1 << 32))]):
        inp = write_bytes(tmp_path / "f.tsv", ("\n".join(rows) + "\n").encode())
        with pytest.raises(cmf._CpuRoute):
            cs.combine_strands_gpu(inp, fa, make_engine=CheckerBackend)
    assert cs.combine_strands_gpu(write_bytes(tmp_path / "none.tsv", b""), fa, make_engine=CheckerBackend) == []
    e = object.__new__(eng.Engine)                                 # argument checks come before any library call
    for call in (lambda: eng.Engine.combine_begin(e, 2, [4], 1, 1), lambda: eng.Engine.combine_begin(e, 0, [], 1, 1),
                 lambda: eng.Engine.combine_begin(e, 0, [(1 << 40) + 1], 1, 1), lambda: eng.Engine.combine_begin(e, 0, [4], 1, 0),
                 lambda: eng.Engine.combine_begin(e, 0, [4], (1 << 30) + 1, 1)):
        with pytest.raises(ValueError):
            call()
    with pytest.raises(ValueError):
        cs.combine_strands_gpu(inp, fa, chunk_bytes=0, make_engine=CheckerBackend)
