"""GPU: `combine_strands --on gpu` -- the device kernels (csrc/ds_combine.hip) against the CPU checkers built from the same
routines, bit for bit, and the command line against the cpu route, byte for byte."""
import numpy as np
import pytest

from deepsignal_amd import combine_strands as cs
from deepsignal_amd import deepsignal
from deepsignal_amd import engine as eng

from combine_cases import (CheckerBackend, KMER, bed_row, fasta_text, load_gold, python_bitmap, random_fasta, random_table, run_route,
                           table_row, write_bytes, write_case)
from freq_cases import bits

pytestmark = pytest.mark.gpu

OK, HOST, SKIP = eng.TEXT_ROW_OK, eng.TEXT_ROW_HOST, eng.COMBINE_ROW_SKIP
SITE_FIELDS = ("chrom", "pos", "sum0", "sum1", "met", "unmet", "cov", "last_plus")


@pytest.fixture(scope="module")
def gold():
    return load_gold()


@pytest.fixture(scope="module")
def engine():
    e = eng.Engine(device=0, max_batch=64, slots=1)
    yield e
    e.close()


def genome_of(tmp_path, data: bytes, contig=""):
    g = cs._Genome(write_bytes(tmp_path / "g.fa", data))
    g.select(contig)
    return g


def scan(backend, g, chunk_bytes):
    for sb, se, sbit, scarry in g.chunks(chunk_bytes):
        backend.combine_genome(g.data, sb, se, sbit, scarry)
    return backend.combine_bitmap()


def both_bitmaps(engine, g, chunk_bytes, form=eng.COMBINE_TABLE):
    """The genome through motif_bitmap_kernel and through the checker, in the same chunks."""
    ref = CheckerBackend()
    ref.combine_begin(form, g.rec_len, 0, 1)
    engine.combine_begin(form, g.rec_len, 0, 1)
    try:
        return scan(engine, g, chunk_bytes), scan(ref, g, chunk_bytes)
    finally:
        engine.combine_end()


def device_sites(engine, form, g, rows, batch_rows, chunk_bytes=64, given=None):
    """`rows` through combine_parse / combine_accumulate in batches of batch_rows -> the device's statuses and sites and the
    checker's, both sorted by (record, pos). given: {global row: None or values} for the rows the device leaves to the host."""
    text = ("\n".join(rows) + "\n").encode()
    begin, end, local, flags, names = eng.freq_locate(text)
    chrom = np.array([g.rec_id.get(n.decode(), -1) for n in names] + [-1], np.int32)[local]
    n, given = len(begin), given or {}
    engine.combine_begin(form, g.rec_len, n, batch_rows)
    try:
        bitmap = scan(engine, g, chunk_bytes)
        status = []
        for s in range(0, n, batch_rows):
            t = min(n, s + batch_rows)
            st = engine.combine_parse(text, begin[s:t], end[s:t], chrom[s:t], flags[s:t])
            status += st.tolist()
            host = np.flatnonzero(st == HOST).tolist()
            engine.combine_accumulate(host, [given[s + i] for i in host])
        got = engine.combine_result()
    finally:
        engine.combine_end()
    ref = eng.combine_reference(form, text, begin, end, chrom, flags, g.rec_len, bitmap, given)
    assert got["rows"] == n

    def ordered(d):
        order = np.lexsort((d["pos"], d["chrom"]))
        return {k: d[k][order] for k in SITE_FIELDS}
    return status, ordered(got), ref["status"].tolist(), ordered(ref)


def assert_sites_equal(got, ref):
    for k in SITE_FIELDS:
        assert got[k].tobytes() == ref[k].tobytes(), k


LENGTHS = (1, 2, 63, 64, 65, 129)


@pytest.mark.parametrize("width", [1, 7, 60])
def test_motif_bitmap_kernel_is_the_checker_and_pythons_find(engine, width, tmp_path):
    """Record lengths 1 .. 129 back to back (records share bitmap words; bit 64 + 65 + ... crosses word boundaries), a chunk of 64
    bytes so that CG falls across a chunk boundary, a line break and a word boundary in the same run."""
    rng = np.random.default_rng(width)
    seqs = ["".join(rng.choice(list("CGcgAT"), n)) for n in LENGTHS + (31, 1)]
    seqs[1], seqs[3], seqs[4] = "cG", seqs[3][:-1] + "C", "G" + seqs[4][1:]      # a C at a record's end, a G opening the next
    seqs[5] = seqs[5][:31] + "cg" + seqs[5][33:59] + "CG" + seqs[5][61:]         # bits 31 | 32 of the record and its line break at 60
    for newline in ("\n", "\r\n"):
        g = genome_of(tmp_path, fasta_text([("r%d" % i, s) for i, s in enumerate(seqs)], width, newline, final_newline=width != 7))
        want = python_bitmap([s.upper() for s in seqs])
        for chunk in (64, 1 << 20):
            dev, ref = both_bitmaps(engine, g, chunk)
            assert dev.tobytes() == ref.tobytes() and dev.tolist() == want.tolist(), (width, newline, chunk)


def test_one_long_line_in_small_chunks(engine, tmp_path):
    rng = np.random.default_rng(9)
    seq = "".join(rng.choice(list("CGcg"), 5000))
    g = genome_of(tmp_path, b">a note\n" + seq.encode() + b"\n>b\nCG")
    for chunk in (64, 999, 1 << 26):
        dev, ref = both_bitmaps(engine, g, chunk)
        assert dev.tobytes() == ref.tobytes() and dev.tolist() == python_bitmap([seq.upper(), "CG"]).tolist()


@pytest.mark.parametrize("nrows", [1, 63, 64, 65, 1000])
@pytest.mark.parametrize("bed", [False, True])
def test_row_counts_in_batches_of_64(engine, nrows, bed, tmp_path):
    text, genome = random_fasta(20 + nrows, 600)
    g = genome_of(tmp_path, text)
    rows = random_table(nrows, genome, nrows, bed)
    form = eng.COMBINE_BED if bed else eng.COMBINE_TABLE
    status, got, ref_status, ref = device_sites(engine, form, g, rows, 64)
    assert status == ref_status and HOST not in status and (nrows < 60 or (OK in status and SKIP in status))
    assert_sites_equal(got, ref)
    if nrows == 1000:                          # and in one batch
        status, got, ref_status, ref = device_sites(engine, form, g, rows, 1024, chunk_bytes=1 << 20)
        assert status == ref_status
        assert_sites_equal(got, ref)


def test_sums_follow_the_row_order(engine, tmp_path):
    """One site of 3,000 rows whose reversed sum has other bits, '+' and '-' rows mixed."""
    rng = np.random.default_rng(5)
    vals = ["%.3f" % x for x in 10.0 ** rng.uniform(-3, 3, 3000)]
    fwd = rev = 0.0
    for v in vals:
        fwd += float(v)
    for v in reversed(vals):
        rev += float(v)
    assert bits(fwd) != bits(rev)              # otherwise the input proves nothing
    g = genome_of(tmp_path, b">c1\nAACGT\n")
    rows = [table_row("c1", 2 + i % 2, "+-"[i % 2], v, "0.0", 1, 2, 3, kmer="K%d" % i) for i, v in enumerate(vals)]
    for batch in (64, 4096):
        status, got, ref_status, ref = device_sites(engine, eng.COMBINE_TABLE, g, rows, batch)
        assert status == [OK] * 3000
        assert_sites_equal(got, ref)
        assert got["pos"].tolist() == [2] and bits(float(got["sum0"][0])) == bits(fwd)
        assert got["met"].tolist() == [3000] and got["cov"].tolist() == [9000] and got["last_plus"].tolist() == [2998]


def test_run_heads_on_workgroup_edges(engine, tmp_path):
    """Three CGs of 256 rows each, interleaved in file order, '+' and '-' rows mixed: whatever order the hash gives the sites, their
    runs begin on sorted lanes 0, 256 and 512, the first lanes of three workgroups, with 256 pad keys behind. Then in batches of 256,
    where every run goes on from the sums the batch before it stored."""
    rng = np.random.default_rng(11)
    vals = ["%.3f" % x for x in 10.0 ** rng.uniform(-3, 3, 768)]
    differs = False
    for site in range(3):
        fwd = rev = 0.0
        for v in vals[site::3]:
            fwd += float(v)
        for v in reversed(vals[site::3]):
            rev += float(v)
        differs = differs or bits(fwd) != bits(rev)
    assert differs                             # otherwise the input proves nothing
    g = genome_of(tmp_path, b">c1\nACGACGACGT\n")
    rows = [table_row("c1", 1 + 3 * (i % 3) + (i // 3) % 2, "+-"[(i // 3) % 2], v, "0.5", i, 2, 3, kmer="K%d" % i) for i, v in enumerate(vals)]
    for batch in (768, 256):
        status, got, ref_status, ref = device_sites(engine, eng.COMBINE_TABLE, g, rows, batch)
        assert status == ref_status == [OK] * 768
        assert_sites_equal(got, ref)
        assert got["pos"].tolist() == [1, 4, 7] and got["cov"].tolist() == [768] * 3 and got["last_plus"].tolist() == [762, 763, 764]


def test_keys_at_the_edges(engine, tmp_path):
    """A '-' row at position 0, positions len - 1, len and 2^40, an unknown chromosome, coverage 0, a site with '-' rows only."""
    g = genome_of(tmp_path, b">c1\nCGACG\n>c2\nCG\n")
    L = 5
    rows = [table_row("c1", 0, "-"), table_row("c1", 0, "+", kmer="first"), table_row("c1", 1, "-"), table_row("c1", L - 1, "+"),
            table_row("c1", L - 1, "-"), table_row("c1", L, "-"), table_row("c1", L, "+"), table_row("c1", 1 << 40, "+"),
            table_row("c1", 1 << 40, "-"), table_row("c1", (1 << 40) + 1, "-"), table_row("cX", 0, "+"), table_row("c2", 0, "+", cov=0, met=0, unmet=0),
            table_row("c2", 2, "-"), table_row("c1", 4, "-"), table_row("c1", 4, "-", "0.5", "0.25"), table_row("c1", -1, "+"),
            table_row("c1", 1, "+", "junk", "junk", "junk", "junk", "junk")]
    status, got, ref_status, ref = device_sites(engine, eng.COMBINE_TABLE, g, rows, 64)
    assert status == ref_status == [SKIP, OK, OK, SKIP, OK, SKIP, SKIP, SKIP, SKIP, SKIP, SKIP, OK, SKIP, OK, OK, SKIP, SKIP]
    assert_sites_equal(got, ref)
    assert got["chrom"].tolist() == [0, 0, 1] and got["pos"].tolist() == [0, 3, 0]
    assert got["last_plus"].tolist() == [1, -1, 11] and got["cov"].tolist() == [8, 12, 0]
    status, got, ref_status, ref = device_sites(engine, eng.COMBINE_BED, g, [bed_row("c1", 0, "-"), bed_row("c1", 1, "-", 9, "12.5"),
                                                                              bed_row("c1", L, "-"), bed_row("cX", 0, "+"), bed_row("c2", 0, "+", 0, 0)], 64)
    assert status == ref_status == [SKIP, OK, SKIP, SKIP, OK]
    assert_sites_equal(got, ref)


def test_host_rows_in_the_middle_of_a_sites_run(engine, tmp_path):
    g = genome_of(tmp_path, b">c1\nAACGT\n>c2\nCG\n")
    rows, given = [], {}
    for i in range(150):
        rows.append(table_row("c1", 2 + i % 2, "+-"[i % 2], "%.3f" % (0.37 * i), "%.3f" % (1000 - 0.11 * i), i, 1, i + 1, kmer="K%d" % i))
        if i % 20 == 7:                        # forms the device leaves to the host; the values are the host's to give
            given[len(rows)] = (0, 2, i % 3 == 0, 1e-30 * i, float(i), 5, 6, 11)
            rows.append(table_row("c1", "+2", "+", "nan", "inf"))
        if i % 50 == 9:
            given[len(rows)] = None
            rows.append(" " + table_row("c1", 2, "+"))
    for batch in (64, 256):
        status, got, ref_status, ref = device_sites(engine, eng.COMBINE_TABLE, g, rows, batch, given=given)
        assert status == [HOST if i in given else OK for i in range(len(rows))]
        assert ref_status == [(SKIP if given[i] is None else OK) if i in given else OK for i in range(len(rows))]
        assert_sites_equal(got, ref)
        assert len(got["pos"]) == 1 and got["last_plus"].tolist() == [max(len(rows) - 2, max(i for i, v in given.items() if v and v[2]))]
    engine.combine_begin(eng.COMBINE_TABLE, g.rec_len, 4, 4)
    try:
        scan(engine, g, 64)
        text = ("\n".join(rows[:4]) + "\n").encode()
        begin, end, local, flags, names = eng.freq_locate(text)
        st = engine.combine_parse(text, begin, end, np.zeros(4, np.int32), np.array([0, 1, 0, 0], np.uint8))
        assert st.tolist() == [OK, HOST, OK, OK]
        with pytest.raises(RuntimeError, match="left to the caller"):
            engine.combine_accumulate()
    finally:
        engine.combine_end()


@pytest.mark.parametrize("idx", [0, 1, 2, 3])
def test_golden_cases_on_the_gpu(gold, idx, tmp_path, capsys):
    case = gold["cases"][idx]
    inp, fa = write_case(tmp_path, gold, case)
    out, stdout = run_route(tmp_path, capsys, inp, fa, "gpu", case["contig"], batch_rows=64, chunk_bytes=64)
    assert out == ("\n".join(case["output"]) + "\n").encode() and stdout == case["stdout"]


def test_command_line_gpu_against_cpu(gold, tmp_path, capsys):
    text, genome = random_fasta(4, 2000)
    fa = write_bytes(tmp_path / "g.fa", text)
    rows = random_table(8, genome, 1500)
    rows[700:700] = [table_row("ctg0", "+3", "+", "nan", "1e-30"), " " + rows[0], table_row("chrUn", "1_0", "-")]
    for name, body in (("f.tsv", rows), ("f.bed", random_table(9, genome, 1500, bed=True))):
        inp = write_bytes(tmp_path / name, ("\n".join(body) + "\n").encode())
        outs = {}
        for on in ("cpu", "gpu"):
            out = str(tmp_path / (on + "_" + name))
            capsys.readouterr()
            assert deepsignal.main(["combine_strands", "--frequency_fp", inp, "-r", fa, "-o", out, "--on", on] + (["--device", "0"] if on == "gpu" else [])) == 0
            outs[on] = (open(out, "rb").read(), capsys.readouterr().out)
        assert outs["gpu"] == outs["cpu"] and outs["cpu"][0].count(b"\n") > 20 and "not in selected" in outs["cpu"][1]
    # call_freq --combine_ref on the gpu route: the same two files as on the cpu route
    inp, fa = write_case(tmp_path, gold, gold["cases"][0])
    from freq_cases import call_row
    calls = [call_row(*r.split("\t")[:2], 0.1 + 0.05 * (i % 17), 0.9 - 0.05 * (i % 17), strand=r.split("\t")[2], pis=i)
             for i, r in enumerate(gold["cases"][3]["input_rows"])]
    cin = write_bytes(tmp_path / "calls.tsv", ("\n".join(calls) + "\n").encode())
    files = {}
    for on in ("cpu", "gpu"):
        out = str(tmp_path / (on + "_freq.tsv"))
        capsys.readouterr()
        assert deepsignal.main(["call_freq", "-i", cin, "-o", out, "--sort", "--combine_ref", fa, "--on", on]) == 0
        stdout = [line for line in capsys.readouterr().out.splitlines() if "parsed on the host" not in line]      # call_freq --on gpu's own note
        files[on] = (open(out, "rb").read(), open(cs.default_output(out), "rb").read(), stdout)
    assert files["gpu"] == files["cpu"] and files["cpu"][1].count(b"\n") > 3
