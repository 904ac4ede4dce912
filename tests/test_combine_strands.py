"""CPU: `combine_strands` (scope row f5) -- the cpu route held to the reference script's own outputs and stdout
(tests/golden/combine_golden.json, made by running the script), and the command line around it."""
import os

import pytest

from deepsignal_amd import call_modification_frequency as cmf
from deepsignal_amd import combine_strands as cs
from deepsignal_amd import deepsignal

from combine_cases import load_gold, run_route, table_row, write_bytes, write_case
from freq_cases import call_row


@pytest.fixture(scope="module")
def gold():
    return load_gold()


@pytest.mark.parametrize("idx", [0, 1, 2, 3])
def test_cpu_route_is_the_reference_byte_for_byte(gold, idx, tmp_path, capsys):
    case = gold["cases"][idx]
    inp, fa = write_case(tmp_path, gold, case)
    argv = ["combine_strands", "--frequency_fp", inp, "-r", fa] + (["--contig", case["contig"]] if case["contig"] else [])
    capsys.readouterr()
    assert deepsignal.main(argv) == 0
    assert capsys.readouterr().out == case["stdout"]
    base, ext = os.path.splitext(inp)
    assert open(base + ".fb_combined" + ext, "rb").read() == ("\n".join(case["output"]) + "\n").encode()


def test_golden_covers_what_it_should(gold):
    fasta = gold["fasta"]
    assert "\r\n" in fasta and "\n\n" in fasta.replace("\r\n", "\n") and not fasta.endswith("\n") and any(c.islower() for c in fasta)
    assert fasta.count(">chrD") == 2 and ">empty\n>" in fasta and ">chr1 " in fasta
    table = gold["cases"][0]
    assert any(line.endswith("\t-") for line in table["output"])                      # a site with '-' rows only
    assert any(r.split("\t")[8] == "0" for r in table["input_rows"])                  # coverage 0
    assert "chr1\t19\t" in "\n".join(table["output"])                                 # the CG across the line break
    sites = [tuple(r.split("\t")[:2]) for r in gold["cases"][3]["input_rows"]]
    assert max(sites.count(s) for s in set(sites)) >= 3                               # many rows on one site


def test_contig_that_the_genome_lacks_raises_keyerror(gold, tmp_path):
    inp, fa = write_case(tmp_path, gold, gold["cases"][0])
    for name in ("chrNope", "empty", "first"):
        with pytest.raises(KeyError):
            cs.main(["--frequency_fp", inp, "-r", fa, "--contig", name])
    assert not os.path.exists(cs.default_output(inp))


def test_output_names_and_forms(gold, tmp_path, capsys):
    assert cs.default_output("/a/b/freq.tsv") == "/a/b/freq.fb_combined.tsv"
    assert cs.default_output("freq.run1.BED") == "freq.run1.fb_combined.BED" and cs.default_output("freq") == "freq.fb_combined"
    assert cs.is_bed("x.bed") and cs.is_bed("x.BeD") and not cs.is_bed("x.bed.txt") and not cs.is_bed("x.tsv")
    inp, fa = write_case(tmp_path, gold, gold["cases"][2])
    out = str(tmp_path / "elsewhere.txt")
    assert cs.main(["--frequency_fp", inp, "-r", fa, "-o", out]) == 0
    assert open(out).read().splitlines() == gold["cases"][2]["output"]                # the form follows the input's name
    assert not os.path.exists(cs.default_output(inp))


def test_genome_records_as_the_script_keeps_them(tmp_path):
    fa = write_bytes(tmp_path / "g.fa", b"ACG\n>a x y\n ac\tg \r\n\ncgT\n>b\n>\nCG\n>a\nttcg\n>c\n")
    assert cs.read_contigs(fa) == {"a": "TTCG", "c": ""}                              # '' and b dropped, a replaced, the last kept
    assert list(cs.read_contigs(fa)) == ["a", "c"]
    fa = write_bytes(tmp_path / "h.fa", b"cg\nCG")
    assert cs.read_contigs(fa) == {"": "CGCG"}                                        # no header at all: the last record, named ''
    assert cs.read_contigs(write_bytes(tmp_path / "e.fa", b"")) == {"": ""}
    fa = write_bytes(tmp_path / "i.fa", b">a\nA C\x0bG\nc\rg\n")                        # inner whitespace stays a base; a bare CR ends a line
    assert cs.read_contigs(fa) == {"a": "A C\x0bGCG"}


def test_row_semantics(tmp_path, capsys):
    fa = write_bytes(tmp_path / "g.fa", b">c1\nACGTCGC\n>c2\nCG\n")
    rows = [table_row("c1", 1, "+", "0.1", "0.2", 1, 2, 3, kmer="K1"), table_row("c1", 2, "-", "0.3", "0.4", 4, 5, 9),
            table_row("c1", 1, "+", "0.5", "0.6", 0, 0, 0, kmer="K2"), table_row("c1", 5, "-", "1", "2", 1, 1, 2),
            table_row("c1", 0, "-"), table_row("c1", 6, "+"), table_row("c1", 7, "+"), table_row("c3", 0, "+"),
            table_row("c2", 7, "-", "x", "y", "z", "?", "!"),       # skipped before its numbers are read
            table_row("c2", 0, "*", "0.25", "0.5", 1, 0, 0), table_row("c2", 1, "-", "0", "0", 0, 0, 0)]
    inp = write_bytes(tmp_path / "f.tsv", ("\n".join(rows) + "\n").encode())
    got = cs.combine_strands_cpu(inp, fa)
    out = capsys.readouterr().out.splitlines()
    assert got == [["c1", 1, "+", 1, 0.1 + 0.3 + 0.5, 0.2 + 0.4 + 0.6, 5, 7, 12, 5 / 12, "K2"],
                   ["c1", 4, "+", 4, 1.0, 2.0, 1, 1, 2, 0.5, "-"]]                     # c2:0 has coverage 0 and is dropped
    assert out[:3] == [cs.MSG_GENOME, cs.MSG_MOTIF, cs.MSG_COMBINE] and len(out) == 3 + 5
    assert out[3] == "%s, not in selected motif poses of the genome" % rows[4].split("\t")
    bad = write_bytes(tmp_path / "bad.tsv", (rows[0] + "\n" + "\t".join(rows[0].split("\t")[:10]) + "\n").encode())
    with pytest.raises(IndexError):
        cs.combine_strands_cpu(bad, fa)
    bed = write_bytes(tmp_path / "f.bed", b"c1\t1\t2\t.\t7\t+\t1\t2\t0,0,0\t7\t33\nc1\t2\t3\t.\t5\t-\t2\t3\t0,0,0\t5\t12.5\n")
    met = 33.0 / 100 * 7 + 12.5 / 100 * 5
    assert cs.combine_strands_cpu(bed, fa) == [["c1", 1, 2, ".", 12, "+", 1, 2, "0,0,0", 12, int(round(met / 12, 2) * 100)]]


def test_flag_validation(gold, tmp_path):
    inp, fa = write_case(tmp_path, gold, gold["cases"][0])
    for argv in (["--device", "0"], ["--on", "tpu"], ["--on", "gpu", "--device", "-1"]):
        with pytest.raises(SystemExit):
            cs.main(["--frequency_fp", inp, "-r", fa] + argv)
        with pytest.raises(SystemExit):
            deepsignal.main(["combine_strands", "--frequency_fp", inp, "-r", fa] + argv)
    with pytest.raises(SystemExit):
        cs.main(["--frequency_fp", inp])
    with pytest.raises(SystemExit):
        cmf.main(["-i", inp, "-o", str(tmp_path / "o.tsv"), "--combine_contig", "chr1"])


def test_call_freq_combine_ref_is_call_freq_then_combine_strands(gold, tmp_path, capsys):
    fa = write_bytes(tmp_path / "genome.fa", gold["fasta"].encode())
    calls = [call_row(*r.split("\t")[:2], 0.1 + 0.05 * (i % 17), 0.9 - 0.05 * (i % 17), strand=r.split("\t")[2], pis=i)
             for i, r in enumerate(gold["cases"][3]["input_rows"])]
    inp = write_bytes(tmp_path / "calls.tsv", ("\n".join(calls) + "\n").encode())
    for extra, name in (([], "a.tsv"), (["--bed"], "b.bed"), (["--sort", "--combine_contig", "chr2"], "c.txt")):
        one, two = str(tmp_path / ("one_" + name)), str(tmp_path / ("two_" + name))
        assert deepsignal.main(["call_freq", "-i", inp, "-o", one, "--combine_ref", fa] + extra) == 0
        out_one = capsys.readouterr().out
        plain = [a for a in extra if a not in ("--combine_contig", "chr2")]
        assert deepsignal.main(["call_freq", "-i", inp, "-o", two] + plain) == 0
        assert deepsignal.main(["combine_strands", "--frequency_fp", two, "-r", fa] + (["--contig", "chr2"] if "chr2" in extra else [])) == 0
        assert capsys.readouterr().out == out_one
        assert open(one, "rb").read() == open(two, "rb").read()
        combined = open(cs.default_output(one), "rb").read()
        assert combined == open(cs.default_output(two), "rb").read() and combined.count(b"\n") > 3
