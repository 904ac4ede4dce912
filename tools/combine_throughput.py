"""Rate of the strand-combining step: `combine_strands --on cpu` against `--on gpu` on one synthetic genome and table.

Writes a FASTA of --bases bases over --contigs contigs (60-base lines) and an 11-column frequency table of --rows rows over its
CGs, both strands (the rows of a site scattered through the file), runs both routes --runs times each through the command line's
main(), checks that the two outputs and stdouts are byte-identical, and prints one JSON object: the median seconds of each route,
the device time per step of the gpu route (ds_get_combine_times) and the share of the gpu route's wall time that is not device
time -- the host's: finding lines and rows, Python's glue, writing. Both routes are new code; neither is a yardstick for more
than the other on the same box.

    python tools/combine_throughput.py --out profiles/combine_throughput.json
"""
import argparse
import contextlib
import io
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from deepsignal_amd import combine_strands as cs     # noqa: E402


def write_genome(path: str, bases: int, contigs: int, seed: int):
    """-> [(name, positions of its CGs)]"""
    rng = np.random.default_rng(seed)
    out = []
    with open(path, "w") as f:
        for k in range(contigs):
            n = bases // contigs
            seq = rng.choice(np.frombuffer(b"ACGTacgt", np.uint8), n, p=[0.2, 0.2, 0.2, 0.2, 0.05, 0.05, 0.05, 0.05])
            up = seq & 0xDF
            out.append(("chr%d" % (k + 1), np.flatnonzero((up[:-1] == ord("C")) & (up[1:] == ord("G")))))
            f.write(">chr%d synthetic\n" % (k + 1))
            pad = (-n) % 60
            lines = np.concatenate([seq, np.full(pad, ord("\n"), np.uint8)]).reshape(-1, 60)
            body = np.concatenate([lines, np.full((lines.shape[0], 1), ord("\n"), np.uint8)], axis=1).tobytes()
            f.write(body.rstrip(b"\n").decode("ascii") + "\n")
    return out


def write_table(path: str, genome, rows: int, seed: int) -> None:
    rng = np.random.default_rng(seed)
    contig = rng.integers(0, len(genome), rows)
    with open(path, "w") as f:
        for lo in range(0, rows, 100_000):
            hi = min(rows, lo + 100_000)
            lines = []
            for i in range(lo, hi):
                name, cgs = genome[contig[i]]
                minus = int(rng.integers(0, 2))
                pos = int(cgs[int(rng.integers(0, len(cgs)))]) + minus if len(cgs) and rng.random() > 0.02 else int(rng.integers(0, 1000))
                cov = int(rng.integers(1, 60))
                met = int(rng.integers(0, cov + 1))
                p1 = rng.uniform(0, cov)
                lines.append("%s\t%d\t%s\t%d\t%.3f\t%.3f\t%d\t%d\t%d\t%.4f\tACGTACGTCGACGTACG\n" % (
                    name, pos, "+-"[minus], pos, cov - p1, p1, met, cov - met, cov, met / cov))
            f.write("".join(lines))


def timed(argv):
    buf = io.StringIO()
    t0 = time.perf_counter()
    with contextlib.redirect_stdout(buf):
        assert cs.main(argv) == 0
    return time.perf_counter() - t0, buf.getvalue()


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--bases", type=int, default=50_000_000)
    ap.add_argument("--contigs", type=int, default=5)
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--out", default=None, help="also write the JSON here")
    a = ap.parse_args(argv)
    with tempfile.TemporaryDirectory() as d:
        fa, table, out_c, out_g = (os.path.join(d, n) for n in ("genome.fa", "freq.tsv", "cpu.tsv", "gpu.tsv"))
        genome = write_genome(fa, a.bases, a.contigs, a.seed)
        write_table(table, genome, a.rows, a.seed + 1)
        gpu = [timed(["--frequency_fp", table, "-r", fa, "-o", out_g, "--on", "gpu", "--device", str(a.device)]) for _ in range(a.runs)]
        cpu = [timed(["--frequency_fp", table, "-r", fa, "-o", out_c]) for _ in range(a.runs)]
        same = open(out_c, "rb").read() == open(out_g, "rb").read() and cpu[-1][1] == gpu[-1][1]
        sites = open(out_c, "rb").read().count(b"\n")
        info: dict = {}
        t0 = time.perf_counter()
        with contextlib.redirect_stdout(io.StringIO()):
            cs.combine_strands_gpu(table, fa, "", a.device, info=info)
        wall = time.perf_counter() - t0
        sizes = {"fasta_bytes": os.path.getsize(fa), "table_bytes": os.path.getsize(table)}
    steps = ("copy_ms", "motif_ms", "parse_ms", "sort_ms", "accumulate_ms")
    device_s = sum(info.get(k, 0.0) for k in steps) / 1000.0
    cpu_med, gpu_med = statistics.median(t for t, _ in cpu), statistics.median(t for t, _ in gpu)
    res = dict(sizes, bases=a.bases, contigs=a.contigs, rows=a.rows, sites=sites, runs=a.runs, host_threads=os.cpu_count(),
               usable_threads=len(os.sched_getaffinity(0)), cpu_seconds=[t for t, _ in cpu], gpu_seconds=[t for t, _ in gpu],
               cpu_median_s=cpu_med, gpu_median_s=gpu_med, speedup=cpu_med / gpu_med, outputs_identical=same,
               gpu_host_rows=info.get("host_rows"), skipped_rows=info.get("skipped"),
               device_ms={k: info.get(k) for k in steps + ("chunks", "batches")},
               gpu_route_wall_s=wall, host_share_of_gpu_route=(wall - device_s) / wall if wall else None)
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")
    return 0 if same else 1


if __name__ == "__main__":
    sys.exit(main())
