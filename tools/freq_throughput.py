"""Rate of the per-site frequency step: `call_modification_frequency --on cpu` against `--on gpu` on one synthetic call file.

Writes a call_mods result file of --rows rows over --sites sites (the rows of a site scattered through the file, probabilities
as call_mods prints them), runs both routes --runs times each through the command line's main(), checks that the two tables are
byte-identical, and prints one JSON object: the median seconds and rows/s of each route, the device-time split of the gpu route
(ds_get_freq_times) and the host's thread count. The cpu route on the same box is the yardstick.

    python tools/freq_throughput.py --out profiles/freq_throughput.json
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

from deepsignal_amd import call_modification_frequency as cmf     # noqa: E402


def write_calls(path: str, rows: int, sites: int, seed: int) -> None:
    rng = np.random.default_rng(seed)
    site_chrom = rng.integers(1, 23, sites)
    site_pos = rng.integers(0, 200_000_000, sites)
    which = rng.integers(0, sites, rows)                 # scattered: a site's rows lie anywhere in the file
    p1 = rng.random(rows).astype(np.float32)
    p0 = np.float32(1) - p1
    with open(path, "w") as f:
        for lo in range(0, rows, 100_000):
            hi = min(rows, lo + 100_000)
            f.write("".join("chr%d\t%d\t+\t%d\tread%d\tt\t%s\t%s\t%d\tACGTACGTCGACGTACG\n" % (
                site_chrom[s], site_pos[s], site_pos[s] + 1, i, a, b, b > a)
                for i, s, a, b in zip(range(lo, hi), which[lo:hi], p0[lo:hi], p1[lo:hi])))


def timed(argv):
    t0 = time.perf_counter()
    with contextlib.redirect_stdout(io.StringIO()):
        assert cmf.main(argv) == 0
    return time.perf_counter() - t0


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--rows", type=int, default=2_000_000)
    ap.add_argument("--sites", type=int, default=100_000)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--out", default=None, help="also write the JSON here")
    a = ap.parse_args(argv)
    with tempfile.TemporaryDirectory() as d:
        calls, out_c, out_g = os.path.join(d, "calls.tsv"), os.path.join(d, "cpu.tsv"), os.path.join(d, "gpu.tsv")
        write_calls(calls, a.rows, a.sites, a.seed)
        size = os.path.getsize(calls)
        gpu_s = [timed(["-i", calls, "-o", out_g, "--on", "gpu", "--device", str(a.device)]) for _ in range(a.runs)]
        cpu_s = [timed(["-i", calls, "-o", out_c]) for _ in range(a.runs)]
        same = open(out_c, "rb").read() == open(out_g, "rb").read()
        info: dict = {}
        with contextlib.redirect_stdout(io.StringIO()):
            stats = cmf.calculate_mods_frequency_gpu([calls], 0.0, a.device, info=info)
    cpu_med, gpu_med = statistics.median(cpu_s), statistics.median(gpu_s)
    res = {"rows": a.rows, "sites": len(stats), "reads_per_site": a.rows / float(a.sites), "file_bytes": size, "runs": a.runs,
           "host_threads": os.cpu_count(), "usable_threads": len(os.sched_getaffinity(0)),
           "cpu_seconds": cpu_s, "gpu_seconds": gpu_s, "cpu_median_s": cpu_med, "gpu_median_s": gpu_med,
           "cpu_rows_per_s": a.rows / cpu_med, "gpu_rows_per_s": a.rows / gpu_med, "speedup": cpu_med / gpu_med,
           "tables_identical": same, "gpu_host_rows": info.get("host_rows"),
           "device_ms": {k: info.get(k) for k in ("copy_ms", "parse_ms", "sort_ms", "accumulate_ms", "batches")}}
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")
    return 0 if same else 1


if __name__ == "__main__":
    sys.exit(main())
