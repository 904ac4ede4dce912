"""Rate of the evaluation step: `evaluate --on cpu` against `--on gpu` on two synthetic call_mods result files.

Writes an unmethylated and a methylated file of --rows rows each (prob_1 at --places decimals around 0.33 and 0.68), runs both routes
--runs times each through the command line's main() with the same --seed, checks that the two result files and stdouts are
byte-identical, and prints one JSON object: the median seconds and rows/s of each route, the device time per step of the gpu route
(ds_get_eval_times) and the share of the gpu route's wall time that is not device time -- the host's: finding the rows, shuffling the
index lists, Python's glue. Both routes are new code; neither is a yardstick for more than the other on the same box.

    python tools/evaluate_throughput.py --out profiles/evaluate_throughput.json
"""
import argparse
import contextlib
import io
import json
import os
import random
import statistics
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from deepsignal_amd import evaluate_mods_call as ev     # noqa: E402


def write_calls(path: str, rows: int, centre: float, places: int, seed: int) -> None:
    rng = np.random.default_rng(seed)
    with open(path, "w") as f:
        for lo in range(0, rows, 100_000):
            n = min(rows, lo + 100_000) - lo
            p1 = np.round(np.clip(rng.normal(centre, 0.22, n), 0.0, 1.0), places)
            pos = rng.integers(0, 50_000_000, n)
            read = rng.integers(0, 1 << 30, n)
            f.write("".join("chr%d\t%d\t%s\t%d\tread_%d\tt\t%.*f\t%.*f\t%d\tACGTACGTCGACGTACG\n" % (
                1 + pos[i] % 5, pos[i], "+-"[read[i] & 1], 50_000_000 - pos[i], read[i], places, 1 - p1[i], places, p1[i], p1[i] > 0.5)
                for i in range(n)))


def timed(argv):
    out, err = io.StringIO(), io.StringIO()
    t0 = time.perf_counter()
    with contextlib.redirect_stdout(out), contextlib.redirect_stderr(err):
        assert ev.main(argv) == 0
    return time.perf_counter() - t0, out.getvalue()


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--rows", type=int, default=1_000_000, help="rows of each of the two files")
    ap.add_argument("--places", type=int, default=4, help="decimals of the probabilities: 10^places distinct scores at most")
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--out", default=None, help="also write the JSON here")
    a = ap.parse_args(argv)
    with tempfile.TemporaryDirectory() as d:
        un, me, out_c, out_g = (os.path.join(d, n) for n in ("unmethylated.tsv", "methylated.tsv", "cpu.tsv", "gpu.tsv"))
        write_calls(un, a.rows, 0.33, a.places, a.seed)
        write_calls(me, a.rows, 0.68, a.places, a.seed + 1)
        common = ["--unmethylated", un, "--methylated", me, "--seed", str(a.seed)]
        gpu = [timed(common + ["--result_file", out_g, "--on", "gpu", "--device", str(a.device)]) for _ in range(a.runs)]
        cpu = [timed(common + ["--result_file", out_c]) for _ in range(a.runs)]
        same = open(out_c, "rb").read() == open(out_g, "rb").read() and cpu[-1][1] == gpu[-1][1]
        info: dict = {}
        t0 = time.perf_counter()
        with contextlib.redirect_stdout(io.StringIO()), contextlib.redirect_stderr(io.StringIO()):
            ev.evaluate_gpu(un, me, out_g, ev.NUM_SITES, random.Random(a.seed), a.device, info=info)
        wall = time.perf_counter() - t0
        sizes = {"unmethylated_bytes": os.path.getsize(un), "methylated_bytes": os.path.getsize(me)}
    steps = ("copy_ms", "parse_ms", "count_ms", "result_ms")
    device_s = sum(info.get(k, 0.0) for k in steps) / 1000.0
    cpu_med, gpu_med = statistics.median(t for t, _ in cpu), statistics.median(t for t, _ in gpu)
    total = 2 * a.rows
    res = dict(sizes, rows_per_file=a.rows, rows=total, places=a.places, runs=a.runs, host_threads=os.cpu_count(),
               usable_threads=len(os.sched_getaffinity(0)), cpu_seconds=[t for t, _ in cpu], gpu_seconds=[t for t, _ in gpu],
               cpu_median_s=cpu_med, gpu_median_s=gpu_med, cpu_rows_per_s=total / cpu_med, gpu_rows_per_s=total / gpu_med,
               speedup=cpu_med / gpu_med, outputs_identical=same, gpu_host_rows=info.get("host_rows"),
               device_ms={k: info.get(k) for k in steps + ("batches",)},
               gpu_route_wall_s=wall, host_share_of_gpu_route=(wall - device_s) / wall if wall else None)
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")
    return 0 if same else 1


if __name__ == "__main__":
    sys.exit(main())
