"""End to end: feature file -> per-site frequency table, three ways on one box, one input and one model.

    two_step     call_mods -o calls.tsv, then call_freq -i calls.tsv --on gpu      (result text written, found again and parsed)
    both         call_mods -o calls.tsv --freq_file freq.tsv                        (result text written, the table from the forward)
    table_only   call_mods --freq_file freq.tsv                                     (no result text at all)

Writes a synthetic feature file of --rows rows over --sites sites (the rows of a site scattered over the reads) and seeded
random weights, runs every route --runs times through the command line's main(), checks that the three tables are byte-identical,
and prints one JSON object: the seconds of every run, the medians, the ratios against two_step, and the device-time split of the
frequency stream (ds_get_freq_times, plus freq_values_kernel and the table growths: ds_get_freq_stream_times).

    python tools/callfreq_e2e.py --out profiles/callfreq_e2e.json
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

from deepsignal_amd import call_modifications as cm     # noqa: E402
from deepsignal_amd import deepsignal, synth, weights     # noqa: E402
from deepsignal_amd.utils.process_utils import code2base_dna     # noqa: E402


def write_features(path: str, rows: int, sites: int, seed: int, distinct: int = 1024) -> None:
    """`distinct` feature rows' text, repeated under rows x sampleinfo columns: what the forward computes does not matter here."""
    rng = np.random.default_rng(seed)
    feats = synth.synthetic_features(distinct, seed=seed)
    tails = ["\t".join(["".join(code2base_dna[int(c)] for c in feats["kmer"][i]), ",".join("%s" % np.float32(x) for x in feats["means"][i]),
                        ",".join("%s" % np.float32(x) for x in feats["stds"][i]), ",".join(str(int(x)) for x in feats["sanums"][i]),
                        ",".join("%s" % np.float32(x) for x in feats["signals"][i]), "1"]) for i in range(distinct)]
    site_chrom, site_pos = rng.integers(1, 23, sites), rng.integers(0, 200_000_000, sites)
    which = rng.integers(0, sites, rows)
    with open(path, "w") as f:
        for i, s in enumerate(which.tolist()):
            f.write("chr%d\t%d\t+\t%d\tread_%05d\tt\t%s\n" % (site_chrom[s], site_pos[s], site_pos[s] + 1, i // 50, tails[i % distinct]))


def timed(argv):
    t0 = time.perf_counter()
    with contextlib.redirect_stdout(io.StringIO()):
        assert deepsignal.main(argv) == 0
    return time.perf_counter() - t0


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--rows", type=int, default=131072)
    ap.add_argument("--sites", type=int, default=8000)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--precision", default="fp32")
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--out", default=None, help="also write the JSON here")
    a = ap.parse_args(argv)
    with tempfile.TemporaryDirectory() as d:
        tsv, dsw, calls = os.path.join(d, "features.tsv"), os.path.join(d, "model.dsw"), os.path.join(d, "calls.tsv")
        tables = {k: os.path.join(d, k + ".freq.tsv") for k in ("two_step", "both", "table_only")}
        write_features(tsv, a.rows, a.sites, a.seed)
        weights.save_weights(dsw, weights.random_weights(seed=7, lstm_bias_std=0.1))
        base = ["call_mods", "-i", tsv, "-m", dsw, "--precision", a.precision]
        secs = {k: [] for k in tables}
        split = []
        for _ in range(a.runs):
            t = timed(base + ["-o", calls])
            u = timed(["call_freq", "-i", calls, "-o", tables["two_step"], "--on", "gpu"])
            secs["two_step"].append(t + u)
            split.append((t, u))
            secs["both"].append(timed(base + ["-o", calls, "--freq_file", tables["both"]]))
            secs["table_only"].append(timed(base + ["--freq_file", tables["table_only"]]))
        calls_bytes = os.path.getsize(calls)
        blobs = {k: open(p, "rb").read() for k, p in tables.items()}
        same = blobs["two_step"] == blobs["both"] == blobs["table_only"]
        info: dict = {}
        with contextlib.redirect_stdout(io.StringIO()):       # once more through the function, for the stream's device times
            cm.call_mods(tsv, dsw, None, 17, 360, 512, 0.001, 2, 1, True, True, True, True, None, precision=a.precision,
                         freq_file=tables["table_only"], freq_info=info)
    med = {k: statistics.median(v) for k, v in secs.items()}
    res = {"rows": a.rows, "sites": blobs["two_step"].count(b"\n"), "precision": a.precision, "runs": a.runs, "result_file_bytes": calls_bytes,
           "usable_threads": len(os.sched_getaffinity(0)), "seconds": secs, "median_s": med,
           "two_step_split_s": {"call_mods": statistics.median(t for t, _ in split), "call_freq_on_gpu": statistics.median(u for _, u in split)},
           "ratio_vs_two_step": {k: med["two_step"] / med[k] for k in med}, "tables_identical": same,
           "stream": {k: info.get(k) for k in ("rows", "used", "host_rows", "batches", "growths")},
           "device_ms": {k: info.get(k) for k in ("copy_ms", "values_ms", "rehash_ms", "sort_ms", "accumulate_ms")}}
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")
    return 0 if same else 1


if __name__ == "__main__":
    sys.exit(main())
