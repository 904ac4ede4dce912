"""Throughput of `call_mods` on fast5 reads: host feature extraction (--extract_on cpu) against the device extractor
(--extract_on gpu) at the same --nproc, on seeded synthetic reads held in memory.

    python tools/fast5_throughput.py [--reads 24] [--nproc 8] [--norm mad] [--precision fp32] [--out result.json]

HDF5 reading is bypassed: each worker synthesises the reads (deepsignal_amd.synth.synthetic_read: 10 - 50 k bases, 4 - 15
samples per base, random ACGT, CG sites) before the clock starts, then runs the route's own per-read code on them --
extract_features.extract_read_features + call_modifications._features_item for the host route,
extract_features._device_read_record (motif scan, site list, packing) for the device route -- and the main process drives the
engine exactly as _call_mods_from_fast5s does (_call_mods; one _ReadsPipeline fed through _rows_from_device per task). As there, --nproc > 2 runs nproc - 1 worker
processes next to the engine process; otherwise the workers' part runs inline.

Printed (one JSON line): sites/s of both routes; the device route's worker-side rate (sites per worker-second times workers:
what the motif scan + packing can feed); the forward alone on resident-size batches (submit / wait of host features); and the
extraction kernels' device time per batch of max_batch sites (Engine.kernel_stats() with profiling on, ds_extract).

    python tools/fast5_throughput.py --mode extract [--reads 24] [--nproc 8] [--norm mad] [--out result.json]

`extract` (fast5-like reads -> the feature TSV's row bytes, no forward, no model): the host route as extract_features runs it --
nproc workers, each extract_read_features + _features_to_str, the parent writing the rows to a file -- against
`extract --extract_on gpu` -- nproc - 1 workers running _device_read_record, the parent driving ds_submit_rows / ds_wait_rows
through extract_features._rows_from_device and writing the returned bytes to a file. Also printed: device microseconds per
batch of the statistics, values, length + scan and format kernels and of the text's device-to-host copy (Engine.rows_times()).
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

KMER, SIGNAL = 17, 360
_READS = {}
_CFG = {}


def _synth_read(i, seed):
    from deepsignal_amd import synth
    rng = np.random.default_rng(seed * 100003 + i)
    raw, starts, lengths, bases, scaling, offset = synth.synthetic_read(int(rng.integers(10000, 50001)), seed * 100003 + i)
    info = ("read-%d" % i, "t", "+", "chr1", 1000000 * i)
    return raw, starts, lengths, bases, scaling, offset, info


def _init(nreads, seed, norm):
    _CFG["norm"] = norm
    for i in range(nreads):
        _READS[i] = _synth_read(i, seed)


def _ready(_):
    return len(_READS)


def _host_task(idx):
    from deepsignal_amd import call_modifications as cm, extract_features as ef
    t0 = time.perf_counter()
    feats = []
    for i in idx:
        raw, starts, lengths, bases, scaling, offset, (name, strand, astrand, chrom, cstart) = _READS[i]
        feats += ef.extract_read_features(raw, starts, lengths, bases, scaling, offset, name, strand, astrand, chrom, cstart,
                                          None, ["CG"], 0, KMER, SIGNAL, 1, _CFG["norm"])
    return cm._features_item(feats), time.perf_counter() - t0


def _host_rows_task(idx):
    from deepsignal_amd import extract_features as ef
    t0 = time.perf_counter()
    rows = []
    for i in idx:
        raw, starts, lengths, bases, scaling, offset, (name, strand, astrand, chrom, cstart) = _READS[i]
        rows += [ef._features_to_str(f) for f in
                 ef.extract_read_features(raw, starts, lengths, bases, scaling, offset, name, strand, astrand, chrom, cstart,
                                          None, ["CG"], 0, KMER, SIGNAL, 1, _CFG["norm"])]
    return "".join(r + "\n" for r in rows).encode(), time.perf_counter() - t0


def _device_task(idx):
    from deepsignal_amd import extract_features as cm
    t0 = time.perf_counter()
    recs = []
    for i in idx:
        raw, starts, lengths, bases, scaling, offset, info = _READS[i]
        rec = cm._device_read_record(raw, starts, lengths, bases, scaling, offset, info, ["CG"], 0, None, KMER)
        if rec:
            recs.append(rec)
    return recs, time.perf_counter() - t0


def _run_route(route, eng, tasks, nproc, args):
    from deepsignal_amd import call_modifications as cm
    fn = _host_task if route == "cpu" else _device_task
    pool = None
    workers = 1
    if nproc > 2 and len(tasks) > 1:
        import multiprocessing as mp
        workers = min(nproc - 1, len(tasks))
        pool = mp.get_context("spawn").Pool(workers, initializer=_init, initargs=(args.reads, args.seed, args.norm))
        pool.map(_ready, range(4 * workers))          # every worker has synthesised its reads before the clock starts
    else:
        _init(args.reads, args.seed, args.norm)
    pipe = cm._ReadsPipeline(eng, args.norm) if route == "gpu" else None
    try:
        nsites, worker_s = 0, 0.0
        t0 = time.perf_counter()
        results = pool.imap(fn, tasks) if pool is not None else (fn(t) for t in tasks)
        for payload, dt in results:
            worker_s += dt
            if route == "cpu":
                rows, _, _ = cm._call_mods(payload, eng, args.batch_size)
                nsites += len(rows)
            else:
                nsites += sum(c.count(b"\n") for c in cm._rows_from_device(payload, pipe, args.batch_size))
        wall = time.perf_counter() - t0
    finally:
        if pipe is not None:
            pipe.close()
        if pool is not None:
            pool.close()
            pool.join()
    return {"sites": nsites, "seconds": round(wall, 4), "sites_per_s": round(nsites / wall, 1),
            "worker_seconds": round(worker_s, 4), "worker_sites_per_s": round(nsites / worker_s * workers, 1), "workers": workers}


def _run_extract_route(route, eng, tasks, nproc, args, out_path):
    """One route of `extract`: rows to out_path; the host route uses all nproc processes as workers (extract_features does),
    the device route nproc - 1 beside the process that drives the engine."""
    from deepsignal_amd import extract_features as ef
    fn = _host_rows_task if route == "cpu" else _device_task
    workers = min(nproc if route == "cpu" else nproc - 1, len(tasks))
    pool = None
    if workers > 1 or (route == "gpu" and nproc > 2):
        import multiprocessing as mp
        workers = max(1, workers)
        pool = mp.get_context("spawn").Pool(workers, initializer=_init, initargs=(args.reads, args.seed, args.norm))
        pool.map(_ready, range(4 * workers))
    else:
        workers = 1
        _init(args.reads, args.seed, args.norm)
    try:
        nsites = nbytes = 0
        worker_s = 0.0
        with open(out_path, "wb") as wf:
            t0 = time.perf_counter()
            results = (pool.imap_unordered if route == "cpu" else pool.imap)(fn, tasks) if pool is not None else (fn(t) for t in tasks)
            for payload, dt in results:
                worker_s += dt
                chunks = [payload] if route == "cpu" else ef._rows_from_device(payload, eng, args.norm, 1)[0]
                for c in chunks:
                    wf.write(c)
                    nsites += c.count(b"\n")
                    nbytes += len(c)
            wf.flush()
            os.fsync(wf.fileno())
            wall = time.perf_counter() - t0
    finally:
        if pool is not None:
            pool.close()
            pool.join()
    return {"sites": nsites, "bytes": nbytes, "seconds": round(wall, 4), "sites_per_s": round(nsites / wall, 1),
            "MB_per_s": round(nbytes / wall / 1e6, 1), "worker_seconds": round(worker_s, 4), "workers": workers}


def _rows_kernel_times(eng, args, repeats=3):
    """extract_rows of the reads in full batches with profiling on: device µs per batch of each step (first pass is warm-up)."""
    from deepsignal_amd.engine import ReadBatch, pack_info
    _init(args.reads, args.seed, args.norm)
    recs = _device_task(list(range(args.reads)))[0]
    B = eng.max_batch
    sr = np.concatenate([np.full(len(r[2]), i, np.int32) for i, r in enumerate(recs)])
    sl = np.concatenate([r[2] for r in recs])
    lines = [line for r in recs for line in r[3].split(b"\n")[:-1]]
    batches = []
    for k in range(len(sr) // B):
        used = np.unique(sr[k * B:(k + 1) * B])
        remap = np.full(len(recs), -1, np.int32)
        remap[used] = np.arange(len(used), dtype=np.int32)
        batches.append((ReadBatch([recs[i][1] for i in used], remap[sr[k * B:(k + 1) * B]], sl[k * B:(k + 1) * B], norm=args.norm),)
                       + pack_info(lines[k * B:(k + 1) * B]))
    nbytes = [len(eng.extract_rows(b, info, off, 1)[0]) for b, info, off in batches]
    eng.set_profiling(1)
    eng.rows_times(reset=True)
    for _ in range(repeats):
        for b, info, off in batches:
            eng.extract_rows(b, info, off, 1)
    t = eng.rows_times(reset=True)
    eng.set_profiling(0)
    n = max(1, t["batches"])
    out = {"batches": len(batches), "repeats": repeats, "sites_per_batch": B, "text_bytes_per_batch": round(float(np.mean(nbytes)), 1)}
    for k in ("stats_ms", "values_ms", "length_ms", "format_ms", "d2h_ms"):
        out[k[:-3] + "_us_per_batch"] = round(t[k] * 1e3 / n, 1)
    return out


def _main_extract(args):
    import tempfile
    from deepsignal_amd.engine import Engine
    eng = Engine(device=0, max_batch=args.engine_batch)          # no weights: extraction has no model
    tmp = tempfile.mkdtemp(prefix="fast5_throughput_")
    try:
        tasks = [list(range(i, min(args.reads, i + args.reads_per_task))) for i in range(0, args.reads, args.reads_per_task)]
        res = {"tool": "fast5_throughput", "mode": "extract", "reads": args.reads, "nproc": args.nproc, "norm": args.norm,
               "engine_batch": args.engine_batch, "hdf5": "bypassed (reads synthesised in memory)"}
        for route in args.routes.split(","):
            res[route] = _run_extract_route(route, eng, tasks, args.nproc, args, os.path.join(tmp, route + ".tsv"))
            print("# %s route: %s" % (route, res[route]), file=sys.stderr, flush=True)
        if "cpu" in res and "gpu" in res:
            res["gpu_over_cpu"] = round(res["gpu"]["sites_per_s"] / res["cpu"]["sites_per_s"], 2)
            res["same_sites"] = res["gpu"]["sites"] == res["cpu"]["sites"]
        res["rows_kernels"] = _rows_kernel_times(eng, args)
    finally:
        eng.close()
        import shutil
        shutil.rmtree(tmp, ignore_errors=True)
    return res


def _kernel_times(eng, args):
    """ds_extract of the reads in batches of max_batch sites with profiling on: µs per batch of each extraction kernel."""
    from deepsignal_amd.engine import ReadBatch
    _init(args.reads, args.seed, args.norm)
    recs = _device_task(list(range(args.reads)))[0]
    reads = [r[1] for r in recs]
    sr = np.concatenate([np.full(len(r[2]), i, np.int32) for i, r in enumerate(recs)])
    sl = np.concatenate([r[2] for r in recs])
    B = eng.max_batch
    nfull = len(sr) // B
    batches = [ReadBatch(reads, sr[k * B:(k + 1) * B], sl[k * B:(k + 1) * B], norm=args.norm) for k in range(nfull)]
    # only the reads a batch touches travel with it (as _rows_from_device does)
    slim = []
    for b in batches:
        used = np.unique(b.site_read)
        remap = np.full(len(reads), -1, np.int32)
        remap[used] = np.arange(len(used), dtype=np.int32)
        slim.append(ReadBatch([reads[i] for i in used], remap[b.site_read], b.site_loc, norm=args.norm))
    eng.extract(slim[0])                                # warm-up (staging blocks grow once)
    eng.set_profiling(1)
    eng.reset_stage_times()
    t0 = time.perf_counter()
    for b in slim:
        eng.extract(b)
    wall = time.perf_counter() - t0
    ks = {k["name"]: k for k in eng.kernel_stats()}
    eng.set_profiling(0)
    out = {"batches": len(slim), "sites_per_batch": B,
           "reads_per_batch": round(float(np.mean([b.desc.nreads for b in slim])), 2),
           "ds_extract_wall_us_per_batch": round(wall / len(slim) * 1e6, 1)}
    for name in ("extract_stats_kernel", "extract_sites_kernel"):
        k = ks[name]
        out[name + "_us_per_batch"] = round(k["total_ms"] * 1e3 / max(1, k["launches"]), 1)
    return out


def _forward_rate(eng, reps=20):
    from deepsignal_amd import synth
    f = synth.synthetic_features(eng.max_batch, seed=4)
    args = (f["kmer"], f["means"], f["stds"], f["sanums"], f["signals"])
    for _ in range(eng.slots):
        eng.wait(eng.submit(*args))
    t0 = time.perf_counter()
    inflight = []
    for _ in range(reps):
        if len(inflight) == eng.slots:
            eng.wait(inflight.pop(0))
        inflight.append(eng.submit(*args))
    for t in inflight:
        eng.wait(t)
    return round(reps * eng.max_batch / (time.perf_counter() - t0), 1)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--reads", type=int, default=24)
    ap.add_argument("--reads_per_task", type=int, default=2, help="reads per worker task (the f5_batch_num of the synthetic run)")
    ap.add_argument("--nproc", type=int, default=8)
    ap.add_argument("--norm", default="mad", choices=["mad", "zscore"])
    ap.add_argument("--precision", default="fp32")
    ap.add_argument("--batch_size", type=int, default=512)
    ap.add_argument("--engine_batch", type=int, default=4096)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--routes", default="cpu,gpu")
    ap.add_argument("--out", default=None)
    ap.add_argument("--mode", default="call_mods", choices=["call_mods", "extract"])
    args = ap.parse_args(argv)
    if args.mode == "extract":
        line = json.dumps(_main_extract(args))
        print(line)
        if args.out:
            with open(args.out, "w") as f:
                f.write(line + "\n")
        return
    from deepsignal_amd import weights
    from deepsignal_amd.engine import Engine
    eng = Engine(device=0, max_batch=args.engine_batch, precision=args.precision)
    eng.load_weights(weights.random_weights(seed=3, lstm_bias_std=0.1))
    try:
        tasks = [list(range(i, min(args.reads, i + args.reads_per_task))) for i in range(0, args.reads, args.reads_per_task)]
        res = {"tool": "fast5_throughput", "reads": args.reads, "nproc": args.nproc, "norm": args.norm, "precision": args.precision,
               "engine_batch": args.engine_batch, "batch_size": args.batch_size, "hdf5": "bypassed (reads synthesised in memory)"}
        for route in args.routes.split(","):
            res[route] = _run_route(route, eng, tasks, args.nproc, args)
            print("# %s route: %s" % (route, res[route]), file=sys.stderr, flush=True)
        if "cpu" in res and "gpu" in res:
            res["gpu_over_cpu"] = round(res["gpu"]["sites_per_s"] / res["cpu"]["sites_per_s"], 2)
        res["forward_only_sites_per_s"] = _forward_rate(eng)
        res["extract_kernels"] = _kernel_times(eng, args)
    finally:
        eng.close()
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
