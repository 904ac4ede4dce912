"""What cascaded precision (`call_mods --precision bf16_all --recheck_margin M`) buys in sites per second.

    python tools/recheck_throughput.py [--batch 4096] [--batches 4] [--rounds 5] [--out profiles/recheck_throughput.json]

Weights: `weights.stress_weights` with the committed head (tests/golden/stress_golden.npz) -- a stand-in for a trained model:
saturating gates, logits spanning +-10, both labels. The share of sites inside a margin depends on the model; a really trained
checkpoint may show another one. Features: `synth.synthetic_features`. Every configuration is driven the way call_mods drives
the engine: host arrays through submit / wait, every pipeline slot in flight.

Measured, each in a child process of its own under `timeout`, the next one started only when the one before succeeded:
  * bf16_all, bf16x3 and fp32 alone;
  * the cascade bf16_all -> fp32 and bf16_all -> bf16x3 at margins 0.05, 0.1, 0.2 and 0.4, with the share of sites rechecked;
  * the selection kernel's device microseconds per batch (profiling run at margin 0.1).
"""
import argparse
import collections
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

KEYS = ("kmer", "means", "stds", "sanums", "signals")
MARGINS = (0.05, 0.1, 0.2, 0.4)
FINE = ("fp32", "bf16x3")
STEP_TIMEOUT_S = 240


def _weights():
    import numpy as np
    from deepsignal_amd import weights
    g = np.load(os.path.join(ROOT, "tests", "golden", "stress_golden.npz"))
    return weights.stress_weights(int(g["stress_seed"]), head=g["stress_head"])


def _pass(eng, feats, batch, nb):
    inflight = collections.deque()
    for b in range(nb):
        if len(inflight) == eng.slots:
            eng.wait(inflight.popleft())
        inflight.append(eng.submit(*(feats[k][b * batch:(b + 1) * batch] for k in KEYS)))
    while inflight:
        eng.wait(inflight.popleft())


def step(args):
    """One configuration in this process: prints one JSON line."""
    from deepsignal_amd import synth
    from deepsignal_amd.engine import Engine
    w = _weights()
    feats = synth.synthetic_features(args.batch * args.batches, seed=77)
    eng = Engine(device=0, max_batch=args.batch, precision=args.precision)
    eng.load_weights(w)
    fine = None
    res = {"precision": args.precision, "batch": args.batch, "sites_per_round": args.batch * args.batches, "rounds": args.rounds}
    if args.margin > 0:
        fine = Engine(device=0, max_batch=args.batch, precision=args.fine)
        fine.load_weights(w)
        eng.set_recheck(fine, args.margin, own=True)
        res.update(margin=args.margin, fine=args.fine)
    _pass(eng, feats, args.batch, args.batches)                       # warm-up: plans, graphs, pinned buffers of every slot
    _pass(eng, feats, args.batch, args.batches)
    if fine is not None:
        eng.set_recheck(fine, args.margin, own=True)                  # restart the counters
    t0 = time.perf_counter()
    for _ in range(args.rounds):
        _pass(eng, feats, args.batch, args.batches)
    dt = time.perf_counter() - t0
    res["sites_per_s"] = round(args.rounds * args.batch * args.batches / dt, 1)
    if fine is not None:
        st = eng.recheck_stats()
        res.update(share=round(st["rechecked"] / max(1, st["sites"]), 5), fine_forwards_per_batch=round(
            st["fine_forwards"] / (args.rounds * args.batches), 3))
        if args.select_time:
            eng.set_profiling(1)
            one = [feats[k][:args.batch] for k in KEYS]
            eng.run(*one)
            eng.recheck_times(reset=True)
            for _ in range(5):
                eng.run(*one)
            t = eng.recheck_times()
            eng.set_profiling(0)
            res["select_kernel_us_per_batch"] = round(1e3 * t["select_ms"] / max(1, t["launches"]), 2)
    eng.close()
    print("RESULT " + json.dumps(res, sort_keys=True), flush=True)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--batches", type=int, default=4, help="distinct batches per round")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "recheck_throughput.json"))
    ap.add_argument("--step", action="store_true", help="(internal) run one configuration in this process")
    ap.add_argument("--precision", default="bf16_all")
    ap.add_argument("--fine", default="fp32")
    ap.add_argument("--margin", type=float, default=0.0)
    ap.add_argument("--select_time", action="store_true")
    args = ap.parse_args(argv)
    if args.step:
        step(args)
        return 0
    configs = [("bf16_all", None, 0.0), ("bf16x3", None, 0.0), ("fp32", None, 0.0)]
    configs += [("bf16_all", fine, m) for fine in FINE for m in MARGINS]
    out = {"tool": "recheck_throughput", "weights": "weights.stress_weights + tests/golden/stress_golden.npz head (stands in for a "
           "trained model)", "features": "synth.synthetic_features", "batch": args.batch, "alone": {}, "cascade": []}
    status = 0
    for precision, fine, margin in configs:
        cmd = ["timeout", "-k", "10", str(STEP_TIMEOUT_S), sys.executable, os.path.abspath(__file__), "--step", "--batch", str(args.batch),
               "--batches", str(args.batches), "--rounds", str(args.rounds), "--precision", precision, "--margin", str(margin)]
        if fine:
            cmd += ["--fine", fine]
            if margin == 0.1:
                cmd.append("--select_time")
        r = subprocess.run(cmd, capture_output=True, text=True)
        line = [l for l in r.stdout.splitlines() if l.startswith("RESULT ")]
        if r.returncode != 0 or not line:
            # nothing more is started on the GPU after a step that failed or ran out of time
            print("step %s failed (exit %d):\n%s" % (cmd[6:], r.returncode, r.stderr[-2000:]), file=sys.stderr)
            out["failed_step"] = {"precision": precision, "fine": fine, "margin": margin, "exit": r.returncode}
            status = 1
            break
        res = json.loads(line[0][7:])
        print(json.dumps(res, sort_keys=True), flush=True)
        if fine:
            out["cascade"].append(res)
        else:
            out["alone"][precision] = res["sites_per_s"]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    return status


if __name__ == "__main__":
    sys.exit(main())
