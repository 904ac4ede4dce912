"""A/B of DS_PRECISION_BF16X3 against DS_PRECISION_FP16X2 in ONE process on ONE box (measuring-on-mi355x: never compare numbers from
two boxes or two processes). Both precisions, the three-step (fold_fc=False) and the folded (default) engine, batch 512 with 8 slots,
resident inputs, captured graphs:

    python tools/fp16x2_ab.py [runs=5] [steps=40] [out=profiles/fp16x2_ab.json]

The four engines stay alive for the whole measurement and take turns: run r measures bf16x3 then fp16x2 (odd r: the other way round),
so drift of the box's clocks falls on both. A run = `steps` pipelined forwards, timed from the first submit to ds_sync; every engine
is warmed first. Then, with graphs off and per-kernel profiling on, a few forwards per engine give the per-kernel times of
ds_get_kernel_stat (us per launch). Verdict per engine kind: every fp16x2 run faster than bf16x3's FASTEST run, or not."""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from deepsignal_amd import synth, weights as W  # noqa: E402
from deepsignal_amd.engine import Engine  # noqa: E402

KEYS = ("kmer", "means", "stds", "sanums", "signals")
B, SLOTS = 512, 8


def main():
    runs = int(sys.argv[1]) if len(sys.argv) > 1 else 5
    steps = int(sys.argv[2]) if len(sys.argv) > 2 else 40
    out = sys.argv[3] if len(sys.argv) > 3 else os.path.join("profiles", "fp16x2_ab.json")
    assert runs >= 4, "at least four runs per precision"
    dev = torch.device("cuda", 0)
    f = synth.synthetic_features(B, seed=1)
    d = {k: torch.from_numpy(f[k]).to(dev) for k in KEYS}
    act = torch.zeros((B, 2), dtype=torch.float32, device=dev)
    pred = torch.zeros((B,), dtype=torch.int32, device=dev)
    w = W.random_weights(seed=W.WEIGHT_SEED)
    eng = {}
    for kind, fold in (("three_step", False), ("folded", True)):
        for prec in ("bf16x3", "fp16x2"):
            e = Engine(device=0, max_batch=B, slots=SLOTS, precision=prec, fold_fc=fold)
            e.load_weights(w)
            eng[kind, prec] = e

    def window(e, n):
        t0 = time.perf_counter()
        for _ in range(n):
            e.run_device(B, *(d[k].data_ptr() for k in KEYS), act.data_ptr(), pred.data_ptr())
        e.sync()
        return (time.perf_counter() - t0) / n * 1e6      # us per forward of 512 sites

    for e in eng.values():
        window(e, 20)
    res = {}
    for kind in ("three_step", "folded"):
        t = {"bf16x3": [], "fp16x2": []}
        for r in range(runs):
            order = ("bf16x3", "fp16x2") if r % 2 == 0 else ("fp16x2", "bf16x3")
            for prec in order:
                t[prec].append(round(window(eng[kind, prec], steps), 2))
        fastest3 = min(t["bf16x3"])
        res[kind] = {"us_per_forward": t, "sites_per_s_median": {p: round(B / (sorted(v)[len(v) // 2] * 1e-6)) for p, v in t.items()},
                     "bf16x3_fastest_us": fastest3, "fp16x2_slowest_us": max(t["fp16x2"]),
                     "spread_us": {p: round(max(v) - min(v), 2) for p, v in t.items()},
                     "every_fp16x2_run_faster_than_the_fastest_bf16x3_run": max(t["fp16x2"]) < fastest3}
        print(kind, json.dumps(res[kind]), flush=True)
    # per-kernel times: graphs off, profiling per kernel
    kern = {}
    for (kind, prec), e in eng.items():
        e.sync()
        e.set_graph(False)
        e.set_profiling(1)
        window(e, 6)
        kern["%s/%s" % (kind, prec)] = {k["name"]: k for k in e.kernel_stats() if k["launches"]}
        e.set_profiling(0)
    for e in eng.values():
        e.close()
    rec = {"batch": B, "slots": SLOTS, "runs": runs, "steps_per_run": steps, "device": torch.cuda.get_device_name(0), "engines": res, "kernels": kern}
    os.makedirs(os.path.dirname(out) or ".", exist_ok=True)
    json.dump(rec, open(out, "w"), indent=1, sort_keys=True)
    print("wrote", out)


if __name__ == "__main__":
    main()
