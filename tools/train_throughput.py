"""Throughput of the training step (ds_train_step) at denoise's defaults -- batch 512, T = 17, keep_prob 0.5 -- in steps/s and
samples/s from wall time, device milliseconds per phase from ds_get_train_times, and the fraction of the fp32 matrix peak on the
step's algorithmic FLOPs. The only baseline there is: the float32 torch statement (tests/train_statement.py) on the usable CPU
cores. Writes profiles/train_throughput.json.

    python tools/train_throughput.py [--steps 30] [--warmup 5] [--cpu_steps 2] [--is_base no] [--out profiles/train_throughput.json]
    python tools/train_throughput.py --parity [--out profiles/train_parity.json]
    python tools/train_throughput.py --variant signal [--signal_len 360] [--cpu_steps 1] [--out profiles/train_throughput_signal.json]
    python tools/train_throughput.py --digest [--against other_side.json] [--out profiles/train_runs_digest.json]

--parity writes the distances tests/test_gpu_train_grad.py asserts on (GPU and float32 statement against the float64 statement,
per case and tensor) instead. --is_base yes times the step with the embedding trained (ds_train_step_base, codes uniform over
A, C, G, T); the default no is the step denoise runs, through ds_train_step. --variant signal times the signal-only model's step
(ds_train_step_signal: stem, eleven inception modules, joint layers at J = w_c x 240) on normal signals; its CPU baseline is
tests/train_statement_signal.py in float32, one step without a warm-up (a step takes far longer than any start-up cost).
--cpu_steps 0 skips the CPU baseline, which is what a comparison of two builds wants.

--digest is a refactor's proof that no bit moved: small runs of the three variants (RNN-only, is_base, signal at signal_len 40;
max_batch 8, n 6, kmer_len 5, keep_prob 0.5, pos_weight 1 and 3), three steps and one evaluation each, and a sha256 per quantity:
the loss of every step, the evaluation's loss, prediction and logits, every tensor (a signal run's moving statistics among them),
gradient and mask stream after the third step, and a signal run's taps. It uses public Engine methods only, so the same file runs
in a checkout of another commit. Alone it writes the sha256 per quantity. --against names the file another commit wrote that way:
what is written then is both sides by group of quantities (one combined sha256 per side, how many of the group's quantities differ)
and the first quantity that differs, and the exit status is 1 if any does."""
import argparse
import hashlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

FP32_MATRIX_PEAK = 157.3e12      # MI355X, v_mfma_f32_32x32x2_f32


def step_flops(n, T, in0=3):
    """Algorithmic FLOPs of one step: the forward's matrix products, and twice that for the backward (d[x | h] and dK)."""
    rows = (in0 + 256) + 2 * (256 + 256)
    fwd = 2 * T * n * 2 * rows * 1024 + 2 * n * 512 * 512 + 2 * n * 512 * 2
    return fwd, 2 * fwd


def usable_cores():
    n = os.cpu_count() or 1
    try:
        n = min(n, len(os.sched_getaffinity(0)))
    except (AttributeError, OSError):
        pass
    return max(1, min(n, 16))


def throughput(a):
    import torch
    import train_statement as ts
    from deepsignal_amd import weights
    from deepsignal_amd.engine import Engine
    n, T = a.batch, a.kmer_len
    base = a.is_base == "yes"
    if base:
        import train_statement_base as ts
    w = weights.random_weights(seed=7, is_cnn=False, is_base=base, kmer_len=T)
    feats = ts.train_features(n, T, seed=1)
    labels = np.random.default_rng(2).integers(0, 2, n).astype(np.int32)
    eng = Engine(kmer_len=T, max_batch=n, is_cnn=False, is_base=base, device=a.device)
    eng.load_weights(w)
    eng.train_begin(keep_prob=a.keep_prob, seed=3, base=base)
    kmer = feats["kmer"] if base else None
    for _ in range(a.warmup):
        eng.train_step(feats["means"], feats["stds"], feats["sanums"], labels, 1e-3, kmer=kmer)
    eng.train_times(reset=True)
    t0 = time.perf_counter()
    for _ in range(a.steps):
        loss, _ = eng.train_step(feats["means"], feats["stds"], feats["sanums"], labels, 1e-3, kmer=kmer)
    wall = time.perf_counter() - t0
    times = eng.train_times()
    eng.close()
    fwd, bwd = step_flops(n, T, 131 if base else 3)
    device_ms = sum(times["ms"].values()) / times["steps"]
    out = {"is_base": a.is_base, "batch": n, "kmer_len": T, "keep_prob": a.keep_prob, "steps": a.steps, "warmup": a.warmup, "last_loss": loss,
           "steps_per_s": a.steps / wall, "samples_per_s": a.steps * n / wall, "wall_ms_per_step": 1e3 * wall / a.steps,
           "device_ms_per_step": device_ms, "device_ms_per_phase": {k: v / times["steps"] for k, v in times["ms"].items()},
           "gflop_per_step": {"forward": fwd / 1e9, "backward": bwd / 1e9},
           "fraction_of_fp32_matrix_peak": (fwd + bwd) / (device_ms * 1e-3) / FP32_MATRIX_PEAK}
    if a.cpu_steps > 0:
        cores = usable_cores()
        torch.set_num_threads(cores)
        ts.step(w, feats, labels, None, 1.0, 1.0, torch.float32)          # warm-up
        t0 = time.perf_counter()
        for _ in range(a.cpu_steps):
            ts.step(w, feats, labels, None, 1.0, 1.0, torch.float32)
        cpu = (time.perf_counter() - t0) / a.cpu_steps
        out["cpu_statement"] = {"what": "tests/%s.py, float32" % ts.__name__ + ", forward + autograd backward (no optimiser)", "cores": cores,
                                "s_per_step": cpu, "samples_per_s": n / cpu}
    return out


def throughput_signal(a):
    import torch
    import train_statement_signal as tss
    from deepsignal_amd import spec, weights
    from deepsignal_amd.engine import Engine
    n, S = a.batch, a.signal_len
    J = tss.dims(S).joint
    w = weights.random_weights(seed=7, signal_len=S, is_cnn=True, is_rnn=False, randomize_bn=True)
    rng = np.random.default_rng(1)
    signals, labels = rng.normal(0.0, 1.0, (n, S)).astype(np.float32), rng.integers(0, 2, n).astype(np.int32)
    eng = Engine(signal_len=S, max_batch=n, is_cnn=True, is_rnn=False, device=a.device)
    eng.load_weights(w)
    eng.train_begin(keep_prob=a.keep_prob, seed=3)
    for _ in range(a.warmup):
        eng.train_step_signal(signals, labels, 1e-3)
    eng.train_times(reset=True)
    t0 = time.perf_counter()
    for _ in range(a.steps):
        loss, _ = eng.train_step_signal(signals, labels, 1e-3)
    wall = time.perf_counter() - t0
    times = eng.train_times()
    eng.close()
    # the forward's matrix products: the convolutions (spec.FLOPS_CONV_PER_SITE at signal_len 360, in proportion otherwise) and the
    # two dense layers; the backward twice that (data and weight gradients)
    fwd = n * (spec.FLOPS_CONV_PER_SITE * S / 360.0 + 2.0 * J * J + 2.0 * J * 2)
    device_ms = sum(times["ms"].values()) / times["steps"]
    out = {"variant": "signal", "note": "measured once, not tuned", "batch": n, "signal_len": S, "joint": J, "keep_prob": a.keep_prob, "steps": a.steps,
           "warmup": a.warmup, "last_loss": loss, "steps_per_s": a.steps / wall, "samples_per_s": a.steps * n / wall,
           "wall_ms_per_step": 1e3 * wall / a.steps, "device_ms_per_step": device_ms,
           "device_ms_per_phase": {k: v / times["steps"] for k, v in times["ms"].items()},
           "gflop_per_step": {"forward": fwd / 1e9, "backward": 2 * fwd / 1e9},
           "fraction_of_fp32_matrix_peak": 3 * fwd / (device_ms * 1e-3) / FP32_MATRIX_PEAK}
    if a.cpu_steps > 0:
        cores = usable_cores()
        torch.set_num_threads(cores)
        t0 = time.perf_counter()
        for _ in range(a.cpu_steps):
            tss.step(w, signals, labels, None, 1.0, 1.0, torch.float32)
        cpu = (time.perf_counter() - t0) / a.cpu_steps
        out["cpu_statement"] = {"what": "tests/train_statement_signal.py, float32, forward + autograd backward (no optimiser), no warm-up", "cores": cores,
                                "s_per_step": cpu, "samples_per_s": n / cpu}
    return out


def digest(a):
    from deepsignal_amd import engine, weights
    n, B, T, S, keep_prob = 6, 8, 5, 40, 0.5
    rng = np.random.default_rng(11)
    rows = {"means": rng.normal(0.0, 1.0, (n, T)).astype(np.float32), "stds": rng.uniform(0.05, 1.0, (n, T)).astype(np.float32),
            "sanums": rng.integers(1, 60, (n, T)).astype(np.float32)}
    kmer = rng.integers(0, 1024, (n, T)).astype(np.int32)
    signals = rng.normal(0.0, 1.0, (n, S)).astype(np.float32)
    labels = np.array([0, 1, 1, 0, 1, 0], np.int32)
    out = {}

    def put(key, value):
        out[key] = hashlib.sha256(np.ascontiguousarray(value).tobytes()).hexdigest()

    for variant in ("rnn", "base", "signal"):
        for pos_weight in (1.0, 3.0):
            tag = "%s/pos_weight_%g/" % (variant, pos_weight)
            if variant == "signal":
                w = weights.random_weights(seed=7, signal_len=S, is_cnn=True, is_rnn=False, randomize_bn=True)
                eng = engine.Engine(signal_len=S, max_batch=B, is_cnn=True, is_rnn=False, device=a.device)
                step = lambda: eng.train_step_signal(signals, labels, 1e-3)
                evaluate = lambda: eng.train_eval_signal(signals, labels)
                streams = engine.SIGNAL_MASK_STREAMS
            else:
                base = variant == "base"
                w = weights.random_weights(seed=7, is_cnn=False, is_base=base, kmer_len=T)
                eng = engine.Engine(kmer_len=T, max_batch=B, is_cnn=False, is_base=base, device=a.device)
                step = lambda: eng.train_step(rows["means"], rows["stds"], rows["sanums"], labels, 1e-3, kmer=kmer if base else None)
                evaluate = lambda: eng.train_eval(rows["means"], rows["stds"], rows["sanums"], labels, kmer=kmer if base else None)
                streams = engine.MASK_STREAMS
            eng.load_weights(w)
            eng.train_begin(keep_prob=keep_prob, pos_weight=pos_weight, seed=3, base=variant == "base")
            for k in range(3):
                loss, pred = step()
                put(tag + "step%d/loss" % k, np.float32(loss))
                put(tag + "step%d/prediction" % k, pred)
            for name, v in eng.train_tensors().items():
                put(tag + "tensor/" + name, v)
            for name, v in eng.train_grads().items():
                put(tag + "gradient/" + name, v)
            for name in streams:
                put(tag + "mask/" + name, eng.train_mask(name, n))
            if variant == "signal":
                for name in engine.signal_tap_names():
                    put(tag + "tap/" + name, eng.train_tap(name, n))
            loss, pred, logits = evaluate()
            put(tag + "eval/loss", np.float32(loss))
            put(tag + "eval/prediction", pred)
            put(tag + "eval/logits", logits)
            eng.close()
    if not a.against:
        return out
    with open(a.against) as f:
        other = json.load(f)
    return compare_digests(other, out, {"max_batch": B, "n": n, "kmer_len": T, "signal_len": S, "keep_prob": keep_prob, "steps": 3, "lr": 1e-3})


def compare_digests(parent, change, shape):
    """Both sides in one record that stays readable: the quantities go by group (variant / pos_weight / kind: the steps' and the
    evaluation's outputs, tensor, gradient, mask, tap), and a group carries one sha256 per side over its `key=sha256` lines in key
    order, its number of quantities and how many of them differ."""
    def group(key):
        part = key.split("/")
        return "/".join(part[:2] + [part[2] if part[2] in ("tensor", "gradient", "mask", "tap") else "outputs"])

    def combined(side, keys):
        return hashlib.sha256("".join("%s=%s\n" % (k, side.get(k)) for k in keys).encode()).hexdigest()

    keys = sorted(set(parent) | set(change))
    differ = [k for k in keys if parent.get(k) != change.get(k)]
    groups = {}
    for name in sorted(set(map(group, keys))):
        mine = [k for k in keys if group(k) == name]
        groups[name] = {"quantities": len(mine), "differ": sum(parent.get(k) != change.get(k) for k in mine),
                        "parent": combined(parent, mine), "change": combined(change, mine)}
    # the first differing quantity in the order the run produced them (the change's insertion order: steps, tensors, ..., evaluation)
    first = next((k for k in change if parent.get(k) != change[k]), differ[0] if differ else None)
    return {"shape": shape, "quantities": len(keys), "differ": len(differ), "first_differing": first,
            "differing_outputs": [k for k in differ if group(k).endswith("/outputs")], "groups": groups}


def parity(a):
    import torch
    import test_gpu_train_grad as cases
    import train_statement as ts
    from deepsignal_amd import engine
    out = []
    for n, T, keep_prob, pos_weight, wkind, lkind in cases.CASES:
        w, feats, labels = cases._weights(wkind, T), ts.train_features(n, T, seed=1000 + n), cases._labels(lkind, n)
        eng = engine.Engine(kmer_len=T, max_batch=cases.MAX_BATCH, is_cnn=False, is_base=False, device=a.device)
        eng.load_weights(w)
        eng.train_begin(keep_prob=keep_prob, pos_weight=pos_weight, seed=cases.SEED)
        loss, _ = eng.train_step(feats["means"], feats["stds"], feats["sanums"], labels, 0.0)
        masks = {s: eng.train_mask(s, n) for s in engine.MASK_STREAMS}
        grads = eng.train_grads()
        eng.close()
        l64, _, g64 = ts.step(w, feats, labels, masks, keep_prob, pos_weight, torch.float64)
        l32, _, g32 = ts.step(w, feats, labels, masks, keep_prob, pos_weight, torch.float32)
        out.append({"n": n, "T": T, "keep_prob": keep_prob, "pos_weight": pos_weight, "weights": wkind, "labels": lkind,
                    "loss": {"gpu": loss, "f64": l64, "gpu_distance": abs(loss - l64), "f32_statement_distance": abs(l32 - l64)},
                    "gradient": {k: {"gpu": ts.rel_err(grads[k], g64[k]), "f32_statement": ts.rel_err(g32[k], g64[k])} for k in ts.tensor_names()}})
    return {"distance": "max |g - g_64| / max |g_64| per tensor; bar of the test: 4 x max(f32_statement, 1e-6)", "cases": out}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--batch", type=int, default=512)
    ap.add_argument("--kmer_len", type=int, default=17)
    ap.add_argument("--keep_prob", type=float, default=0.5)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--cpu_steps", type=int, default=2, help="steps of the CPU statement to time (0: skip)")
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--is_base", default="no", choices=["yes", "no"], help="yes: the embedding is trained too (default no: denoise's step)")
    ap.add_argument("--variant", default="rnn", choices=["rnn", "signal"], help="signal: the signal-only model's step (ds_train_step_signal)")
    ap.add_argument("--signal_len", type=int, default=360)
    ap.add_argument("--parity", action="store_true")
    ap.add_argument("--digest", action="store_true", help="sha256 of every quantity of small runs of the three variants")
    ap.add_argument("--against", default=None, help="with --digest: the digest another commit wrote, to be recorded and compared with")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.variant == "signal" and a.parity:
        ap.error("--parity covers the BiLSTM step; the signal step's distances are printed by tests/test_gpu_train_signal_grad.py")
    result = digest(a) if a.digest else parity(a) if a.parity else throughput_signal(a) if a.variant == "signal" else throughput(a)
    default = "train_runs_digest.json" if a.digest else "train_parity.json" if a.parity else "train_throughput_signal.json" if a.variant == "signal" else "train_throughput.json"
    path = a.out or os.path.join(ROOT, "profiles", default)
    with open(path, "w") as f:
        json.dump(result, f, indent=1, sort_keys=True)
        f.write("\n")
    if a.digest:
        differ = result["differ"] if a.against else 0
        print(json.dumps({"quantities": result["quantities"] if a.against else len(result), "differ": differ, "written": path}, sort_keys=True))
        return 1 if differ else 0
    print(json.dumps(result if not a.parity else {"cases": len(result["cases"]), "written": path}, sort_keys=True))
    return 0


if __name__ == "__main__":
    sys.exit(main())
