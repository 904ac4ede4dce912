"""Records tests/golden/small_kernel_parent_bits.npz: the BITS of the forward as the commit before the pass over the step's short
non-matrix kernels computes them (stem1_kernel, avgpool7_kernel, head_kernel, head_folded_kernel, gather_inputs_kernel,
scatter_outputs_kernel: issue priority, addressing and the order of independent work only -- no sum, fma chain or maximum was
reordered, so nothing may move), for tests/test_gpu_small_kernel_bits.py.

Run once on an MI355X from a build of that parent commit:   python tests/golden/make_small_kernel_parent_bits.py [out.npz]

Per case and n the file holds `act` and `pred` raw and the SHA-256 of the taps the case has (`stem_pool`: what stem1_kernel
writes; `signal_feat`: what avgpool7_kernel writes; `logits`: what the head writes) -- stem_pool alone is 1.6 MB at 70 sites,
and equal digests are equal bytes. The case list itself is stored in the file (`cases`, JSON), so the test runs exactly what
was recorded. max_batch 128, n = 1, 33, 70, fp32 with the three-step joint model unless the case says otherwise:
  default           signal_len 360: the pool at w = 23
  s100 / s90 / s40  pooled widths 7, 6 and 3: a 7-wide window clips on both sides, or everywhere
  s16               the shortest signal_len ds_create accepts: every width down to 1
  class3            class_num 3: the head's generic path
  no_rnn            is_rnn=False: J = 5520
  no_cnn            is_cnn=False: no stem, no pool launch
  bf16x3            split operands at max_batch 128: the dense leaves partial products and the head's nparts loop adds them
  folded            the folded joint model: head_folded_kernel
  hostile           signal row 0 all NaN, row 1 alternating +-1e30 (n >= 33): the stem's NaN-keeping maximum"""
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
KEYS = ("kmer", "means", "stds", "sanums", "signals")
SIZES = (1, 33, 70)
MAX_BATCH = 128
CNN_TAPS = ["stem_pool", "signal_feat", "logits"]

CASES = [
    {"name": "default", "signal_len": 360, "model": {}, "precision": "fp32", "fold": False, "taps": CNN_TAPS},
    {"name": "s100", "signal_len": 100, "model": {}, "precision": "fp32", "fold": False, "taps": CNN_TAPS},
    {"name": "s90", "signal_len": 90, "model": {}, "precision": "fp32", "fold": False, "taps": CNN_TAPS},
    {"name": "s40", "signal_len": 40, "model": {}, "precision": "fp32", "fold": False, "taps": CNN_TAPS},
    {"name": "s16", "signal_len": 16, "model": {}, "precision": "fp32", "fold": False, "taps": CNN_TAPS},
    {"name": "class3", "signal_len": 360, "model": {"class_num": 3}, "precision": "fp32", "fold": False, "taps": CNN_TAPS},
    {"name": "no_rnn", "signal_len": 360, "model": {"is_rnn": False}, "precision": "fp32", "fold": False, "taps": CNN_TAPS},
    {"name": "no_cnn", "signal_len": 360, "model": {"is_cnn": False}, "precision": "fp32", "fold": False, "taps": ["logits"]},
    {"name": "bf16x3", "signal_len": 360, "model": {}, "precision": "bf16x3", "fold": False, "taps": ["stem_pool", "logits"]},
    {"name": "folded", "signal_len": 360, "model": {}, "precision": "fp32", "fold": True, "taps": ["stem_pool", "logits"]},
    {"name": "hostile", "signal_len": 360, "model": {}, "precision": "fp32", "fold": False, "taps": CNN_TAPS, "hostile": True},
]


def case_key(index, n):
    return "c%02d_n%d" % (index, n)


def weights_of(case):
    from deepsignal_amd import weights
    return weights.random_weights(seed=7, lstm_bias_std=0.1, signal_len=case["signal_len"], **case["model"])


def features_of(case, index, n):
    from deepsignal_amd import synth
    sl = case["signal_len"]
    # (synthetic_features zeroes the tail of a few windows from a sample past the k-mer's length on: a window no longer than the
    # k-mer is the head of a longer one)
    feats = synth.synthetic_features(n, seed=7300 + 10 * index + SIZES.index(n), signal_len=max(sl, 64))
    feats["signals"] = np.ascontiguousarray(feats["signals"][:, :sl])
    if case.get("hostile"):
        feats["signals"] = np.array(feats["signals"], np.float32)
        feats["signals"][0, :] = np.nan
        if n > 1:
            feats["signals"][1, :] = np.where(np.arange(case["signal_len"]) % 2 == 0, 1e30, -1e30).astype(np.float32)
    return feats


def make_engine(case, slots=1, w=None):
    from deepsignal_amd.engine import Engine
    eng = Engine(max_batch=MAX_BATCH, signal_len=case["signal_len"], slots=slots, precision=case["precision"], fold_fc=case["fold"],
                 fuse_min_tiles=1, **case["model"])
    eng.load_weights(weights_of(case) if w is None else w)
    return eng


def tap_shape(case, name, n):
    from deepsignal_amd import spec
    d = spec.net_dims(signal_len=case["signal_len"], **{k: v for k, v in case["model"].items() if k != "class_num"})
    return {"stem_pool": (n, d.w_a, 64), "module11": (n, d.w_c, 240), "signal_feat": (n, d.w_c * 240),
            "logits": (n, case["model"].get("class_num", 2))}[name]


def run_case(case, index, eng=None):
    """-> {key: array} of one case on the GPU, every n in SIZES: act, pred and one digest per tap"""
    own = eng is None
    if own:
        eng = make_engine(case)
    out = {}
    for n in SIZES:
        feats = features_of(case, index, n)
        act, pred = eng.run(*(feats[k] for k in KEYS))
        key = case_key(index, n)
        out[key + "/act"] = np.ascontiguousarray(act)
        out[key + "/pred"] = np.ascontiguousarray(pred)
        for name in case["taps"]:
            t = np.ascontiguousarray(eng.intermediate(name, tap_shape(case, name, n)))
            out[key + "/sha256_" + name] = np.frombuffer(hashlib.sha256(t.tobytes()).digest(), np.uint8).copy()
    if own:
        eng.close()
    return out


def main():
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "small_kernel_parent_bits.npz")
    rec = {"cases": np.array(json.dumps(CASES))}
    for i, case in enumerate(CASES):
        rec.update(run_case(case, i))
        print("recorded", i, case["name"], flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    np.savez_compressed(path, **rec)
    print("wrote %s: %d cases, %d bytes" % (path, len(CASES), os.path.getsize(path)))


if __name__ == "__main__":
    main()
