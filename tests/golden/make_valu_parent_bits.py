"""Records tests/golden/valu_parent_bits.npz: the BITS of the fp32 forward as the commit before the vector-ALU pass over the
fp32 kernels computes them (address, index and packing work only: nothing may move), for tests/test_gpu_valu_bits.py.

Run once on an MI355X from a build of that parent commit:   python tests/golden/make_valu_parent_bits.py [out.npz]

Per case the file holds `act` and `pred` raw and, for the debug engines (three-step joint model: debug taps switch the folded
head off), the SHA-256 of every debug tap's bytes -- module1 alone is 11 MB at 130 sites, and equal digests are equal bytes.
The case list itself is stored in the file (`cases`, JSON), so the test runs exactly what was recorded:
  n = 1, 5 (fuse_min_tiles=1)   ragged last chain tiles at 4 and 2 sites per tile, every <TM> at signal_len 360
  n = 33                        a cell workgroup with one full and one ragged m-tile
  n = 130                       n % 128 != 0: the masked dense
  signal_len 128 / 200          every chain on <1> (widths 32, 16, 8) / the first chain on <2> (width 50)
each with the seeded random weights and the stress weights (hot BN channels, saturating gates)."""
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
KEYS = ("kmer", "means", "stds", "sanums", "signals")

CASES = []
for wname in ("random", "stress"):
    for n, extra in ((1, {"fuse_min_tiles": 1}), (5, {"fuse_min_tiles": 1}), (33, {}), (130, {})):
        for engine in ("threestep", "folded"):
            CASES.append({"weights": wname, "n": n, "signal_len": 360, "engine": engine, "kw": extra})
    for sl in (128, 200):
        CASES.append({"weights": wname, "n": 7, "signal_len": sl, "engine": "threestep", "kw": {"fuse_min_tiles": 1}})


def case_key(i):
    return "c%02d" % i


def weights_of(case):
    from deepsignal_amd import weights
    geom = {"signal_len": case["signal_len"]}
    if case["weights"] == "random":
        return weights.random_weights(seed=7, lstm_bias_std=0.1, **geom)
    g = np.load(os.path.join(ROOT, "tests", "golden", "stress_golden.npz"))
    head = g["stress_head"] if case["signal_len"] == 360 else None      # the committed head is the 360-sample geometry's
    return weights.stress_weights(int(g["stress_seed"]), head=head, **geom)


def tap_shapes(n, signal_len):
    from deepsignal_amd import spec
    d = spec.net_dims(signal_len=signal_len)
    shapes = {"module%d" % m: (n, d.module_width(m), 240) for m in range(1, 12)}
    shapes.update({"lstm_%s_l%d" % (dr, l): (n, 17, 256) for dr in ("fw", "bw") for l in range(3)})
    shapes.update({"signal_feat": (n, d.signal_feat), "fc1": (n, d.joint), "logits": (n, 2)})
    return shapes


def run_case(case, index):
    """-> {key: array} of one case on the GPU: act, pred and (debug engines) one digest per tap"""
    from deepsignal_amd import synth
    from deepsignal_amd.engine import Engine
    n, sl = case["n"], case["signal_len"]
    feats = synth.synthetic_features(n, seed=4100 + index, signal_len=sl)
    debug = case["engine"] == "threestep"
    eng = Engine(max_batch=256, signal_len=sl, slots=1, precision="fp32", debug=debug, fold_fc=not debug, **case["kw"])
    eng.load_weights(weights_of(case))
    act, pred = eng.run(*(feats[k] for k in KEYS))
    out = {"act": np.ascontiguousarray(act), "pred": np.ascontiguousarray(pred)}
    if debug:
        for name, shape in tap_shapes(n, sl).items():
            t = np.ascontiguousarray(eng.intermediate(name, shape))
            out["sha256_" + name] = np.frombuffer(hashlib.sha256(t.tobytes()).digest(), np.uint8).copy()
    eng.close()
    return out


def main():
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "valu_parent_bits.npz")
    rec = {"cases": np.array(json.dumps(CASES))}
    for i, case in enumerate(CASES):
        for k, v in run_case(case, i).items():
            rec[case_key(i) + "/" + k] = v
        print("recorded", i, case, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    np.savez_compressed(path, **rec)
    print("wrote %s: %d cases, %d bytes" % (path, len(CASES), os.path.getsize(path)))


if __name__ == "__main__":
    main()
