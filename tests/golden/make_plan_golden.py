"""Generate tests/golden/plan_kernels.json -- which kernels the forward planner launches, and what it books per stage.

The host planner (deepsignal_amd/csrc/ds_engine.cpp) chooses one kernel variant per launch from the precision, the tuning
flags, the BiLSTM tiling and the sites per forward. This fixture pins that choice: for every case below, after eager
forwards with `set_profiling(1)`, the `(kernel name, launches)` pairs of `kernel_stats()` with launches > 0 and the whole
`stage_times()` table as `(name, launches, flops_per_site)` in order. tests/test_gpu_plan_kernels.py replays the cases and
asserts equality (flops_per_site are exact doubles; JSON round-trips them).

The fixture is a record of the engine as it was BEFORE a change to the planner: regenerate it from the parent commit of
such a change, never from the change itself. Needs the GPU. Run: python tests/golden/make_plan_golden.py
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

FIXTURE = os.path.join(HERE, "plan_kernels.json")
KEYS = ("kmer", "means", "stds", "sanums", "signals")
PRECISIONS = ("fp32", "bf16", "bf16_all", "bf16x3")
TILINGS = ("auto", "narrow", "wide", "lds1", "lds2", "wide8")
# kernel-table entries no configuration launches from a forward: the grouped-GEMM BiLSTM configurations the dedicated cell
# kernels replaced, the wide conv tile and the two-n-tile fp32 cell (kept: recorded profiles are keyed by position and
# name), and the two feature-extraction kernels, which ds_extract books (tests/test_gpu_extract.py), not a forward
NEVER_LAUNCHED = {
    "gemm_kernel<1,4,4,1,1,0,1,1>", "gemm_kernel<1,4,4,1,1,2,1,1>", "gemm_kernel<1,4,4,1,1,0,3,1,bf16>",
    "gemm_kernel<1,4,4,1,1,2,3,1,bf16>", "gemm_kernel<1,1,4,1,2,0,1,1>", "gemm_kernel<1,1,4,1,2,2,1,1>",
    "gemm_kernel<1,1,4,1,2,0,3,1,bf16>", "gemm_kernel<1,1,4,1,2,2,3,1,bf16>", "gemm_kernel<2,2,2,2,0,0,1,1>",
    "lstm_cell_kernel<2>", "extract_stats_kernel", "extract_sites_kernel",
}


def cases():
    """(id, Engine keyword arguments, sites of each forward) of every case."""
    out = []
    variants = (("default", {}), ("no_fused", {"no_fused": True}), ("three_step", {"fold_fc": False}),
                ("no_chain", {"chain_modules": False}), ("debug", {"debug": True}), ("serial", {"serial": True}))
    for prec in PRECISIONS:
        for vname, kw in variants:
            if prec == "bf16x3" and vname == "no_fused":
                continue      # refused by ds_create: the mode runs the fused inception kernels only (tests/test_gpu_split.py)
            for n in (96, 1100, 2048):
                out.append(("%s-%s-%d" % (prec, vname, n), dict(kw, precision=prec, max_batch=n), [n]))
        for tiling in TILINGS:
            out.append(("%s-tiling_%s-1100" % (prec, tiling), dict(precision=prec, max_batch=1100, lstm_tiling=tiling), [1100]))
    x3 = dict(precision="bf16x3", max_batch=1100)
    for xp in (True, "all", False):
        out.append(("bf16x3-xproj_%s-1100" % str(xp).lower(), dict(x3, lstm_xproj=xp), [1100]))
    out.append(("bf16x3-dense_narrow-1100", dict(x3, split_dense_narrow=True), [1100]))
    out.append(("bf16x3-dense_narrow-three_step-1100", dict(x3, split_dense_narrow=True, fold_fc=False), [1100]))
    out.append(("bf16x3-ragged-1100-77", dict(x3), [1100, 77]))
    out.append(("bf16x3-ragged-three_step-1100-77", dict(x3, fold_fc=False), [1100, 77]))
    for prec in ("fp32", "bf16x3"):
        out.append(("%s-cnn_only-1100" % prec, dict(precision=prec, max_batch=1100, is_rnn=False), [1100]))
        out.append(("%s-rnn_only-1100" % prec, dict(precision=prec, max_batch=1100, is_cnn=False), [1100]))
    return out


_weights, _feats = {}, {}


def replay(engine_kw, forwards):
    """Run the case on the library under test; returns (kernels, stages) as the fixture stores them and the kernel table's names."""
    from deepsignal_amd import synth, weights
    from deepsignal_amd.engine import Engine
    net = (engine_kw.get("is_cnn", True), engine_kw.get("is_rnn", True))
    if net not in _weights:
        _weights[net] = weights.random_weights(seed=7, lstm_bias_std=0.1, is_cnn=net[0], is_rnn=net[1])
    eng = Engine(slots=1, **engine_kw)
    try:
        eng.load_weights(_weights[net])
        eng.set_profiling(1)
        for n in forwards:
            if n not in _feats:
                _feats[n] = synth.synthetic_features(n, seed=5000 + n)
            eng.run(*(_feats[n][k] for k in KEYS))
        kernels = [[k["name"], k["launches"]] for k in eng.kernel_stats() if k["launches"] > 0]
        stages = [[s["name"], s["launches"], s["flops_per_site"]] for s in eng.stage_times()]
        names = [k["name"] for k in eng.kernel_stats()]
    finally:
        eng.close()
    return kernels, stages, names


def main():
    recorded, seen, names = [], set(), []
    for cid, kw, forwards in cases():
        kernels, stages, names = replay(kw, forwards)
        seen.update(k for k, _ in kernels)
        recorded.append({"id": cid, "engine": kw, "forwards": forwards, "kernels": kernels, "stages": stages})
        print("%-44s %2d kernels, %2d stages" % (cid, len(kernels), len(stages)), flush=True)
    with open(FIXTURE, "w") as f:
        f.write('{"kernel_table": %s,\n"cases": [\n%s\n]}\n' % (json.dumps(names), ",\n".join(json.dumps(c) for c in recorded)))
    never = [k for k in names if k not in seen]
    print("kernel-table entries never launched (%d of %d):" % (len(never), len(names)))
    for k in never:
        print("  %s%s" % (k, "" if k in NEVER_LAUNCHED else "   <-- UNEXPECTED: add a case that reaches it"))
    print("wrote %s: %d cases" % (FIXTURE, len(recorded)))
    return 0 if set(never) <= NEVER_LAUNCHED else 1


if __name__ == "__main__":
    sys.exit(main())
