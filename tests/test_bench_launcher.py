"""bench.py's launch contract on a CPU-only box: `python bench.py --gpus N` with no launcher environment must start its
own ranks (fresh child processes, spawned before the parent touches the GPU) and print ONE JSON line. `--dry-run` swaps
the engine for a stub and RCCL for gloo, so what runs here is the launcher, the barriers, the result gather and the
JSON plumbing -- not a measurement (the line says so)."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(*flags):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--dry-run", *flags], env=env, cwd=ROOT,
                         stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert out.returncode == 0, out.stderr.decode()[-2000:]
    lines = [l for l in out.stdout.decode().splitlines() if l.startswith("{")]
    assert len(lines) == 1, out.stdout.decode()
    return json.loads(lines[0])


def test_gpus_2_self_launches_two_ranks():
    r = _run("--gpus", "2", "--steps", "20", "--warmup", "5", "--full")
    assert r["n_gpus"] == 2 and r["steps"] == 20 and r["warmup"] == 5 and r["dry_run"] is True
    assert r["scaling"] == "weak" and r["unit"] == "sites/s" and r["windows"]["n"] == 5
    assert "2 rank(s)" in r["config"]["sharding"]


def test_gpus_1_line_has_the_contract_keys():
    r = _run("--steps", "4", "--warmup", "1", "--windows", "3")
    for key in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
                "vs_baseline", "dtype", "data", "config"):
        assert key in r
    assert r["n_gpus"] == 1 and r["windows"]["n"] == 3 and r["vs_baseline"] is None


def test_plain_run_times_exactly_the_given_steps_and_dumps_the_last_one(tmp_path):
    """A plain run is ONE window of exactly --steps steps; --dump-outputs writes the last step's results as float32 .npy."""
    import numpy as np
    r = _run("--steps", "6", "--warmup", "2", "--dump-outputs", str(tmp_path))
    assert r["steps"] == 6 and r["warmup"] == 2 and r["windows"]["n"] == 1 and r["windows"]["steps_each"] == 6
    act, pred = np.load(os.path.join(str(tmp_path), "act.npy")), np.load(os.path.join(str(tmp_path), "pred.npy"))
    assert act.shape == (512, 2) and act.dtype == np.float32
    assert pred.shape == (512,) and pred.dtype == np.float32


# what moved behind --full: a plain run computes none of it
FULL_ONLY = ("roofline", "kernels", "stages_us_per_step", "pcie_inclusive", "ds_forward_blocking", "fast_mode_folded", "e2e_tsv",
             "e2e_tsv_sharded", "fp32_class_bf16x3", "configs2_bf16_batch4096", "e2e_tsv_bf16_all", "cpu_baseline")


@pytest.mark.gpu
def test_plain_bench_is_the_headline_alone_and_its_dump_is_the_last_step(tmp_path):
    """`bench.py --gpus 1 --steps K --warmup W --dump-outputs DIR` on the GPU: the contract keys, one window of K steps, none of
    the --full legs, and DIR/act.npy / pred.npy are the three-step engine's results for the batch the last step ran
    (batch (K - 1) % 8 of the seeded synthetic pool, seeded weights), checked against the CPU oracle."""
    import numpy as np
    from deepsignal_amd import synth, weights
    from oracle import oracle
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "11", "--warmup", "2",
                          "--dump-outputs", str(tmp_path)], env=env, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                         timeout=300)
    assert out.returncode == 0, out.stderr.decode()[-3000:]
    lines = [l for l in out.stdout.decode().splitlines() if l.startswith("{")]
    assert len(lines) == 1, out.stdout.decode()[-2000:]
    r = json.loads(lines[0])
    for key in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert key in r
    assert r["steps"] == 11 and r["windows"]["n"] == 1 and r["value"] > 1e5 and r["ms_per_step"] > 0
    assert not [k for k in FULL_ONLY if k in r]
    act, pred = np.load(os.path.join(str(tmp_path), "act.npy")), np.load(os.path.join(str(tmp_path), "pred.npy"))
    feats = synth.synthetic_features(8 * 512, seed=synth.FEATURE_SEED)
    b = (11 - 1) % 8 * 512
    o_act, o_pred = oracle.forward(weights.random_weights(seed=weights.WEIGHT_SEED), {k: v[b:b + 512] for k, v in feats.items()}, "f32")
    assert np.isfinite(act).all() and np.abs(act - o_act).max() <= 1e-5
    decided = np.abs(o_act[:, 1] - o_act[:, 0]) > 1e-3
    assert (pred[decided] == o_pred[decided]).all()


def test_committed_pmc_constants_resolve_for_the_kernels_the_line_quotes():
    """bench.py cannot read counters from inside the process: roofline.traffic, fc_path.mfma_busy_pmc and
    conv_path_hbm.traffic_per_step are constants of the latest profiles/rNN_pmc_*.json. A renamed kernel or file would
    silently turn them into null: the three lookups of the default line must resolve, name the file and the commit, and
    be consistent with the raw counter CSVs' summaries."""
    sys.path.insert(0, ROOT)
    import bench
    t = bench.pmc_traffic("lstm_cell_lds_kernel<1>")
    assert t["traffic"] and abs(t["traffic"] - t["traffic_fetch"] - t["traffic_write"]) <= 2
    assert "NOT measured in this run" in t["traffic_source"] and ("collected at commit" in t["traffic_source"] or "no build identity" in t["traffic_source"])
    assert 15e6 < t["traffic"] < 60e6                      # ~28 MB per BiLSTM diagonal at 512 sites
    f = bench.pmc_traffic("inception_fused_bf16_kernel<3>", "r[0-9][0-9]_bf16_all_4096_pmc_traffic.json")
    assert f["traffic"] and "bf16_all_4096_pmc_traffic.json" in f["traffic_source"]
    assert 3 * f["traffic"] < 992 * 564 * 4096             # the LDS chain moves fewer bytes than the module-granular figure
    m = bench.pmc_mfma_busy("gemm_kernel<1,3,4,1,0,2,2,1>")
    assert 0.5 < m["mfma_busy_pmc"] < 1.0 and "NOT measured in this run" in m["mfma_busy_source"]
