"""GPU: cascaded precision (ds_set_recheck; `call_mods --precision bf16_all --recheck_margin M`). A bf16_all forward on every
site, a device-side selection and compaction of the sites whose result falls within the margin of the threshold, an fp32-class
forward on just those, the two results merged.

Three engines of one max_batch per fine precision: coarse-only C (bf16_all), fine-only F, and the cascade K (a coarse and a
fine engine of its own). The selection is restated in numpy float32 (`_select`: the rule of include/deepsignal_hip.h,
operation by operation), and the claim is exact: K carries F's bits on the selected sites and C's bits on the others. That
rests on the property the project asserts elsewhere -- a site's bits do not depend on its batch mates -- because the fine
engine sees the selected sites alone, compacted.

Weights: `stress_weights` (a trained model's scale, both labels in every batch), as tests/test_gpu_stress.py.

The what-it-buys figures (Delta, share rechecked, label flips by margin; n = 512, stress weights) are printed (pytest -s) by
test_labels_equal_the_fine_engines_beyond_the_measured_distance and, where DS_RECORD_DIR names a directory, written to
recheck_parity.json in it; DESIGN.md section 9 quotes them.
"""
import json
import os

import numpy as np
import pytest

from deepsignal_amd import synth, weights as W
from deepsignal_amd.engine import Engine, ReadBatch, extract_reference

import extract_cases as xc

pytestmark = pytest.mark.gpu

KEYS = ("kmer", "means", "stds", "sanums", "signals")
FINE = ["fp32", "bf16x3"]
LABEL_MARGIN = 1e-3        # tests/test_gpu_stress.py


def _engine(w, precision, max_batch=512, **kw):
    e = Engine(device=0, max_batch=max_batch, precision=precision, **kw)
    e.load_weights(w)
    return e


def _run(e, f):
    return e.run(*(f[k] for k in KEYS))


def _select(act, margin):
    """include/deepsignal_hip.h, ds_set_recheck: float32, one rounding per operation."""
    act = np.asarray(act, np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        d = np.abs(act[:, 1] - act[:, 0])
        s = act[:, 0] + act[:, 1]
        return (d < np.float32(margin) * s) | ~np.isfinite(d) | ~np.isfinite(s)


def _pdiff(act):
    p = act / act.sum(axis=1, keepdims=True)
    return p[:, 1] - p[:, 0]


def _median_margin(act):
    """About half the sites fall below it, whatever the weights."""
    return float(np.float32(np.median(np.abs(_pdiff(act)))))


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _assert_merged(k, c, f, sel, nan_positions=False):
    """K == F on the selected sites, K == C on the others: act as raw bits, pred exactly."""
    (ka, kp), (ca, cp), (fa, fp) = k, c, f
    assert ka.shape == ca.shape == fa.shape and kp.shape == cp.shape
    assert np.array_equal(kp[sel], fp[sel]) and np.array_equal(kp[~sel], cp[~sel])
    assert np.array_equal(_bits(ka)[~sel], _bits(ca)[~sel])
    if nan_positions:
        assert xc.same_bits(np.ascontiguousarray(ka[sel]), np.ascontiguousarray(fa[sel]), nan_positions=True)
    else:
        assert np.array_equal(_bits(ka)[sel], _bits(fa)[sel])


class _Trio:
    def __init__(self, w, fine):
        self.w, self.fine = w, fine
        self.C, self.F = _engine(w, "bf16_all"), _engine(w, fine)
        self.K, self.Kf = _engine(w, "bf16_all"), _engine(w, fine)
        self._ref = {}

    def ref(self, n):
        """Features and the two plain engines' outputs for n sites: computed once, shared, never modified."""
        if n not in self._ref:
            f = synth.synthetic_features(n, seed=4100 + n)
            c, fo = _run(self.C, f), _run(self.F, f)
            for a in c + fo:
                a.setflags(write=False)
            self._ref[n] = (f, c, fo)
        return self._ref[n]

    def close(self):
        for e in (self.K, self.Kf, self.C, self.F):
            e.close()


@pytest.fixture(scope="module", params=FINE)
def trio(request, stress_weights):
    t = _Trio(stress_weights, request.param)
    yield t
    t.close()


# ---- 1. exact merge ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 63, 64, 130, 512])     # one lane, a partial wave, a wave, a wave border + a tail, several workgroups
def test_exact_merge(trio, n):
    f, c, fo = trio.ref(n)
    margin = _median_margin(c[0])
    sel = _select(c[0], margin)
    if n >= 2:
        assert 1 <= int(sel.sum()) <= n - 1, "vacuous: %d of %d selected" % (sel.sum(), n)
    trio.K.set_recheck(trio.Kf, margin)
    k = _run(trio.K, f)
    _assert_merged(k, c, fo, sel)
    m = int(sel.sum())
    assert trio.K.recheck_stats() == {"sites": n, "rechecked": m, "fine_forwards": (m + 511) // 512}


# ---- 2. ends ---------------------------------------------------------------------------------------------------------------
def test_ends_all_none_detached(trio):
    n = 130
    f, c, fo = trio.ref(n)
    trio.K.set_recheck(trio.Kf, 2.0)
    assert _select(c[0], 2.0).all()
    k = _run(trio.K, f)
    assert np.array_equal(_bits(k[0]), _bits(fo[0])) and np.array_equal(k[1], fo[1])
    assert trio.K.recheck_stats() == {"sites": n, "rechecked": n, "fine_forwards": 1}
    trio.K.set_recheck(trio.Kf, 1e-30)
    assert not _select(c[0], 1e-30).any()
    k = _run(trio.K, f)
    assert np.array_equal(_bits(k[0]), _bits(c[0])) and np.array_equal(k[1], c[1])
    assert trio.K.recheck_stats() == {"sites": n, "rechecked": 0, "fine_forwards": 0}
    trio.K.set_recheck(None, 0)
    k = _run(trio.K, f)
    assert np.array_equal(_bits(k[0]), _bits(c[0])) and np.array_equal(k[1], c[1])
    assert trio.K.recheck_stats()["sites"] == n          # nothing counted while detached
    trio.K.set_recheck(trio.Kf, 0.0)                      # margin <= 0 detaches as well
    assert trio.K._fine is None
    k = _run(trio.K, f)
    assert np.array_equal(_bits(k[0]), _bits(c[0]))


# ---- 3. chunking -----------------------------------------------------------------------------------------------------------
def test_fine_engine_with_a_smaller_max_batch_runs_in_chunks(trio):
    n = 300
    f = synth.synthetic_features(n, seed=4400)
    small = _engine(trio.w, trio.fine, max_batch=128)
    try:
        want = _run(small, f)                              # the fine-only engine loops 128 + 128 + 44 itself
        trio.K.set_recheck(small, 2.0)
        k = _run(trio.K, f)
        assert trio.K.recheck_stats() == {"sites": n, "rechecked": n, "fine_forwards": 3}
        assert np.array_equal(_bits(k[0]), _bits(want[0])) and np.array_equal(k[1], want[1])
    finally:
        trio.K.set_recheck(None, 0)
        small.close()


# ---- 4. non-finite results and the selection kernel on directed values -----------------------------------------------------
def test_non_finite_coarse_result_is_selected(trio):
    """NaN inputs of one site: where they reach the coarse act as NaN / inf the site is selected at any margin and takes the
    fine engine's result (NaN positions compared, payload not)."""
    n = 70
    f = {k: v.copy() for k, v in synth.synthetic_features(n, seed=4500).items()}
    f["means"][5, :] = np.nan
    f["signals"][66, :] = np.nan
    c, fo = _run(trio.C, f), _run(trio.F, f)
    sel = _select(c[0], 1e-30)
    print("non-finite coarse rows:", np.flatnonzero(~np.isfinite(c[0]).all(axis=1)).tolist())
    trio.K.set_recheck(trio.Kf, 1e-30)
    k = _run(trio.K, f)
    _assert_merged(k, c, fo, sel, nan_positions=True)
    assert trio.K.recheck_stats()["rechecked"] == int(sel.sum())
    for i in np.flatnonzero(~np.isfinite(c[0]).all(axis=1)):
        assert sel[i]


@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 130, 256, 257, 512])
def test_selection_kernel_on_directed_values(trio, n):
    """ds_recheck_select: the kernel's selection for act rows given by the test -- every special, ties at the margin's edge,
    dense / sparse / empty / full patterns -- equals the numpy rule, indices ascending."""
    rng = np.random.default_rng(n)
    act = rng.random((n, 2), dtype=np.float32)
    specials = [(np.nan, 0.5), (0.5, np.nan), (np.inf, 0.5), (0.5, np.inf), (-np.inf, 0.5), (np.inf, -np.inf), (np.inf, np.inf),
                (0.0, 0.0), (0.5, 0.5), (1.0, 0.0), (3e38, 3e38), (-3e38, 3e38), (0.55, 0.45), (0.45, 0.55)]
    for j, v in enumerate(specials):
        if n > 2:
            act[(j * 37 + 3) % n] = v
    for margin in (0.1, 0.5, 2.0, 1e-30, float(np.float32(0.1))):
        sel = _select(act, margin)
        got = trio.C.recheck_select(act, margin)
        assert np.array_equal(got, np.flatnonzero(sel).astype(np.int32)), (n, margin)
    if n > 2:
        assert _select(act, 1e-30).any() and not _select(act, 1e-30).all()
    # a dense block, then nothing, then one lane per wave
    act[:] = (0.9, 0.1)
    act[: n // 3] = (0.5, 0.5)
    act[::64] = (0.5, 0.5)
    assert np.array_equal(trio.C.recheck_select(act, 0.1), np.flatnonzero(_select(act, 0.1)).astype(np.int32))


# ---- 5. every route --------------------------------------------------------------------------------------------------------
def test_submit_wait_with_the_pipeline_full(trio):
    """slots + 1 tickets, every slot in flight, waited in order: each ticket is complete (rechecks merged) when its wait returns."""
    n = 130
    f0, c0, _ = trio.ref(n)
    margin = _median_margin(c0[0])
    K = trio.K
    K.set_recheck(trio.Kf, margin)
    batches = [{k: np.ascontiguousarray(np.roll(f0[k], 7 * j, axis=0)) for k in KEYS} for j in range(K.slots + 1)]
    refs = [(_run(trio.C, b), _run(trio.F, b)) for b in batches]
    tickets = [K.submit(*(b[k] for k in KEYS)) for b in batches[:K.slots]]
    got = [K.wait(tickets[0])]
    tickets.append(K.submit(*(batches[-1][k] for k in KEYS)))
    got += [K.wait(t) for t in tickets[1:]]
    total = 0
    for (c, fo), k in zip(refs, got):
        sel = _select(c[0], margin)
        assert 1 <= int(sel.sum()) <= n - 1
        _assert_merged(k, c, fo, sel)
        total += int(sel.sum())
    assert K.recheck_stats()["sites"] == n * (K.slots + 1) and K.recheck_stats()["rechecked"] == total


def test_submit_parts_and_run(trio):
    n = 130
    f, c, fo = trio.ref(n)
    margin = _median_margin(c[0])
    sel = _select(c[0], margin)
    trio.K.set_recheck(trio.Kf, margin)
    parts = [tuple(np.array(f[k][s:e]) for k in KEYS) for s, e in ((0, 50), (50, n))]       # two segments, separate buffers
    _assert_merged(trio.K.wait(trio.K.submit_parts(parts)), c, fo, sel)
    _assert_merged(_run(trio.K, f), c, fo, sel)


def test_submit_reads(trio):
    """The GPU extraction route: the features are already in the slot's device buffers when the selection runs."""
    reads, sr, sl, norm, _, _, seed = xc.BY_NAME["block_growth"].steps("mad")[0]
    b = ReadBatch(reads, sr, sl, norm=norm, seed=seed)
    f = extract_reference(b)
    c, fo = _run(trio.C, f), _run(trio.F, f)
    margin = _median_margin(c[0])
    sel = _select(c[0], margin)
    assert 1 <= int(sel.sum()) <= b.nsites - 1
    trio.K.set_recheck(trio.Kf, margin)
    _assert_merged(trio.K.wait(trio.K.submit_reads(b)), c, fo, sel)


def test_forward_device_is_refused_while_attached(trio):
    trio.K.set_recheck(trio.Kf, 0.1)
    with pytest.raises(RuntimeError, match="recheck attached"):
        trio.K.run_device(1, 0, 0, 0, 0, 0, 0, 0)


# ---- 6. invalid attachments ------------------------------------------------------------------------------------------------
def test_invalid_attachments(trio):
    K, Kf, C = trio.K, trio.Kf, trio.C
    K.set_recheck(Kf, 0.1)
    other = Engine(device=0, max_batch=32, kmer_len=9, signal_len=100)
    three = [Engine(device=0, max_batch=32, class_num=3, precision=p) for p in ("bf16_all", "fp32")]
    try:
        with pytest.raises(RuntimeError, match=r"\(-1\).*kmer_len differs"):
            C.set_recheck(other, 0.1)
        with pytest.raises(RuntimeError, match=r"\(-1\).*coarse handle itself"):
            C.set_recheck(C, 0.1)
        with pytest.raises(RuntimeError, match=r"\(-1\).*recheck attached itself"):
            C.set_recheck(K, 0.1)
        with pytest.raises(RuntimeError, match=r"\(-4\).*class_num 3"):
            three[0].set_recheck(three[1], 0.1)
        with pytest.raises(RuntimeError, match=r"\(-1\).*NaN"):
            C.set_recheck(trio.F, float("nan"))
        assert C._fine is None and K._fine is Kf
        f, c, _ = trio.ref(63)
        k = _run(C, f)                                     # the refused calls left C as it was
        assert np.array_equal(_bits(k[0]), _bits(c[0]))
    finally:
        other.close()
        for e in three:
            e.close()


# ---- 7. what it buys -------------------------------------------------------------------------------------------------------
def test_labels_equal_the_fine_engines_beyond_the_measured_distance(trio):
    """Delta = the largest distance of the coarse engine's p1 - p0 from the fine engine's, measured on the two plain engines.
    A site the cascade does not recheck at margin 1.25 Delta has |p1 - p0|_C >= 1.25 Delta, so the fine engine's p1 - p0 has
    the same sign: the cascade's labels equal the fine engine's wherever that one is decided (LABEL_MARGIN)."""
    n = 512
    f, c, fo = trio.ref(n)
    dc, df = _pdiff(c[0]), _pdiff(fo[0])
    delta = float(np.abs(dc - df).max())
    decided = np.abs(df) > LABEL_MARGIN
    share1 = float(fo[1].mean())
    assert 0.2 <= share1 <= 0.8, "label check would be vacuous: label-1 share %.3f" % share1
    trio.K.set_recheck(trio.Kf, 1.25 * delta)
    k = _run(trio.K, f)
    st = trio.K.recheck_stats()
    rec = {"n": n, "fine": trio.fine, "delta": delta, "margin": 1.25 * delta, "share_rechecked": st["rechecked"] / n,
           "flips_coarse_alone": int((c[1][decided] != fo[1][decided]).sum()), "decided": int(decided.sum()),
           "flips_cascade_at_1.25_delta": int((k[1][decided] != fo[1][decided]).sum()), "flips_by_margin": {}, "share_by_margin": {}}
    for m in (0.0, 0.05, 0.1, 0.2, 0.4):
        trio.K.set_recheck(trio.Kf if m > 0 else None, m)
        km = _run(trio.K, f)
        rec["flips_by_margin"]["%g" % m] = int((km[1][decided] != fo[1][decided]).sum())
        rec["share_by_margin"]["%g" % m] = (trio.K.recheck_stats()["rechecked"] / n) if m > 0 else 0.0
    print("recheck parity:", json.dumps(rec, sort_keys=True))
    if os.environ.get("DS_RECORD_DIR"):                    # a directory for the measured figures, beside the printed line
        path = os.path.join(os.environ["DS_RECORD_DIR"], "recheck_parity.json")
        try:
            os.makedirs(os.path.dirname(path), exist_ok=True)
            old = json.load(open(path)) if os.path.exists(path) else {}
            old[trio.fine] = rec
            json.dump(old, open(path, "w"), indent=1, sort_keys=True)
        except OSError:
            pass
    assert (k[1][decided] == fo[1][decided]).all()


# ---- 8. the command line ---------------------------------------------------------------------------------------------------
def _write_feature_tsv(path, feats, reads):
    from deepsignal_amd.utils.process_utils import code2base_dna
    with open(path, "w") as f:
        for i in range(len(reads)):
            kmer = "".join(code2base_dna[int(c)] for c in feats["kmer"][i])
            cols = ["chr%d" % (1 + i % 5), str(100 + i), "+-"[i % 2], str(9000 - i), reads[i], "tc"[i % 2], kmer,
                    ",".join("%s" % np.float32(x) for x in feats["means"][i]),
                    ",".join("%s" % np.float32(x) for x in feats["stds"][i]),
                    ",".join(str(int(x)) for x in feats["sanums"][i]),
                    ",".join("%s" % np.float32(x) for x in feats["signals"][i]),
                    str(int(feats["labels"][i]))]
            f.write("\t".join(cols) + "\n")


@pytest.fixture(scope="module")
def cli_files(stress_weights, tmp_path_factory):
    d = tmp_path_factory.mktemp("recheck_cli")
    n = 600
    feats = synth.synthetic_features(n, seed=4800)
    tsv, dsw = str(d / "features.tsv"), str(d / "model.dsw")
    _write_feature_tsv(tsv, feats, ["read_%04d" % (i // 20) for i in range(n)])
    W.save_weights(dsw, stress_weights)
    return d, tsv, dsw, n


def _cli(cli_files, tag, extra):
    from deepsignal_amd.deepsignal import main
    d, tsv, dsw, _ = cli_files
    out = str(d / (tag + ".tsv"))
    assert main(["call_mods", "-i", tsv, "-m", dsw, "-o", out, "--engine_batch", "512"] + extra) == 0
    return open(out, "rb").read()


@pytest.mark.parametrize("fine", FINE)
def test_cli_margin_2_gives_the_fine_precisions_rows(cli_files, capsys, fine):
    n = cli_files[3]
    want = _cli(cli_files, "plain_" + fine, ["--precision", fine])
    capsys.readouterr()
    got = _cli(cli_files, "cascade_" + fine, ["--precision", "bf16_all", "--recheck_margin", "2.0", "--recheck_precision", fine])
    out = capsys.readouterr().out
    assert got == want and got.count(b"\n") == n
    assert "recheck: %d sites, %d rechecked in %s (margin 2), share 1.0000" % (n, n, fine) in out


def test_cli_margin_0_is_the_plain_bf16_run(cli_files, capsys):
    want = _cli(cli_files, "bf16_all", ["--precision", "bf16_all"])
    capsys.readouterr()
    got = _cli(cli_files, "bf16_all_m0", ["--precision", "bf16_all", "--recheck_margin", "0"])
    assert got == want and got.count(b"\n") == cli_files[3]
    out = capsys.readouterr().out                          # the parameter dump names the two flags; no summary line is printed
    assert not [l for l in out.splitlines() if l.startswith("recheck") and "sites" in l]
