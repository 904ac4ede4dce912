"""GPU: feature rows formatted on the device (ds_submit_rows / ds_wait_rows / ds_extract_rows, ds_format_values) against the CPU
statement of the same code (ds_extract_rows_reference, held to the host extractor by tests/test_extract_rows_reference.py), and
`extract --extract_on gpu` against `extract --extract_on cpu`."""
import collections
import os

import numpy as np
import pytest

from deepsignal_amd import extract_features as ef
from deepsignal_amd import synth, weights
from deepsignal_amd.engine import Engine, ReadBatch, base_codes, extract_rows_reference, format_values, pack_info

import extract_cases as xc
import rows_cases as rc

pytestmark = pytest.mark.gpu

FAST5 = os.path.join(os.path.dirname(__file__), "golden", "fast5")


@pytest.fixture(scope="module")
def geometry_engines():
    """One engine per geometry, never given weights: consecutive cases share slot 0 and the row buffers the case before left."""
    engines = {}
    yield lambda T, S: engines.setdefault((T, S), Engine(kmer_len=T, signal_len=S, device=0, max_batch=512))
    for e in engines.values():
        e.close()


def test_format_values_on_the_device_matches_the_host_code(geometry_engines):
    values = rc.directed_values()
    e = geometry_engines(17, 360)
    got, want = format_values(values, engine=e), format_values(values)
    assert got == want and want.count(b",") == len(values) - 1
    assert format_values([1.2e-5, -0.0, np.nan, -np.inf, 2.0], engine=e) == b"1.2e-05,-0.0,nan,-inf,2.0"
    with pytest.raises(RuntimeError, match="31 bytes needed"):
        format_values([2.0] * 8, engine=e, cap=30)


def _info(step):
    """Leading columns of a step's rows: what the host extractor writes for them, without running its numeric part."""
    reads, site_read, site_loc, norm, T, S, seed = step
    rows = ["\t".join(["chr%d" % (rd % 3), str(1000 * rd + loc), "+", "-1", "r%d" % rd, "t"]).encode()
            for rd, loc in zip(site_read.tolist(), site_loc.tolist())]
    return (ReadBatch(reads, site_read, site_loc, norm=norm, seed=seed),) + pack_info(rows)


@pytest.mark.parametrize("name,norm", xc.case_norm_params())
def test_case_table_rows_match_reference(geometry_engines, name, norm):
    """Engine.extract_rows == extract_rows_reference byte for byte (SUB rows included: both use the same hash), offsets too, on
    every step of every case in the case's order on one slot."""
    case = xc.BY_NAME[name]
    e = geometry_engines(*case.geometry)
    for i, step in enumerate(case.steps(norm)):
        batch, info, info_off = _info(step)
        got, got_off = e.extract_rows(batch, info, info_off, rc.LABEL)
        want, want_off = extract_rows_reference(batch, info, info_off, rc.LABEL, *case.geometry)
        assert np.array_equal(got_off, want_off), i
        assert got == want, i
        rc.split_rows(got, got_off)


def _small_batches(n):
    out = []
    for i in range(n):
        raw, starts, lengths, bases, scaling, offset = synth.synthetic_read(300 + 70 * i, 40 + i, long_bases=i % 2)
        codes = base_codes(bases)
        locs = [loc for loc in range(8, len(codes) - 8) if codes[loc] == 1 and codes[loc + 1] == 2][:20 + 7 * i]
        rows = [("chrX\t%d\t-\t%d\tread%d\tt" % (loc, 5 * loc, i)).encode() for loc in locs]
        out.append((ReadBatch([(raw, starts, lengths, codes, scaling, offset, 500 + i)], [0] * len(locs), locs,
                              norm=("mad", "zscore")[i % 2], seed=3),) + pack_info(rows) + (i % 2,))
    return out


def test_rows_pipeline_beside_forwards():
    """slots + 1 submit_rows of different small batches, waited in order: each equals its blocking counterpart and the checker.
    A forward submitted between them returns the act it returns without the rows traffic; a rows ticket is no forward ticket,
    and a short buffer consumes nothing."""
    e = Engine(device=0, max_batch=512, slots=3)
    try:
        e.load_weights(weights.random_weights(seed=3, lstm_bias_std=0.1))
        batches = _small_batches(e.slots + 1)
        fwd = batches[1][0]
        act0, pred0 = e.wait(e.submit_reads(fwd))
        blocking = [e.extract_rows(b, info, off, label) for b, info, off, label in batches]
        t0 = e.submit_rows(*batches[0])
        t1 = e.submit_rows(*batches[1])
        tf = e.submit_reads(fwd)
        with pytest.raises(RuntimeError, match="ds_wait"):
            e.wait(t0)
        need = e._lib.ds_wait_rows(e._h, t0[0], np.empty(8, np.uint8).ctypes.data, 8, None)
        assert need == -len(blocking[0][0])
        got = [e.wait_rows(t0), e.wait_rows(t1)]
        act, pred = e.wait(tf)
        assert np.array_equal(act.view(np.uint32), act0.view(np.uint32)) and np.array_equal(pred, pred0)
        tickets = collections.deque()
        for b in batches[2:] + batches[:1]:         # wraps over every slot once more
            tickets.append(e.submit_rows(*b))
        got += [e.wait_rows(t) for t in tickets]
        for (text, off), k in zip(got, [0, 1] + list(range(2, len(batches))) + [0]):
            b, info, info_off, label = batches[k]
            assert text == blocking[k][0] and np.array_equal(off, blocking[k][1])
            want, want_off = extract_rows_reference(b, info, info_off, label)
            assert text == want and np.array_equal(off, want_off)
            assert text.endswith(("\t%d\n" % label).encode())
        with pytest.raises(RuntimeError, match="ds_wait_rows"):
            e.wait_rows(t0)
    finally:
        e.close()


def test_invalid_rows_calls_are_refused(geometry_engines):
    e = geometry_engines(17, 360)
    b, info, off, label = _small_batches(1)[0]
    with pytest.raises(RuntimeError, match="info_off"):
        e.extract_rows(b, info, off[::-1].copy(), label)
    big = ReadBatch([(b.raw, b.start, b.length, b.base, 1.0, 0.0)], [0] * 513, [20] * 513)
    with pytest.raises(RuntimeError, match="nsites"):
        e.extract_rows(big, np.zeros(0, np.uint8), np.zeros(514, np.int64), label)


# ---- the command: extract --extract_on gpu == extract --extract_on cpu ---------------------------------------------------------
def _extract(tmp, style, norm, where, nproc=1, extra=(), name=None):
    from deepsignal_amd import deepsignal as cli
    out = str(tmp / (name or "%s_%s_%s_%d" % (style, norm, where, nproc)))
    rc_ = cli.main(["extract", "-i", os.path.join(FAST5, style), "-o", out, "--normalize_method", norm, "--f5_batch_num", "2",
                    "--nproc", str(nproc), "--extract_on", where, "--engine_batch", "64"] + list(extra))
    assert rc_ in (0, None)
    return out


def _sub_sites(style):
    """Sites of the fixture whose middle base alone holds >= 360 samples (the one documented difference), and the site count."""
    sub, n = set(), 0
    for fp in ef.get_fast5s(os.path.join(FAST5, style)):
        _, _, lengths, bases, _, _, info = ef._read_fast5(fp, "RawGenomeCorrected_000", "BaseCalled_template")
        for loc, pos, _ in ef.read_sites(bases, ["CG"], 0, 17, info[2], info[3], info[4], None):
            n += 1
            if lengths[loc] >= 360:
                sub.add((info[3], str(pos), info[2], info[0]))
    return sub, n


def _assert_same_rows(cpu_file, gpu_file, sub):
    a, b = open(cpu_file, "rb").read(), open(gpu_file, "rb").read()
    if not sub:
        assert a == b and a.count(b"\n") > 0
        return
    la, lb = a.decode().splitlines(), b.decode().splitlines()
    assert len(la) == len(lb) > 0
    for x, y in zip(la, lb):
        cx, cy = x.split("\t"), y.split("\t")
        if (cx[0], cx[1], cx[2], cx[4]) in sub:
            assert cx[:10] + cx[11:] == cy[:10] + cy[11:]
        else:
            assert x == y


_CPU_RUNS = {}


@pytest.fixture(scope="module")
def cpu_run(tmp_path_factory):
    """The host route's TSV of a fixture directory (one process: file batches in order), made once per (style, norm)."""
    tmp = tmp_path_factory.mktemp("extract_cpu")

    def get(style, norm):
        if (style, norm) not in _CPU_RUNS:
            _CPU_RUNS[(style, norm)] = (_extract(tmp, style, norm, "cpu"), _sub_sites(style))
        return _CPU_RUNS[(style, norm)]
    return get


@pytest.mark.parametrize("nproc", [1, 3])
@pytest.mark.parametrize("norm", ["mad", "zscore"])
@pytest.mark.parametrize("style", ["plain", "ont", "latest"])
def test_extract_on_gpu_writes_the_cpu_routes_tsv(tmp_path, cpu_run, style, norm, nproc):
    cpu_file, (sub, nsites) = cpu_run(style, norm)
    assert len(sub) <= 0.05 * nsites
    gpu_file = _extract(tmp_path, style, norm, "gpu", nproc)
    _assert_same_rows(cpu_file, gpu_file, sub)
    assert open(gpu_file, "rb").read().count(b"\n") == nsites


def test_extract_on_gpu_directory_output_and_positions(tmp_path):
    sub, nsites = _sub_sites("plain")
    dirs = {w: _extract(tmp_path, "plain", "mad", w, 1, ["--w_is_dir", "yes", "--w_batch_num", "1"], name="dir_" + w)
            for w in ("cpu", "gpu")}
    names = sorted(os.listdir(dirs["cpu"]))
    assert names == sorted(os.listdir(dirs["gpu"])) == ["0.tsv", "1.tsv", "2.tsv"]      # 5 files in batches of 2
    for n in names:
        _assert_same_rows(os.path.join(dirs["cpu"], n), os.path.join(dirs["gpu"], n), sub)
    rows = [r.split("\t") for n in names for r in open(os.path.join(dirs["cpu"], n)).read().splitlines()]
    picked = [rows[1], rows[-2]]
    pos = tmp_path / "positions.tsv"
    pos.write_text("".join("%s\t%s\t%s\n" % (r[0], r[1], r[2]) for r in picked))
    files = {w: _extract(tmp_path, "plain", "mad", w, 1, ["--positions", str(pos), "--methy_label", "0"], name="pos_" + w)
             for w in ("cpu", "gpu")}
    _assert_same_rows(files["cpu"], files["gpu"], sub)
    got = open(files["gpu"]).read().splitlines()
    assert len(got) >= 2 and all(r.endswith("\t0") for r in got)
    assert {tuple(r.split("\t")[:3]) for r in got} == {tuple(r[:3]) for r in picked}


def test_call_mods_reads_the_gpu_tsv(tmp_path, cpu_run):
    """call_mods -i <tsv> calls the GPU-extracted TSV as it calls the host-extracted one."""
    from deepsignal_amd import deepsignal as cli
    cpu_file, (sub, _) = cpu_run("ont", "mad")
    gpu_file = _extract(tmp_path, "ont", "mad", "gpu", 1)
    wfile = str(tmp_path / "model.dsw")
    weights.save_weights(wfile, weights.random_weights(seed=3, lstm_bias_std=0.1))
    outs = []
    for tsv in (cpu_file, gpu_file):
        outs.append(str(tmp_path / (os.path.basename(tsv) + ".calls")))
        assert cli.main(["call_mods", "-i", tsv, "-m", wfile, "-o", outs[-1], "--batch_size", "16", "--engine_batch", "64",
                         "--is_gpu", "yes"]) in (0, None)
    a, b = open(outs[0]).read().splitlines(), open(outs[1]).read().splitlines()
    assert len(a) == len(b) > 0
    for x, y in zip(a, b):
        cx = x.split("\t")
        assert x == y or ((cx[0], cx[1], cx[2], cx[4]) in sub and cx[:6] == y.split("\t")[:6])
