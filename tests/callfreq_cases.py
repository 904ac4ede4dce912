"""Shared by the `call_mods --freq_file` tests (CPU and GPU): act rows whose normalised probabilities are chosen float32 values,
what Python reads from the text call_mods prints for them, synthetic result-row batches in the arguments of fastio.format_rows,
and the CPU checker ds_freq_values_reference put behind the interface FreqStream drives."""
import struct

import numpy as np

from deepsignal_amd import call_modification_frequency as cmf
from deepsignal_amd import engine as eng
from deepsignal_amd import fastio

OK, HOST = eng.TEXT_ROW_OK, eng.TEXT_ROW_HOST
LOW = np.float32(1e-14)                # every finite q in [LOW, 1] is the device's: nine digits at >= 1e-14 need <= 22 decimal places


def normalised(act):
    """q0, q1 as ds_format_rows computes them: float32, operation by operation."""
    act = np.asarray(act, np.float32)
    with np.errstate(all="ignore"):
        s = act[:, 0] + act[:, 1]
        return act[:, 0] / s, act[:, 1] / s


def python_value(q) -> float:
    """What call_freq reads from the text call_mods prints for the float32 q."""
    return float(str(np.float32(q)))


def bits(x: float) -> bytes:
    return struct.pack("<d", x)


def act_for(q):
    """act rows (q, 1 - q): 1 - q rounds by at most 2^-25, so the float32 sum is exactly 1 and q0 is exactly q, q1 exactly
    float32(1 - q)."""
    q = np.asarray(q, np.float32)
    act = np.stack([q, (1.0 - q.astype(np.float64)).astype(np.float32)], axis=1)
    assert (act[:, 0] + act[:, 1] == np.float32(1)).all()
    return act


def _neighbours(x):
    x = np.float32(x)
    return [np.nextafter(x, np.float32(0)), x, np.nextafter(x, np.float32(2))]


def edge_q():
    """The float32 values in [1e-14, 1] where a shortest-digits routine goes wrong first: both neighbours of every power of two and
    of ten (and the powers), 0.5 and 1e-4 (the positional / scientific switch of the printed form) with theirs, 1.0, a value half
    way between two eight-digit decimals, and exact binary fractions of one to eight digits."""
    q = []
    for k in range(-46, 1):
        q += _neighbours(np.ldexp(np.float32(1), k))
    for k in range(-14, 1):
        q += _neighbours(np.float32(10.0 ** k))
    q += _neighbours(0.5) + _neighbours(1e-4) + [np.float32(1.0), np.float32(87.0 / 512.0)]
    q += [np.ldexp(np.float32(1), -k) for k in range(1, 9)]           # 0.5, 0.25, ... 0.00390625: 1 .. 8 digits
    q = np.array(q, np.float32)
    return q[(q >= LOW) & (q <= 1)]


def random_q(n, seed):
    """Uniformly random BIT PATTERNS between 1e-14 and 1: every exponent as likely as any other."""
    lo, hi = int(LOW.view(np.uint32)), int(np.float32(1).view(np.uint32))
    rng = np.random.default_rng(seed)
    return rng.integers(lo, hi + 1, n, dtype=np.uint32).view(np.float32)


def digits_of(q) -> int:
    """Significant digits of the printed form."""
    t = str(np.float32(q)).split("e")[0].replace(".", "").lstrip("0").rstrip("0")
    return max(1, len(t))


def outside_act():
    """act rows whose q lies outside [1e-14, 1]: subnormal, tiny, zero sum (NaN), a zero denominator (inf), negative, above one."""
    tiny = [np.float32(1e-45), np.float32(1e-39), np.float32(1e-30), np.float32(9.9e-15), np.float32(2.7581529e-17), np.float32(1e-22),
            np.float32(1.5e-23)]
    rows = [(t, np.float32(1)) for t in tiny]
    rows += [(0.0, 0.0), (1.0, -1.0), (np.inf, 1.0), (np.nan, 0.5), (-0.25, 1.0), (3.0, -1.0), (0.0, 1.0), (-0.0, 1.0), (1.0, 0.0)]
    return np.array(rows, np.float32)


def assert_values(act, p0, p1, status, must_be_ok=None):
    """The contract of call_value against Python, row by row: a row whose two q are 0 or in [1e-14, 1] is ROW_OK; a ROW_OK row holds
    Python's doubles bit for bit; any other row may only be ROW_HOST."""
    q0, q1 = normalised(act)
    inside = lambda q: np.isfinite(q) & ((q == 0) | ((q >= LOW) & (q <= 1)))
    need = inside(q0) & inside(q1)
    if must_be_ok is not None:
        assert need.all() == must_be_ok
    wrong = []
    for i in range(len(act)):
        if status[i] == OK:
            if bits(float(p0[i])) != bits(python_value(q0[i])) or bits(float(p1[i])) != bits(python_value(q1[i])):
                wrong.append((i, float(q0[i]), float(q1[i]), float(p0[i]), float(p1[i])))
        else:
            assert status[i] == HOST
            if need[i]:
                wrong.append((i, float(q0[i]), float(q1[i]), "ROW_HOST"))
    assert not wrong, wrong[:10]


# ---- result rows as call_mods has them ---------------------------------------------------------------------------------------
def make_batch(infos, act, pred, kmer):
    """The arguments of fastio.format_rows for rows with these sampleinfo strings (str, or bytes as they are)."""
    enc = [s if isinstance(s, bytes) else s.encode("utf-8") for s in infos]
    off = np.zeros(len(enc) + 1, np.int64)
    off[1:] = np.cumsum([len(b) for b in enc])
    return (np.frombuffer(b"".join(enc), np.uint8), off, np.ascontiguousarray(act, np.float32), np.ascontiguousarray(pred, np.int32),
            np.ascontiguousarray(kmer, np.int32))


def random_rows(seed, nrows, nsites, nchrom=3, kmer_len=17):
    """nrows rows scattered over nsites sites: sampleinfo strings, act rows (sigmoid-like pairs, now and then a nearly undecided or
    a saturated one), pred, k-mer codes."""
    rng = np.random.default_rng(seed)
    sites = []
    while len(sites) < nsites:
        s = ("chr%d" % rng.integers(1, nchrom + 1), int(rng.integers(0, 100000)))
        if s not in sites:
            sites.append(s)
    pick = rng.integers(0, nsites, nrows)
    pick[:min(nrows, nsites)] = rng.permutation(nsites)[:min(nrows, nsites)]      # every site at least once when there is room
    infos = ["%s\t%d\t%s\t%d\tread%d\tt" % (sites[k][0], sites[k][1], "+-"[k % 2], 9000 + k, r) for r, k in enumerate(pick.tolist())]
    logit = rng.normal(0, 3, nrows)
    a1 = 1 / (1 + np.exp(-logit))
    a0 = 1 / (1 + np.exp(logit + rng.normal(0, 0.3, nrows)))
    sat = rng.random(nrows) < 0.05
    a0[sat] = 10.0 ** -rng.uniform(5, 12, int(sat.sum()))
    act = np.stack([a0, a1], axis=1).astype(np.float32)
    pred = (act[:, 1] > act[:, 0]).astype(np.int32)
    kmer = rng.integers(0, 4, (nrows, kmer_len)).astype(np.int32)
    return infos, act, pred, kmer


def text_of(batches) -> bytes:
    """The result file call_mods writes for these batches."""
    return b"".join(fastio.format_rows(*b) for b in batches)


def cpu_table(tmp_path, batches, prob_cf=0.0, sort=False, bed=False, name="calls.tsv"):
    """calculate_mods_frequency on the text of the batches -> (stats, the table's bytes)."""
    calls, out = str(tmp_path / name), str(tmp_path / (name + ".freq"))
    with open(calls, "wb") as f:
        f.write(text_of(batches))
    stats = cmf.calculate_mods_frequency([calls], prob_cf)
    cmf.write_sitekey2stats(stats, out, sort, bed)
    return stats, open(out, "rb").read()


def stream_table(tmp_path, batches, prob_cf=0.0, sort=False, bed=False, name="stream.freq", **kw):
    """The same batches through FreqStream -> (stats, the table's bytes, the stream's info)."""
    out = str(tmp_path / name)
    st = cmf.FreqStream(prob_cf, **kw)
    try:
        for b in batches:
            st.push(*b)
        stats = st.finish()
    finally:
        st.close()
    cmf.write_sitekey2stats(stats, out, sort, bed)
    return stats, open(out, "rb").read(), st.info


class StreamReferenceBackend:
    """freq_begin_stream .. freq_end of Engine without a GPU: the values by ds_freq_values_reference (the routine freq_values_kernel
    runs), the aggregation by a plain dict in row order."""

    def __init__(self):
        self.sites = {}            # key -> [first_row, sum0, sum1, met, unmet]
        self.rows = self.used = 0
        self.pending = None

    def freq_begin_stream(self, initial_slots, batch_rows, prob_cf=0.0):
        self.batch, self.cf = batch_rows, prob_cf

    def freq_push(self, chrom, pos, act, pred):
        assert self.pending is None and 1 <= len(pred) <= self.batch
        chrom, pos = np.array(chrom, np.int32), np.array(pos, np.int64)
        p0, p1, status = eng.freq_values_reference(act)
        status[(chrom < 0) | (chrom >= eng.FREQ_CHROM_LIMIT) | (pos < 0) | (pos >= eng.FREQ_POS_LIMIT)] = HOST
        self.pending = [chrom, pos, p0, p1, (np.asarray(pred) == 1).astype(np.int32), status]
        return status.copy()

    def freq_accumulate(self, rows=(), chrom=(), pos=(), p0=(), p1=(), met=()):
        c, q, a, b, m, status = self.pending
        self.pending = None
        for r, cc, qq, aa, bb, mm in zip(rows, chrom, pos, p0, p1, met):
            assert status[r] == HOST
            c[r], q[r], a[r], b[r], m[r], status[r] = cc, qq, aa, bb, mm, OK
        assert (status == OK).all(), "a host row got no values"
        opened = np.zeros(len(c), np.int32)
        for i in range(len(c)):
            if abs(float(a[i]) - float(b[i])) < self.cf:
                continue
            key = (int(c[i]), int(q[i]))
            site = self.sites.get(key)
            if site is None:
                site = self.sites[key] = [self.rows + i, 0.0, 0.0, 0, 0]
                opened[i] = 1
            site[1] += float(a[i])
            site[2] += float(b[i])
            site[3 if m[i] else 4] += 1
            self.used += 1
        self.rows += len(c)
        return opened

    def freq_result(self):
        keys = list(self.sites)
        col = lambda j, dt: np.array([self.sites[k][j] for k in keys], dt)
        return {"first_row": col(0, np.int64), "chrom": np.array([k[0] for k in keys], np.int32), "pos": np.array([k[1] for k in keys], np.int64),
                "sum0": col(1, np.float64), "sum1": col(2, np.float64), "met": col(3, np.int32), "unmet": col(4, np.int32),
                "rows": self.rows, "used": self.used}

    def freq_times(self, reset=False):
        return {}

    def freq_end(self):
        pass

    def close(self):
        pass
