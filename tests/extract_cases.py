"""The inputs of the feature-extraction tests: one table of named, seeded cases, shared by tests/test_extract_reference.py (CPU:
ds_extract_reference == the numpy host extractor) and tests/test_gpu_extract.py (GPU: the kernels == ds_extract_reference), so
the checker is proven against numpy on exactly the inputs it then judges the kernels on.

A case is a sequence of steps (almost always one); a step is the argument list of a ReadBatch plus the geometry:
(reads, site_read, site_loc, norm, kmer_len, signal_len, seed). Steps of one case run in their order on one engine slot.
Every case names the code paths of csrc/ds_extract.hip it is there for; `derive_paths` computes, from a step's arrays alone,
the paths those arrays take, and the CPU suite requires the union over the table to be ALL_PATHS.

Base codes are drawn from A / G / T with a C, G pair written at every site, so the host extractor's motif scan for "CG" finds
exactly the case's sites."""
import functools

import numpy as np

from deepsignal_amd import synth

NP_BLOCK = 8192        # numpy's reduction block (ds_extract.h NP_BLOCK)
WG_BLOCKS = 16         # numpy blocks per pass of wg_np_sum: STATS_THREADS / 64
NP_LEAF = 128          # leaf of numpy's pairwise sum
CDF_LDS = 8192         # histogram bins kept in LDS
SCAN_CHUNK = 1024      # bins per pass of the workgroup scan (STATS_THREADS)
GEOMETRIES = ((17, 360), (9, 100))
SCALING, OFFSET = 1400.0 / 8192.0 * 1.003, 12.0

WINDOW_PATHS = ("pad", "pad_total=S-1", "split_unclamped", "split_left_clamp", "split_right_clamp", "split_total=S",
                "split_mid=S-1", "sub", "sub_mid=S")
ALL_PATHS = frozenset(
    ["z:passes=%s" % p for p in ("0", "1", "2", "3+")] + ["z:tail=%s" % t for t in ("none", "lt8", "leaf", "leaves")] +
    ["mad:hist=lds", "mad:hist=global", "mad:chunks=1", "mad:chunks=2", "mad:chunks=3+", "mad:n=odd", "mad:n=even"] +
    ["win%d:%s" % (t, w) for t, _ in GEOMETRIES for w in WINDOW_PATHS] +
    ["base:%s" % b for b in ("1", "lt8", "8", "leaf", "128", "leaves", "blocks")] + ["read:empty"])


# ---- the paths a step takes, from its inputs alone ----------------------------------------------------------------------
def _window_paths(lens, S):
    T, total, mid = len(lens), int(sum(lens)), (len(lens) - 1) // 2
    if total < S:
        return {"pad"} | ({"pad_total=S-1"} if total == S - 1 else set())
    if lens[mid] >= S:
        return {"sub"} | ({"sub_mid=S"} if lens[mid] == S else set())
    left = int(sum(lens[:mid]))
    right = total - left
    left_len = (S - int(lens[mid])) // 2
    right_len = S - left_len
    out = {"split_left_clamp" if left_len > left else "split_right_clamp" if right_len > right else "split_unclamped"}
    if total == S:
        out.add("split_total=S")
    if lens[mid] == S - 1:
        out.add("split_mid=S-1")
    return out


def _base_class(n):
    if n in (1, 8, 128):
        return str(n)
    return "lt8" if n < 8 else "leaf" if n < NP_LEAF else "leaves" if n < NP_BLOCK else "blocks"


def derive_paths(step):
    reads, site_read, site_loc, norm, T, S, _ = step
    out = set()
    for r in reads:
        n = len(r[0])
        if n == 0:
            out.add("read:empty")
            continue
        if norm == "zscore":
            passes = -(-(n // NP_BLOCK) // WG_BLOCKS)
            out.add("z:passes=%s" % (passes if passes < 3 else "3+"))
            tail = n % NP_BLOCK
            out.add("z:tail=%s" % ("none" if tail == 0 else "lt8" if tail < 8 else "leaf" if tail <= NP_LEAF else "leaves"))
        else:
            span = int(r[0].max()) - int(r[0].min()) + 1
            chunks = -(-span // SCAN_CHUNK)
            out.add("mad:hist=%s" % ("lds" if span <= CDF_LDS else "global"))
            out.add("mad:chunks=%s" % (chunks if chunks < 3 else "3+"))
            out.add("mad:n=%s" % ("odd" if n % 2 else "even"))
    nb = (T - 1) // 2
    for rd, loc in zip(site_read, site_loc):
        lens = [int(v) for v in reads[rd][2][loc - nb:loc + nb + 1]]
        out |= {"win%d:%s" % (T, w) for w in _window_paths(lens, S)}
        out |= {"base:%s" % _base_class(v) for v in lens}
    return out


# ---- builders ------------------------------------------------------------------------------------------------------------
def _signal(n, rng):
    return np.clip(rng.normal(500, 80, n), -32768, 32767).astype(np.int16)


def _codes(nbases, locs, rng):
    codes = rng.choice(np.array([0, 2, 3], np.int8), nbases)
    locs = sorted(int(v) for v in locs)
    assert all(b - a >= 2 for a, b in zip(locs, locs[1:])) and (not locs or locs[-1] + 1 < nbases)
    for loc in locs:
        codes[loc], codes[loc + 1] = 1, 2
    return codes


def _spread_read(raw, T, rng, key, nsites=4):
    """A read over the given samples for its statistics: T - 1 + 2 * nsites short events spread evenly over it (they overlap
    when the read is shorter than they are together, which ds_reads allows), a site at every second usable base."""
    n, nb, nbases = len(raw), (T - 1) // 2, T - 1 + 2 * nsites
    starts = (np.arange(nbases, dtype=np.int64) * max(n - 15, 0)) // (nbases - 1)
    lengths = np.minimum(rng.integers(1, 16, nbases), n - starts).astype(np.int64)
    locs = [nb + 2 * i for i in range(nsites)]
    return (raw, starts, lengths, _codes(nbases, locs, rng), SCALING, OFFSET, key), locs


def _lens_read(lens, locs, rng, key, raw=None, lead=3):
    """A read whose events have the given lengths and tile the signal after `lead` samples."""
    lengths = np.asarray(lens, np.int64)
    starts = lead + np.concatenate([[0], np.cumsum(lengths)[:-1]]).astype(np.int64)
    n = lead + int(lengths.sum()) + 2
    if raw is None:
        raw = _signal(n, rng)
    assert len(raw) >= n
    return (raw, starts, lengths, _codes(len(lengths), locs, rng), SCALING, OFFSET, key)


def _synthetic(nbases, seed, key, T, nsites, long_bases=0):
    """synth.synthetic_read with `nsites` sites spread over its usable bases."""
    raw, starts, lengths, _, scaling, offset = synth.synthetic_read(nbases, seed, long_bases=long_bases)
    nb = (T - 1) // 2
    step = max(2, (nbases - 2 * nb - 2) // nsites)
    locs = [nb + step * i for i in range(nsites)]
    return (raw, starts, lengths, _codes(nbases, locs, np.random.default_rng(seed)), scaling, offset, key), locs


def _one(read_locs):
    """One step from [(read, locs), ...]."""
    reads = [r for r, _ in read_locs]
    sr = [i for i, (_, locs) in enumerate(read_locs) for _ in locs]
    sl = [loc for _, locs in read_locs for loc in locs]
    return (reads, sr, sl)


def _span_raw(n, lo, span, rng):
    raw = rng.integers(lo, lo + span, n).astype(np.int16)
    raw[0], raw[-1] = lo, lo + span - 1
    return raw


def _split(total, parts):
    assert total >= parts
    return [total // parts + (1 if i < total % parts else 0) for i in range(parts)]


def _segments(T, segs):
    """k-mers of chosen event lengths, one after another: segs = [(samples left of the middle base, middle base, samples right
    of it)]; the site of segment i is its middle base."""
    nb = (T - 1) // 2
    lens, locs = [], []
    for left, mid, right in segs:
        locs.append(len(lens) + nb)
        lens += _split(left, nb) + [mid] + _split(right, nb)
    return lens, locs


class Case:
    def __init__(self, name, group, build, paths, geometry=(17, 360), norms=("zscore", "mad"), degenerate=False, seed_name=None):
        self.name, self.group, self.build, self.paths = name, group, build, frozenset(paths)
        self.geometry, self.norms, self.degenerate = geometry, tuple(norms), degenerate
        self.seed = 1 + sum(ord(c) * (i + 1) for i, c in enumerate(seed_name or name)) % 100000

    def steps(self, norm):
        assert norm in self.norms
        T, S = self.geometry
        return [(reads, np.asarray(sr, np.int32), np.asarray(sl, np.int32), norm, T, S, self.seed % 97)
                for reads, sr, sl in _built(self)]

    def derived(self):
        return set().union(*(derive_paths(s) for norm in self.norms for s in self.steps(norm)))


@functools.lru_cache(maxsize=4)
def _built(case):
    return case.build(np.random.default_rng(case.seed), case.geometry[0], case.geometry[1])


CASES = []


def _add(*a, **k):
    CASES.append(Case(*a, **k))


# z-score block structure / MAD counts: (samples, passes of wg_np_sum, class of the partial last block)
STATS_N = [(5, "0", "lt8"), (8, "0", "leaf"), (100, "0", "leaf"), (128, "0", "leaf"), (129, "0", "leaves"), (8191, "0", "leaves"),
           (8192, "1", "none"), (8193, "1", "lt8"), (8192 * 3, "1", "none"), (8192 * 3 + 1, "1", "lt8"), (8192 * 3 + 7, "1", "lt8"),
           (8192 * 16, "1", "none"), (8192 * 16 + 127, "1", "leaf"), (8192 * 17, "2", "none"), (8192 * 17 + 4000, "2", "leaves"),
           (8192 * 33 + 129, "3+", "leaves"), (300007, "3+", "leaves"), (1050001, "3+", "leaves")]
for _n, _p, _t in STATS_N:
    _add("stats_n%d" % _n, "stats", lambda rng, T, S, n=_n: [_one([_spread_read(_signal(n, rng), T, rng, 11)])],
         {"z:passes=" + _p, "z:tail=" + _t, "mad:hist=lds", "mad:chunks=1", "mad:n=" + ("odd" if _n % 2 else "even")})


def _span_case(span, n, lo):
    return lambda rng, T, S: [_one([_spread_read(_span_raw(n, lo, span, rng), T, rng, 12)])]


for _span, _n, _lo, _paths in [
        (1024, 20001, 100, {"mad:hist=lds", "mad:chunks=1", "mad:n=odd"}),
        (1025, 20000, -500, {"mad:hist=lds", "mad:chunks=2", "mad:n=even"}),
        (8192, 20001, -4000, {"mad:hist=lds", "mad:chunks=3+"}),
        (8193, 20000, -4000, {"mad:hist=global", "mad:chunks=3+"}),
        (65536, 20001, -32768, {"mad:hist=global", "mad:chunks=3+"}),
        (8193, 300001, 0, {"mad:hist=global", "mad:n=odd"})]:
    _add("mad_span%d_n%d" % (_span, _n), "mad_span", _span_case(_span, _n, _lo), _paths, norms=("mad",))


def _two_values(rng, T, S):      # span 2, exactly half the samples each: the median falls between them
    raw = np.repeat(np.array([499, 500], np.int16), 5000)
    rng.shuffle(raw)
    return [_one([_spread_read(raw, T, rng, 13)])]


def _three_values(rng, T, S):    # heavy ties; 40 % of the samples equal the median, so the MAD is not 0
    raw = rng.choice(np.array([400, 500, 600], np.int16), 30001, p=[0.3, 0.4, 0.3])
    return [_one([_spread_read(raw, T, rng, 14)])]


_add("mad_span2", "mad_span", _two_values, {"mad:hist=lds", "mad:chunks=1", "mad:n=even"}, norms=("mad",))
_add("mad_three_values", "mad_span", _three_values, {"mad:hist=lds", "mad:n=odd"}, norms=("mad",))


# degenerate statistics: scale == 0, the host extractor yields NaN / +-inf
def _constant(n):
    return lambda rng, T, S: [_one([_spread_read(np.full(n, 517, np.int16), T, rng, 15)])]


def _mad_zero(rng, T, S):        # 60 % of the samples equal the median: MAD == 0, the rest normalise to +-inf
    raw = _signal(20000, rng)
    raw[rng.random(20000) < 0.6] = 500
    return [_one([_spread_read(raw, T, rng, 16)])]


# z-score of a constant read: the mean carries the rounding of its additions, so the deviations and the std are a few ulps,
# not 0, and every sample normalises to +-1 or NaN by the sign of that rounding error alone: any other order of additions shows
_add("constant_read", "degenerate", _constant(9000), {"mad:chunks=1", "z:passes=1"}, degenerate=True)
_add("constant_read_18_blocks", "degenerate", _constant(8192 * 17 + 4000), {"z:passes=2", "z:tail=leaves"}, norms=("zscore",),
     degenerate=True)
_add("constant_read_300k", "degenerate", _constant(300007), {"z:passes=3+", "z:tail=leaves"}, norms=("zscore",), degenerate=True)
_add("mad_is_zero", "degenerate", _mad_zero, {"mad:hist=lds"}, norms=("mad",), degenerate=True)


def _spiky(n, spike, nspikes, T, rng, key):
    raw = _signal(n, rng)
    raw[rng.choice(n, nspikes, replace=False)] = rng.integers(-spike, spike, nspikes).astype(np.int16)
    raw[0], raw[1] = -spike, spike - 1
    return _spread_read(raw, T, rng, key)


def _global_reuse(rng, T, S):
    """Global-memory histograms, batch after batch on one slot: read counts and spans differ, so every batch lays its
    histograms out differently over what the one before left there; the last batch is back in LDS."""
    return [_one([_spiky(30000, 4600, 30, T, rng, 1), _spiky(52001, 10000, 50, T, rng, 2), _spiky(40000, 32768, 40, T, rng, 3)]),
            _one([_spiky(61001, 20000, 60, T, rng, 4)]),
            _one([_spiky(20000, 15000, 30, T, rng, 5), _spiky(25001, 6000, 30, T, rng, 6)]),
            _one([_spread_read(_signal(45000, rng), T, rng, 7), _spread_read(_signal(9001, rng), T, rng, 8)])]


_add("global_histogram_reuse", "reuse", _global_reuse, {"mad:hist=global", "mad:hist=lds", "mad:chunks=3+"}, norms=("mad",))


def _mixed_reads(rng, T, with_empty=True):
    empty = ((np.zeros(0, np.int16), np.zeros(0, np.int64), np.zeros(0, np.int64), np.zeros(0, np.int8), SCALING, OFFSET, 24), [])
    return ([_spread_read(_signal(5000, rng), T, rng, 21)] + ([empty] if with_empty else []) +
            [_spread_read(_signal(8192 * 17 + 300, rng), T, rng, 22), _spiky(40001, 20000, 40, T, rng, 23)])


_add("mixed_batch", "mixed", lambda rng, T, S: [_one(_mixed_reads(rng, T))],
     {"read:empty", "z:passes=0", "z:passes=2", "mad:hist=lds", "mad:hist=global"})
# the same batch without its empty read (the two must agree on every site: tests compare them)
_add("mixed_batch_no_empty", "mixed", lambda rng, T, S: [_one(_mixed_reads(rng, T, with_empty=False))], {"z:passes=2"},
     seed_name="mixed_batch")


def _many_reads(rng, T, S):
    return [_one([_synthetic(T + 8 + i % 5, 5000 + i, 3000 + i, T, 1) for i in range(512)])]


def _many_sites(rng, T, S):
    return [_one([_synthetic(1100, 77, 31, T, 512)])]


_add("many_reads_512", "many", _many_reads, {"z:passes=0", "mad:hist=lds"})
_add("many_sites_512_one_read", "many", _many_sites, {"z:passes=1"})


def _window_modes(rng, T, S):
    nb = (T - 1) // 2
    half = (S - 6) // 2
    segs = [(S // 4, 5, S // 4),                  # PAD
            (half, 5, S - 6 - half),              # PAD, total == S - 1
            (half, 6, S - 6 - half),              # SPLIT, total == S: both halves taken whole
            (S, 10, S),                           # SPLIT, neither side short
            (nb, 10, 2 * S),                      # SPLIT, one sample per base left of the middle: left clamp
            (2 * S, 10, nb),                      # SPLIT, right clamp
            (40, S, 40),                          # SUB, len(mid) == S
            (40, S - 1, 40),                      # len(mid) == S - 1 stays SPLIT (left_len == 0)
            (40, 5003, 40)]                       # SUB of a very long middle base
    lens, locs = _segments(T, segs)
    return [_one([(_lens_read(lens, locs, rng, 41), locs)])]


def _base_lengths(rng, T, S):
    nb = (T - 1) // 2
    a = [1, 7, 8, 127] + [5] * (nb - 4) + [6] + [128, 129, 8192, 20011] + [4] * (nb - 4)
    b = [3] * nb + [8192 + 77] + [9] * nb         # a middle base of more than one numpy block (SUB)
    locs = [nb, T + nb]
    return [_one([(_lens_read(a + b, locs, rng, 42), locs)])]


for _T, _S in GEOMETRIES:
    _add("window_modes_k%d" % _T, "window", _window_modes, {"win%d:%s" % (_T, w) for w in WINDOW_PATHS}, geometry=(_T, _S))
    _add("base_lengths_k%d" % _T, "base", _base_lengths,
         {"base:%s" % b for b in ("1", "lt8", "8", "leaf", "128", "leaves", "blocks")}, geometry=(_T, _S))


def _growth(rng, T, S):
    """A small batch, one fifty times its size, the small one again."""
    small = _one([_synthetic(2000, 91, 51, T, 40)])
    large = _one([_spread_read(_signal(1000003, rng), T, rng, 52), _synthetic(3000, 92, 53, T, 60)])
    return [small, large, small]


_add("block_growth", "growth", _growth, {"z:passes=3+", "z:passes=1"})

BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)


def case_norm_params():
    return [(c.name, norm) for c in CASES for norm in c.norms]


KEYS = ("kmer", "means", "stds", "sanums", "signals")


def same_bits(a, b, nan_positions=False):
    """Equal shape and equal bits (floats compared as uint32). nan_positions (degenerate cases only): NaNs must sit at the
    same places, their sign and payload are not compared; every other value, +-inf included, bit for bit."""
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.dtype != np.float32:
        return np.array_equal(a, b)
    if not nan_positions:
        return np.array_equal(a.view(np.uint32), b.view(np.uint32))
    na, nb = np.isnan(a), np.isnan(b)
    return np.array_equal(na, nb) and np.array_equal(a.view(np.uint32)[~na], b.view(np.uint32)[~nb])
