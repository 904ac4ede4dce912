// ds_extract.hip — fast5 features on the device (scope row f2): raw int16 signal -> per-read normalisation statistics ->
// per-site k-mer codes, base means / stds / lengths and the central signal window, written straight into a pipeline slot's
// forward inputs. Arithmetic: ds_extract.h (shared with the host checker below); compiled with -ffp-contract=off.
//
// Two launches per batch. extract_stats_kernel: one workgroup per read; MAD builds the read's histogram of raw values
// (span = max - min + 1 bins, known from staging) with LDS atomics when it fits 8192 bins, else with global atomics in the slot's
// device block, scans it into a cumulative histogram and selects the median and the median deviation on it with binary
// searches (ds_extract.h mad_stats: exact, no sort); z-score sums in numpy's order (8192-sample blocks, each a pairwise tree
// whose 128-sample leaves are summed by one lane apiece; the partial last block's leaves likewise, its tree replayed by one lane). extract_sites_kernel: one wave per site; lanes 0 .. kmer_len-1
// each take one base (mean / std in numpy's order), all lanes fill the window. No matrix work: nothing here uses MFMAs.
#include "ds_extract.h"

#include <algorithm>
#include <cstring>

namespace dsx {
namespace {

constexpr int STATS_THREADS = 1024;     // one workgroup per read, and a batch holds only a few reads: as many lanes as a workgroup may have
constexpr int SITES_PER_WG = 4;
constexpr int CDF_LDS = 8192;           // histograms up to this many bins are built, scanned and searched in LDS (32 KB)
constexpr int TAIL_LEAVES = 128;        // leaves of numpy's pairwise tree over < 8192 samples: each holds >= 64 of them

template <class T>
__device__ inline T load_agent(const T* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// numpy's add.reduce of f(0) .. f(n - 1) by one workgroup; the result is valid in thread 0
template <class F>
__device__ double wg_np_sum(const F& f, int64_t n, double* part)
{
    const int tid = threadIdx.x, leaf = tid % 64;
    const int64_t nfull = n / NP_BLOCK;
    double s = 0.0;
    for (int64_t g = 0; g < nfull; g += STATS_THREADS / 64) {
        const int64_t b = g + tid / 64;
        part[tid] = b < nfull ? pw_leaf(f, b * NP_BLOCK + (int64_t)leaf * NP_PW_BLOCK, NP_PW_BLOCK) : 0.0;
        __syncthreads();
        for (int st = 1; st < 64; st <<= 1) {       // the 8192-sample block's pairwise tree is perfect: 64 leaves of 128
            if (leaf % (2 * st) == 0) part[tid] = part[tid] + part[tid + st];
            __syncthreads();
        }
        if (tid == 0)
            for (int j = 0; j < STATS_THREADS / 64 && g + j < nfull; ++j) s += part[j * 64];
        __syncthreads();
    }
    const int64_t tail = n % NP_BLOCK;
    if (tail) {      // the last, partial block: its leaves (<= 128, each >= 64 samples) summed in parallel, then the tree replayed
        __shared__ int64_t leaf_a[TAIL_LEAVES];
        __shared__ int32_t leaf_n[TAIL_LEAVES];
        __shared__ int nleaves;
        if (tid == 0) {
            int k = 0;
            pw_walk([&](int64_t la, int64_t ln) { leaf_a[k] = la; leaf_n[k] = (int32_t)ln; ++k; return 0.0; }, nfull * NP_BLOCK, tail);
            nleaves = k;
        }
        __syncthreads();
        if (tid < nleaves) part[tid] = pw_leaf(f, leaf_a[tid], leaf_n[tid]);
        __syncthreads();
        if (tid == 0) {
            int k = 0;
            s += pw_walk([&](int64_t, int64_t) { return part[k++]; }, nfull * NP_BLOCK, tail);
        }
        __syncthreads();
    }
    return s;
}

__global__ __launch_bounds__(STATS_THREADS) void extract_stats_kernel(ExtractArgs a)
{
    __shared__ double part[STATS_THREADS];
    __shared__ int32_t buf[STATS_THREADS];
    __shared__ int32_t cdf_lds[CDF_LDS];
    __shared__ double bcast;
    const int r = blockIdx.x, tid = threadIdx.x;
    const int64_t o = a.raw_off[r], n = a.raw_off[r + 1] - o;
    const int16_t* x = a.raw + o;
    const double sc = a.scaling[r], of = a.offset[r];
    if (a.norm == DS_NORM_MAD) {
        int32_t* h = a.hist + a.hist_off[r];
        const int vmin = a.vmin[r];
        const int span = (int)(a.hist_off[r + 1] - a.hist_off[r]);
        const bool in_lds = span <= CDF_LDS;      // the usual case (a read's raw values span a few hundred ADC steps)
        if (in_lds) {
            for (int i = tid; i < span; i += STATS_THREADS) cdf_lds[i] = 0;
            __syncthreads();
            for (int64_t i = tid; i < n; i += STATS_THREADS) atomicAdd(&cdf_lds[x[i] - vmin], 1);
        } else {
            for (int64_t i = tid; i < n; i += STATS_THREADS) atomicAdd(&h[x[i] - vmin], 1);
            __threadfence();
        }
        __syncthreads();
        int32_t carry = 0;
        for (int b0 = 0; b0 < span; b0 += STATS_THREADS) {           // inclusive scan, STATS_THREADS bins at a time
            buf[tid] = b0 + tid < span ? (in_lds ? cdf_lds[b0 + tid] : load_agent(&h[b0 + tid])) : 0;
            __syncthreads();
            for (int off = 1; off < STATS_THREADS; off <<= 1) {
                const int32_t t = tid >= off ? buf[tid - off] : 0;
                __syncthreads();
                buf[tid] += t;
                __syncthreads();
            }
            if (b0 + tid < span) {
                if (in_lds) cdf_lds[b0 + tid] = carry + buf[tid];
                else h[b0 + tid] = carry + buf[tid];
            }
            carry += buf[STATS_THREADS - 1];
            __syncthreads();
        }
        __threadfence();
        __syncthreads();
        if (tid == 0) {
            double shift, scale;
            if (in_lds) mad_stats([&](int i) -> int64_t { return cdf_lds[i]; }, span, vmin, n, sc, of, &shift, &scale);
            else mad_stats([&](int i) -> int64_t { return load_agent(&h[i]); }, span, vmin, n, sc, of, &shift, &scale);
            a.stats[2 * r] = shift;
            a.stats[2 * r + 1] = scale;
        }
        return;
    }
    auto f = [&](int64_t i) { return rescale(x[i], sc, of); };
    const double s = wg_np_sum(f, n, part);
    if (tid == 0) bcast = s / (double)n;
    __syncthreads();
    const double m = bcast;
    const double s2 = wg_np_sum([&](int64_t i) { const double d = f(i) - m; return d * d; }, n, part);
    if (tid == 0) {
        a.stats[2 * r] = m;
        a.stats[2 * r + 1] = sqrt(s2 / (double)n);
    }
}

// the features of site s in float64; lanes [lane, lane + nlanes, ...] of the work (the host checkers run it with one lane).
// out.base(j, code, mean, std, len) receives base j of the k-mer, out.signal(q, v) position q of the window.
template <class Sink>
__host__ __device__ inline void site_values(const ExtractArgs& a, int s, int lane, int nlanes, const Sink& out)
{
    const int T = a.T, S = a.S, nb = (T - 1) / 2, mid = (T - 1) / 2;
    const int r = a.site_read[s];
    const int64_t loc = a.site_loc[s];
    const int64_t b0 = a.base_off[r] + loc - nb;
    const int64_t* st = a.start + b0;
    const int32_t* ln = a.len + b0;
    const int16_t* x = a.raw + a.raw_off[r];
    const double sc = a.scaling[r], of = a.offset[r], shift = a.stats[2 * r], scale = a.stats[2 * r + 1];
    auto nv = [&](int64_t i) { return normalise(rescale(x[i], sc, of), shift, scale); };
    for (int j = lane; j < T; j += nlanes) {
        const int64_t s0 = st[j];
        double m, sd;
        np_mean_std([&](int64_t i) { return nv(s0 + i); }, ln[j], &m, &sd);
        out.base(j, a.code[b0 + j], m, sd, ln[j]);
    }
    auto lens = [&](int j) -> int64_t { return ln[j]; };
    auto starts = [&](int j) -> int64_t { return st[j]; };
    const Window w = window_plan(lens, T, S);
    if (w.mode == WIN_SUB) {
        if (lane == 0) {
            const uint64_t key = a.key ? a.key[r] : (uint64_t)r;
            const int64_t s0 = st[mid];
            subsample(a.seed, key, loc, ln[mid], S, [&](int k, int64_t i) { out.signal(k, nv(s0 + i)); });
        }
        return;
    }
    for (int q = lane; q < S; q += nlanes) {
        const int64_t src = window_source(w, lens, starts, T, q);
        out.signal(q, src < 0 ? 0.0 : nv(src));
    }
}

// the forward's inputs: the values narrowed to float32, rows of pitch T / S
struct FloatRows {
    int32_t* kmer; float *means, *stds, *sanums, *signals;
    int T, S, s;
    __host__ __device__ void base(int j, int code, double m, double sd, int len) const
    {
        kmer[(size_t)s * T + j] = code;
        means[(size_t)s * T + j] = (float)m;
        stds[(size_t)s * T + j] = (float)sd;
        sanums[(size_t)s * T + j] = (float)len;
    }
    __host__ __device__ void signal(int q, double v) const { signals[(size_t)s * S + q] = (float)v; }
};

__host__ __device__ inline void site_features(const ExtractArgs& a, int s, int lane, int nlanes, int32_t* kmer, float* means,
                                              float* stds, float* sanums, float* signals)
{
    site_values(a, s, lane, nlanes, FloatRows{kmer, means, stds, sanums, signals, a.T, a.S, s});
}

__global__ __launch_bounds__(64 * SITES_PER_WG) void extract_sites_kernel(ExtractArgs a, int32_t* kmer, float* means, float* stds,
                                                                          float* sanums, float* signals)
{
    const int s = blockIdx.x * SITES_PER_WG + threadIdx.x / 64;
    if (s >= a.nsites) return;
    site_features(a, s, threadIdx.x % 64, 64, kmer, means, stds, sanums, signals);
}

// ---- feature rows: the float64 values of a site, and their text (ds_extract.h: value_text .. elem_put) ------------------------
// the row's values as the text needs them: [means T | stds T | signals S] in float64 (k-mer codes and lengths are read from the
// staged reads)
struct DoubleRow {
    double* row;
    int T;
    __host__ __device__ void base(int j, int, double m, double sd, int) const { row[j] = m; row[T + j] = sd; }
    __host__ __device__ void signal(int q, double v) const { row[2 * T + q] = v; }
};

__global__ __launch_bounds__(64 * SITES_PER_WG) void rows_values_kernel(ExtractArgs a, double* vals)
{
    const int s = blockIdx.x * SITES_PER_WG + threadIdx.x / 64;
    if (s >= a.nsites) return;
    site_values(a, s, threadIdx.x % 64, 64, DoubleRow{vals + (size_t)s * (2 * a.T + a.S), a.T});
}

__host__ __device__ inline const int32_t* site_lens(const ExtractArgs& a, int s)
{
    return a.len + a.base_off[a.site_read[s]] + a.site_loc[s] - (a.T - 1) / 2;
}

// one wave per site: the row's byte length = leading columns, tab, k-mer letters, tab, every list element with its separator
__global__ __launch_bounds__(64 * SITES_PER_WG) void rows_len_kernel(ExtractArgs a, RowsArgs ra)
{
    const int s = blockIdx.x * SITES_PER_WG + threadIdx.x / 64, lane = threadIdx.x % 64;
    if (s >= a.nsites) return;
    const double* vals = ra.vals + (size_t)s * (2 * a.T + a.S);
    const int32_t* lens = site_lens(a, s);
    int n = 0;
    for (int e = lane; e < row_elems(a.T, a.S); e += 64) n += elem_len(row_elem(vals, lens, a.T, a.S, ra.label, e));
    for (int d = 32; d; d >>= 1) n += __shfl_down(n, d, 64);
    if (lane == 0) ra.row_len[s] = n + (int)(ra.info_off[s + 1] - ra.info_off[s]) + a.T + 2;
}

// exclusive scan of the n <= max_batch row lengths into off[0 .. n] by one workgroup: a run of consecutive rows per thread
constexpr int SCAN_THREADS = 1024;
__global__ __launch_bounds__(SCAN_THREADS) void rows_scan_kernel(const int32_t* len, int64_t* off, int n)
{
    __shared__ int64_t part[SCAN_THREADS];
    const int tid = threadIdx.x, per = (n + SCAN_THREADS - 1) / SCAN_THREADS;
    const int b = min(n, tid * per), e = min(n, b + per);
    int64_t sum = 0;
    for (int i = b; i < e; ++i) sum += len[i];
    part[tid] = sum;
    __syncthreads();
    for (int d = 1; d < SCAN_THREADS; d <<= 1) {
        const int64_t t = tid >= d ? part[tid - d] : 0;
        __syncthreads();
        part[tid] += t;
        __syncthreads();
    }
    int64_t run = part[tid] - sum;
    for (int i = b; i < e; ++i) { off[i] = run; run += len[i]; }
    if (tid == SCAN_THREADS - 1) off[n] = part[tid];
}

constexpr int CHUNK_TEXT = 64 * (VALUE_TEXT_MAX + 1);      // most bytes 64 elements take (a value is the longest element)
static_assert(VALUE_TEXT_MAX >= INT_TEXT_MAX, "an LDS chunk is sized by the longest element");

// One wave writes elements elem(0) .. elem(ne - 1) back to back at dst, 64 at a time: every lane takes one element, a wave scan of
// their lengths places them in the wave's LDS chunk, and the chunk leaves with consecutive lanes storing consecutive bytes.
// Every wave of the workgroup calls it with the same ne (idle waves with active == false): the chunk is handed over at
// workgroup barriers. Returns the bytes written.
template <class ElemFn>
__device__ inline int64_t wave_format(int lane, int ne, bool active, const ElemFn& elem, char* lds, char* dst)
{
    int64_t run = 0;
    for (int e0 = 0; e0 < ne; e0 += 64) {
        const int e = e0 + lane;
        RowElem el{};
        int len = 0;
        if (active && e < ne) { el = elem(e); len = elem_len(el); }
        int inc = len;
        for (int d = 1; d < 64; d <<= 1) {
            const int t = __shfl_up(inc, d, 64);
            if (lane >= d) inc += t;
        }
        const int total = __shfl(inc, 63, 64);
        if (len) elem_put(el, lds + (inc - len));
        __syncthreads();
        for (int b = lane; b < total; b += 64) dst[run + b] = lds[b];
        __syncthreads();
        run += total;
    }
    return run;
}

__global__ __launch_bounds__(64 * SITES_PER_WG) void rows_format_kernel(ExtractArgs a, RowsArgs ra)
{
    __shared__ char chunk[SITES_PER_WG][CHUNK_TEXT];
    const int w = threadIdx.x / 64, lane = threadIdx.x % 64;
    const int s = blockIdx.x * SITES_PER_WG + w;
    // a row that would end past the buffer is not written (the buffer is sized for the longest rows there can be)
    const bool active = s < a.nsites && ra.row_off[s + 1] <= ra.text_cap;
    const int sc = active ? s : 0;
    const int T = a.T, S = a.S;
    char* dst = ra.text + ra.row_off[sc];
    const int64_t i0 = ra.info_off[sc], ni = ra.info_off[sc + 1] - i0;
    if (active) {
        for (int64_t b = lane; b < ni; b += 64) dst[b] = ra.info[i0 + b];
        const int8_t* code = a.code + a.base_off[a.site_read[sc]] + a.site_loc[sc] - (T - 1) / 2;
        for (int j = lane; j < T; j += 64) dst[ni + 1 + j] = "ACGTN"[code[j]];
        if (lane == 0) { dst[ni] = '\t'; dst[ni + 1 + T] = '\t'; }
    }
    const double* vals = ra.vals + (size_t)sc * (2 * T + S);
    const int32_t* lens = site_lens(a, sc);
    wave_format(lane, row_elems(T, S), active, [&](int e) { return row_elem(vals, lens, T, S, ra.label, e); }, chunk[w],
                dst + ni + T + 2);
}

// ds_format_values on the device: one wave, the values comma-joined
__global__ __launch_bounds__(64) void format_values_kernel(const double* v, int64_t n, char* text, int64_t* total)
{
    __shared__ char chunk[CHUNK_TEXT];
    const int lane = threadIdx.x;
    int64_t run = 0;
    for (int64_t e0 = 0; e0 < n; e0 += 1 << 20) {      // wave_format counts elements in an int
        const int ne = (int)(n - e0 < (1 << 20) ? n - e0 : 1 << 20);
        run += wave_format(lane, ne, true, [&](int e) {
            return RowElem{false, value_text(v[e0 + e]), 0, e0 + e + 1 < n ? ',' : (char)0}; }, chunk, text + run);
    }
    if (lane == 0) *total = run;
}

size_t align_up(size_t v) { return (v + 15) & ~(size_t)15; }

}  // namespace

int plan(const ds_reads* r, int T, int S, int max_sites, ExtractPlan* p, std::string* err)
{
    auto bad = [&](const std::string& m) { *err = "ds_reads: " + m; return DS_ERR_INVALID; };
    if (!r) return bad("null descriptor");
    if (T < 1 || T % 2 == 0) return bad("kmer_len must be odd");
    if (S < 1) return bad("signal_len must be positive");
    if (r->nreads < 1) return bad("nreads must be >= 1");
    if (r->nsites < 1 || r->nsites > max_sites) return bad("nsites must be in [1, " + std::to_string(max_sites) + "]");
    if (!r->raw_off || !r->base_off || !r->start || !r->length || !r->base || !r->scaling || !r->offset || !r->site_read ||
        !r->site_loc)
        return bad("null array");
    if (r->norm != DS_NORM_MAD && r->norm != DS_NORM_ZSCORE) return bad("norm must be DS_NORM_MAD or DS_NORM_ZSCORE");
    const int R = r->nreads;
    if (r->raw_off[0] != 0 || r->base_off[0] != 0) return bad("raw_off[0] and base_off[0] must be 0");
    for (int i = 0; i < R; ++i) {
        if (r->raw_off[i + 1] < r->raw_off[i] || r->base_off[i + 1] < r->base_off[i]) return bad("offsets must be non-decreasing");
        if (r->raw_off[i + 1] - r->raw_off[i] > INT32_MAX) return bad("a read has more than 2^31 - 1 samples");
    }
    if (r->raw_off[R] > 0 && !r->raw) return bad("null array");
    p->nreads = R; p->nsites = r->nsites; p->T = T; p->S = S;
    p->nsamples = r->raw_off[R]; p->nbases = r->base_off[R];
    for (int i = 0; i < R; ++i) {
        const int64_t ns = r->raw_off[i + 1] - r->raw_off[i];
        for (int64_t b = r->base_off[i]; b < r->base_off[i + 1]; ++b) {
            if (r->start[b] < 0 || r->length[b] < 1 || r->start[b] + r->length[b] > ns)
                return bad("read " + std::to_string(i) + ": base " + std::to_string(b - r->base_off[i]) +
                           ": event runs outside the read's samples (or is empty)");
            if (r->base[b] < 0 || r->base[b] > 4) return bad("base codes must be in 0 .. 4");
        }
    }
    const int nb = (T - 1) / 2;
    for (int s = 0; s < r->nsites; ++s) {
        const int rd = r->site_read[s];
        if (rd < 0 || rd >= R) return bad("site_read out of range");
        const int64_t nbase = r->base_off[rd + 1] - r->base_off[rd];
        if (r->site_loc[s] < nb || r->site_loc[s] >= nbase - nb)
            return bad("site " + std::to_string(s) + ": loc " + std::to_string(r->site_loc[s]) + " has fewer than " +
                       std::to_string(nb) + " bases on one side");
    }
    p->vmin.assign(R, 0);
    p->hist_off.assign(R + 1, 0);
    for (int i = 0; i < R; ++i) {
        int lo = 0, hi = -1;
        if (r->norm == DS_NORM_MAD && r->raw_off[i + 1] > r->raw_off[i]) {
            lo = INT32_MAX; hi = INT32_MIN;
            for (int64_t k = r->raw_off[i]; k < r->raw_off[i + 1]; ++k) { lo = std::min<int>(lo, r->raw[k]); hi = std::max<int>(hi, r->raw[k]); }
        }
        p->vmin[i] = lo;
        p->hist_off[i + 1] = p->hist_off[i] + (hi - lo + 1);
    }
    size_t o = 0;
    auto take = [&](size_t bytes) { const size_t at = o; o = align_up(o + bytes); return at; };
    p->o_raw = take((size_t)p->nsamples * 2);
    p->o_raw_off = take((size_t)(R + 1) * 8);
    p->o_start = take((size_t)p->nbases * 8);
    p->o_len = take((size_t)p->nbases * 4);
    p->o_code = take((size_t)p->nbases);
    p->o_base_off = take((size_t)(R + 1) * 8);
    p->o_scaling = take((size_t)R * 8);
    p->o_offset = take((size_t)R * 8);
    p->o_key = take((size_t)R * 8);
    p->o_site_read = take((size_t)r->nsites * 4);
    p->o_site_loc = take((size_t)r->nsites * 4);
    p->o_vmin = take((size_t)R * 4);
    p->o_hist_off = take((size_t)(R + 1) * 8);
    p->image_bytes = o;
    p->o_stats = take((size_t)R * 16);
    p->o_hist = take((size_t)p->hist_off[R] * 4);
    p->device_bytes = o;
    return DS_OK;
}

void stage(const ds_reads* r, const ExtractPlan& p, char* dst)
{
    const int R = p.nreads;
    if (p.nsamples) memcpy(dst + p.o_raw, r->raw, (size_t)p.nsamples * 2);
    memcpy(dst + p.o_raw_off, r->raw_off, (size_t)(R + 1) * 8);
    memcpy(dst + p.o_start, r->start, (size_t)p.nbases * 8);
    memcpy(dst + p.o_len, r->length, (size_t)p.nbases * 4);
    memcpy(dst + p.o_code, r->base, (size_t)p.nbases);
    memcpy(dst + p.o_base_off, r->base_off, (size_t)(R + 1) * 8);
    memcpy(dst + p.o_scaling, r->scaling, (size_t)R * 8);
    memcpy(dst + p.o_offset, r->offset, (size_t)R * 8);
    uint64_t* key = reinterpret_cast<uint64_t*>(dst + p.o_key);
    for (int i = 0; i < R; ++i) key[i] = r->key ? r->key[i] : (uint64_t)i;
    memcpy(dst + p.o_site_read, r->site_read, (size_t)p.nsites * 4);
    memcpy(dst + p.o_site_loc, r->site_loc, (size_t)p.nsites * 4);
    memcpy(dst + p.o_vmin, p.vmin.data(), (size_t)R * 4);
    memcpy(dst + p.o_hist_off, p.hist_off.data(), (size_t)(R + 1) * 8);
}

ExtractArgs device_args(const ds_reads* r, const ExtractPlan& p, char* d)
{
    ExtractArgs a{};
    a.raw = reinterpret_cast<const int16_t*>(d + p.o_raw);
    a.raw_off = reinterpret_cast<const int64_t*>(d + p.o_raw_off);
    a.start = reinterpret_cast<const int64_t*>(d + p.o_start);
    a.len = reinterpret_cast<const int32_t*>(d + p.o_len);
    a.code = reinterpret_cast<const int8_t*>(d + p.o_code);
    a.base_off = reinterpret_cast<const int64_t*>(d + p.o_base_off);
    a.scaling = reinterpret_cast<const double*>(d + p.o_scaling);
    a.offset = reinterpret_cast<const double*>(d + p.o_offset);
    a.key = reinterpret_cast<const uint64_t*>(d + p.o_key);
    a.site_read = reinterpret_cast<const int32_t*>(d + p.o_site_read);
    a.site_loc = reinterpret_cast<const int32_t*>(d + p.o_site_loc);
    a.vmin = reinterpret_cast<const int32_t*>(d + p.o_vmin);
    a.hist_off = reinterpret_cast<const int64_t*>(d + p.o_hist_off);
    a.stats = reinterpret_cast<double*>(d + p.o_stats);
    a.hist = reinterpret_cast<int32_t*>(d + p.o_hist);
    a.T = p.T; a.S = p.S; a.norm = r->norm; a.nsites = p.nsites; a.seed = r->seed;
    return a;
}

hipError_t launch(const ExtractPlan& p, const ExtractArgs& a, char* d_block, int32_t* kmer, float* means, float* stds,
                  float* sanums, float* signals, hipStream_t stream, hipEvent_t* ev)
{
    hipError_t e = hipSuccess;
    if (p.hist_off[p.nreads] > 0 && (e = hipMemsetAsync(d_block + p.o_hist, 0, (size_t)p.hist_off[p.nreads] * 4, stream)) != hipSuccess)
        return e;
    if (ev && (e = hipEventRecord(ev[0], stream)) != hipSuccess) return e;
    hipLaunchKernelGGL(extract_stats_kernel, dim3(p.nreads), dim3(STATS_THREADS), 0, stream, a);
    if (ev && (e = hipEventRecord(ev[1], stream)) != hipSuccess) return e;
    hipLaunchKernelGGL(extract_sites_kernel, dim3((p.nsites + SITES_PER_WG - 1) / SITES_PER_WG), dim3(64 * SITES_PER_WG), 0, stream,
                       a, kmer, means, stds, sanums, signals);
    if (ev && (e = hipEventRecord(ev[2], stream)) != hipSuccess) return e;
    return hipGetLastError();
}

namespace {

// the per-read statistics on the CPU and the checker's view of r (host pointers)
ExtractArgs host_args(const ds_reads* r, const ExtractPlan& p, int T, int S, std::vector<double>* stats)
{
    stats->assign((size_t)p.nreads * 2, 0.0);
    for (int i = 0; i < p.nreads; ++i) {
        const int16_t* x = r->raw + r->raw_off[i];
        const int64_t n = r->raw_off[i + 1] - r->raw_off[i];
        const double sc = r->scaling[i], of = r->offset[i];
        double* st = stats->data() + 2 * i;
        if (r->norm == DS_NORM_MAD) {
            const int span = (int)(p.hist_off[i + 1] - p.hist_off[i]), vmin = p.vmin[i];
            std::vector<int64_t> cdf(std::max(span, 1), 0);
            for (int64_t k = 0; k < n; ++k) cdf[x[k] - vmin] += 1;
            for (int k = 1; k < span; ++k) cdf[k] += cdf[k - 1];
            mad_stats([&](int k) { return cdf[k]; }, span, vmin, n, sc, of, &st[0], &st[1]);
        } else {
            np_mean_std([&](int64_t k) { return rescale(x[k], sc, of); }, n, &st[0], &st[1]);
        }
    }
    ExtractArgs a{};
    a.raw = r->raw; a.raw_off = r->raw_off; a.start = r->start; a.len = r->length; a.code = r->base; a.base_off = r->base_off;
    a.scaling = r->scaling; a.offset = r->offset; a.key = r->key; a.site_read = r->site_read; a.site_loc = r->site_loc;
    a.stats = stats->data(); a.T = T; a.S = S; a.norm = r->norm; a.nsites = r->nsites; a.seed = r->seed;
    return a;
}

}  // namespace

// host checker: the same functions on the CPU, one read / site at a time
int reference(const ds_reads* r, int T, int S, int32_t* kmer, float* means, float* stds, float* sanums, float* signals,
              std::string* err)
{
    if (!kmer || !means || !stds || !sanums || !signals) { *err = "ds_extract_reference: null output"; return DS_ERR_INVALID; }
    ExtractPlan p;
    int rc = plan(r, T, S, INT32_MAX, &p, err);
    if (rc) return rc;
    std::vector<double> stats;
    const ExtractArgs a = host_args(r, p, T, S, &stats);
    for (int s = 0; s < r->nsites; ++s) site_features(a, s, 0, 1, kmer, means, stds, sanums, signals);
    return DS_OK;
}

int64_t check_info(const char* info, const int64_t* info_off, int nsites, std::string* err)
{
    if (!info_off || info_off[0] != 0) { *err = "rows: info_off must start at 0"; return DS_ERR_INVALID; }
    for (int i = 0; i < nsites; ++i)
        if (info_off[i + 1] < info_off[i]) { *err = "rows: info_off must be non-decreasing"; return DS_ERR_INVALID; }
    if (info_off[nsites] > 0 && !info) { *err = "rows: null info"; return DS_ERR_INVALID; }
    return info_off[nsites];
}

hipError_t launch_rows(const ExtractPlan& p, const ExtractArgs& a, const RowsArgs& ra, char* d_block, hipStream_t stream,
                       hipEvent_t* ev)
{
    hipError_t e = hipSuccess;
    if (p.hist_off[p.nreads] > 0 && (e = hipMemsetAsync(d_block + p.o_hist, 0, (size_t)p.hist_off[p.nreads] * 4, stream)) != hipSuccess)
        return e;
    const dim3 site_grid((p.nsites + SITES_PER_WG - 1) / SITES_PER_WG), site_block(64 * SITES_PER_WG);
    if (ev && (e = hipEventRecord(ev[0], stream)) != hipSuccess) return e;
    hipLaunchKernelGGL(extract_stats_kernel, dim3(p.nreads), dim3(STATS_THREADS), 0, stream, a);
    if (ev && (e = hipEventRecord(ev[1], stream)) != hipSuccess) return e;
    hipLaunchKernelGGL(rows_values_kernel, site_grid, site_block, 0, stream, a, ra.vals);
    if (ev && (e = hipEventRecord(ev[2], stream)) != hipSuccess) return e;
    hipLaunchKernelGGL(rows_len_kernel, site_grid, site_block, 0, stream, a, ra);
    hipLaunchKernelGGL(rows_scan_kernel, dim3(1), dim3(SCAN_THREADS), 0, stream, ra.row_len, ra.row_off, p.nsites);
    if (ev && (e = hipEventRecord(ev[3], stream)) != hipSuccess) return e;
    hipLaunchKernelGGL(rows_format_kernel, site_grid, site_block, 0, stream, a, ra);
    if (ev && (e = hipEventRecord(ev[4], stream)) != hipSuccess) return e;
    return hipGetLastError();
}

int rows_reference(const ds_reads* r, int T, int S, const char* info, const int64_t* info_off, int64_t label, std::string* text,
                   std::vector<int64_t>* off, std::string* err)
{
    ExtractPlan p;
    int rc = plan(r, T, S, INT32_MAX, &p, err);
    if (rc) return rc;
    if (check_info(info, info_off, p.nsites, err) < 0) return DS_ERR_INVALID;
    std::vector<double> stats, vals((size_t)2 * T + S);
    const ExtractArgs a = host_args(r, p, T, S, &stats);
    text->clear();
    off->assign(1, 0);
    char buf[VALUE_TEXT_MAX + 1];
    for (int s = 0; s < p.nsites; ++s) {
        site_values(a, s, 0, 1, DoubleRow{vals.data(), T});
        text->append(info + info_off[s], (size_t)(info_off[s + 1] - info_off[s]));
        text->push_back('\t');
        const int8_t* code = a.code + a.base_off[a.site_read[s]] + a.site_loc[s] - (T - 1) / 2;
        for (int j = 0; j < T; ++j) text->push_back("ACGTN"[code[j]]);
        text->push_back('\t');
        const int32_t* lens = site_lens(a, s);
        for (int e = 0; e < row_elems(T, S); ++e) {
            const RowElem el = row_elem(vals.data(), lens, T, S, label, e);
            elem_put(el, buf);
            text->append(buf, (size_t)elem_len(el));
        }
        off->push_back((int64_t)text->size());
    }
    return DS_OK;
}

std::string format_values_host(const double* v, int64_t n)
{
    std::string out;
    char buf[VALUE_TEXT_MAX + 1];
    for (int64_t i = 0; i < n; ++i) {
        const RowElem el{false, value_text(v[i]), 0, i + 1 < n ? ',' : (char)0};
        elem_put(el, buf);
        out.append(buf, (size_t)elem_len(el));
    }
    return out;
}

hipError_t launch_format_values(const double* d_vals, int64_t n, char* d_text, int64_t* d_total, hipStream_t stream)
{
    hipLaunchKernelGGL(format_values_kernel, dim3(1), dim3(64), 0, stream, d_vals, n, d_text, d_total);
    return hipGetLastError();
}

}  // namespace dsx
