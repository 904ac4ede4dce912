// ds_extract.h — the arithmetic of the fast5 feature extraction (scope row f2 on the device), shared by the gfx950 kernels and
// the host checker ds_extract_reference (both in ds_extract.hip). Every function here is __host__ __device__ so that the CPU
// reference and the kernels are the same code; the translation unit is compiled with -ffp-contract=off (csrc/Makefile): an FMA
// contraction of a*b + c would round once where numpy rounds twice and break the bit-identity with the host extractor
// (deepsignal_amd/extract_features.py). Not part of the public ABI.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

namespace dsx {

#define DSX_HD __host__ __device__ inline

constexpr double MAD_CONSISTENCY = 0.6744897501960817;   // Phi^-1(3/4), extract_features.MAD_NORMAL_CONSISTENCY
constexpr int64_t NP_BLOCK = 8192;                       // numpy's reduction buffer: add.reduce sums blocks of this many
constexpr int NP_PW_BLOCK = 128;                         // numpy pairwise_sum: unrolled leaf size

// raw int16 -> pA, as extract_features._rescale_signals: scaling * (raw + offset) in float64
DSX_HD double rescale(int v, double scaling, double offset) { return scaling * ((double)v + offset); }

// one normalised sample, as extract_features._normalize_signals: np.around((x - shift) / scale, 6) == rint(y * 1e6) / 1e6
DSX_HD double normalise(double x, double shift, double scale) { return rint(((x - shift) / scale) * 1e6) / 1e6; }

// numpy pairwise_sum (numpy/_core/src/umath/loops_utils.h.src) of f(a) .. f(a + n - 1):
// n < 8 a plain loop; n <= 128 eight accumulators; above, split at n/2 rounded down to a multiple of 8
template <class F>
DSX_HD double pw_leaf(const F& f, int64_t a, int64_t n)
{
    if (n < 8) {
        double res = 0.;
        for (int64_t i = 0; i < n; ++i) res += f(a + i);
        return res;
    }
    double r[8];
    for (int j = 0; j < 8; ++j) r[j] = f(a + j);
    int64_t i = 8;
    for (; i < n - (n % 8); i += 8)
        for (int j = 0; j < 8; ++j) r[j] += f(a + i + j);
    double res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
    for (; i < n; ++i) res += f(a + i);
    return res;
}

// the recursion as an explicit post-order walk (no device recursion, no unrolled tree): n <= 8192 is at most 8 levels deep.
// leaf(a, n) gives the value of the leaf [a, a + n) (n <= 128); the leaves are visited left to right.
template <class Leaf>
DSX_HD double pw_walk(const Leaf& leaf, int64_t a, int64_t n)
{
    if (n <= NP_PW_BLOCK) return leaf(a, n);
    struct Frame { int64_t a, n; double left; int stage; };
    Frame st[16];
    int sp = 0;
    st[0] = Frame{a, n, 0.0, 0};
    double ret = 0.0;
    bool have = false;               // ret holds the value of the frame on top of the stack
    for (;;) {
        Frame& fr = st[sp];
        if (!have) {
            if (fr.n <= NP_PW_BLOCK) {
                ret = leaf(fr.a, fr.n);
                have = true;
            } else {
                int64_t n2 = fr.n / 2;
                n2 -= n2 % 8;
                fr.stage = 1;
                st[++sp] = Frame{fr.a, n2, 0.0, 0};
                continue;
            }
        } else if (fr.stage == 1) {      // left half done: walk the right half
            int64_t n2 = fr.n / 2;
            n2 -= n2 % 8;
            fr.left = ret;
            fr.stage = 2;
            have = false;
            st[++sp] = Frame{fr.a + n2, fr.n - n2, 0.0, 0};
            continue;
        } else {
            ret = fr.left + ret;
        }
        if (sp == 0) return ret;
        --sp;
    }
}

template <class F>
DSX_HD double pw_sum(const F& f, int64_t a, int64_t n)
{
    return pw_walk([&](int64_t la, int64_t ln) { return pw_leaf(f, la, ln); }, a, n);
}

// np.add.reduce of a contiguous float64 array: 0.0 plus the pairwise sums of consecutive 8192-element blocks, in order
template <class F>
DSX_HD double np_sum(const F& f, int64_t n)
{
    double s = 0.0;
    for (int64_t b = 0; b < n; b += NP_BLOCK) s += pw_sum(f, b, n - b < NP_BLOCK ? n - b : NP_BLOCK);
    return s;
}

// np.mean / np.std (population) of f(0) .. f(n - 1)
template <class F>
DSX_HD void np_mean_std(const F& f, int64_t n, double* mean, double* std)
{
    const double m = np_sum(f, n) / (double)n;
    const double v = np_sum([&](int64_t i) { const double d = f(i) - m; return d * d; }, n) / (double)n;
    *mean = m;
    *std = sqrt(v);
}

// ---- order statistics of a read through the cumulative histogram of its raw int16 values --------------------------------
// cdf[i] = number of samples with raw <= vmin + i, i in [0, span). The rescale is monotone, so the k-th smallest rescaled
// sample is the rescale of the k-th smallest raw value; no float sort is needed.
template <class C>
DSX_HD int select_raw(const C& cdf, int span, int64_t k)      // smallest i with cdf[i] >= k + 1
{
    int lo = 0, hi = span - 1;
    while (lo < hi) {
        const int mid = lo + (hi - lo) / 2;
        if (cdf(mid) >= k + 1) hi = mid; else lo = mid + 1;
    }
    return lo;
}

// np.median of n values given the order-statistic function: odd n the middle one, even n np.mean of the two middle ones
template <class O>
DSX_HD double np_median(const O& order, int64_t n)
{
    if (n % 2) return (0.0 + order(n / 2)) / 1.0;
    return ((0.0 + order(n / 2 - 1)) + order(n / 2)) / 2.0;
}

// MAD statistics of one read: shift = median, scale = median(|x - median|) / 0.6744897501960817.
// |r(v) - med| is non-increasing in v below the first value whose rescale reaches the median (p) and non-decreasing from p on,
// so "how many samples lie within D of the median" is a cdf difference over one raw interval, and the k-th smallest deviation
// is found by a binary search on each side.
template <class C>
DSX_HD void mad_stats(const C& cdf, int span, int vmin, int64_t n, double scaling, double offset, double* shift, double* scale)
{
    auto r = [&](int i) { return rescale(vmin + i, scaling, offset); };
    const double med = np_median([&](int64_t k) { return r(select_raw(cdf, span, k)); }, n);
    auto dev = [&](int i) { return fabs(r(i) - med); };
    int p = 0;                                          // first index whose rescale is >= med
    {
        int lo = 0, hi = span;
        while (lo < hi) { const int mid = lo + (hi - lo) / 2; if (r(mid) >= med) hi = mid; else lo = mid + 1; }
        p = lo;
    }
    auto cdf_at = [&](int i) -> int64_t { return i < 0 ? 0 : cdf(i); };
    auto count_le = [&](double D) -> int64_t {         // samples whose deviation is <= D
        int lo = p, hi = span;                          // upper side: one past the last i >= p with dev(i) <= D
        while (lo < hi) { const int mid = lo + (hi - lo) / 2; if (dev(mid) <= D) lo = mid + 1; else hi = mid; }
        const int U = lo - 1;
        int a = 0, b = p;                               // lower side: first i < p with dev(i) <= D
        while (a < b) { const int mid = a + (b - a) / 2; if (dev(mid) <= D) b = mid; else a = mid + 1; }
        const int L = a;
        return cdf_at(U) - cdf_at(L - 1);
    };
    auto kth_dev = [&](int64_t k) -> double {
        double best = INFINITY;
        {   // upper side: smallest i in [p, span) with count_le(dev(i)) >= k + 1
            int lo = p, hi = span;
            while (lo < hi) { const int mid = lo + (hi - lo) / 2; if (count_le(dev(mid)) >= k + 1) hi = mid; else lo = mid + 1; }
            if (lo < span) best = dev(lo);
        }
        {   // lower side: largest i in [0, p) with count_le(dev(i)) >= k + 1
            int lo = -1, hi = p - 1;
            while (lo < hi) { const int mid = hi - (hi - lo) / 2; if (count_le(dev(mid)) >= k + 1) lo = mid; else hi = mid - 1; }
            if (lo >= 0 && dev(lo) < best) best = dev(lo);
        }
        return best;
    };
    *shift = med;
    *scale = np_median(kth_dev, n) / MAD_CONSISTENCY;
}

// ---- the central signal window (extract_features._get_central_signals) ---------------------------------------------------
// Window position q of a site: which base / sample of the k-mer it comes from. Bases are lens[0..T), their samples are the
// read's samples starts[j] .. starts[j] + lens[j]. Modes: PAD = all k-mer samples concatenated, then zeros; SPLIT = the last
// left_len samples of the bases left of the middle, then the first right_len samples from the middle base on; SUB = the middle
// base alone holds >= S samples: an ordered subsample of it (subsample).
enum WindowMode { WIN_PAD = 0, WIN_SPLIT = 1, WIN_SUB = 2 };

struct Window {
    int mode;
    int64_t left_len, right_len, left_total;
};

template <class L>
DSX_HD Window window_plan(const L& lens, int T, int S)
{
    Window w{WIN_PAD, 0, 0, 0};
    int64_t total = 0;
    for (int j = 0; j < T; ++j) total += lens(j);
    if (total < S) return w;
    const int mid = (T - 1) / 2;
    if (lens(mid) >= S) { w.mode = WIN_SUB; return w; }
    int64_t left = 0;
    for (int j = 0; j < mid; ++j) left += lens(j);
    const int64_t right = total - left;
    int64_t left_len = (S - lens(mid)) / 2, right_len = S - left_len;
    if (left_len > left) { right_len += left_len - left; left_len = left; }
    else if (right_len > right) { left_len += right_len - right; right_len = right; }
    w.mode = WIN_SPLIT; w.left_len = left_len; w.right_len = right_len; w.left_total = left;
    return w;
}

// PAD / SPLIT: sample index (into the read) of window position q, or -1 for a zero pad
template <class L, class St>
DSX_HD int64_t window_source(const Window& w, const L& lens, const St& starts, int T, int64_t q)
{
    int64_t c = q;                                   // position in the concatenation of the k-mer's samples
    if (w.mode == WIN_SPLIT) c = q < w.left_len ? w.left_total - w.left_len + q : w.left_total + (q - w.left_len);
    for (int j = 0; j < T; ++j) {
        const int64_t l = lens(j);
        if (c < l) return starts(j) + c;
        c -= l;
    }
    return -1;
}

// counter-based uniform double in [0, 1) (splitmix64 finaliser) of (seed, key, loc, i)
DSX_HD double uniform(uint64_t seed, uint64_t key, int64_t loc, int64_t i)
{
    uint64_t x = seed ^ (key * 0x9E3779B97F4A7C15ull) ^ ((uint64_t)loc * 0xC2B2AE3D27D4EB4Full) ^ ((uint64_t)i * 0x165667B19E3779F9ull);
    x += 0x9E3779B97F4A7C15ull;
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
    x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
    x ^= x >> 31;
    return (double)(x >> 11) * (1.0 / 9007199254740992.0);
}

// SUB: Knuth's selection sampling (TAOCP 3.4.2, algorithm S) of S of the middle base's L samples, in increasing index order;
// emit(k, i) receives the k-th chosen sample index i (0 <= i < L)
template <class E>
DSX_HD void subsample(uint64_t seed, uint64_t key, int64_t loc, int64_t L, int S, const E& emit)
{
    int k = 0;
    for (int64_t i = 0; i < L && k < S; ++i)
        if ((double)(L - i) * uniform(seed, key, loc, i) < (double)(S - k)) emit(k++, i);
}

// ---- the text of a feature row (extract_features._features_to_str) ------------------------------------------------------------
// Every float of a row is np.around(v, 6) == rint(v * 1e6) / 1e6, and str() of such a float64 is a function of the integer
// K = rint(v * 1e6) and its sign bit alone (for |K| < 1e15; checked against numpy on 600 k values): K == +-0 prints 0.0 / -0.0;
// 1 <= |K| < 100 prints the exponent form 1e-06, 1.2e-05, 9.9e-05; above, <K div 1e6>.<the six fraction digits without their
// trailing zeros, at least one kept>. NaN prints nan whatever its sign, +-inf inf / -inf. So a value is integer-to-decimal work.
// |K| from 2^63 on prints as +-inf: far outside what a normalised sample can be, and it bounds a value's text (VALUE_TEXT_MAX).
constexpr int VALUE_TEXT_MAX = 27;       // sign, 19 integer digits, point, six fraction digits
constexpr int INT_TEXT_MAX = 20;         // sign and the 19 digits of an int64

struct ValueText { int kind; bool neg; uint64_t a; };      // kind 0: the number +-a / 1e6, 1: nan, 2: +-inf

DSX_HD ValueText value_text(double v)
{
    ValueText t{0, false, 0};
    if (v != v) { t.kind = 1; return t; }
    const double k = rint(v * 1e6);
    t.neg = __builtin_signbit(k) != 0;
    const double ak = fabs(k);
    if (!(ak < 9.2e18)) { t.kind = 2; return t; }
    t.a = (uint64_t)ak;
    return t;
}

DSX_HD int dec_digits(uint64_t x) { int n = 1; while (x >= 10) { x /= 10; ++n; } return n; }
DSX_HD void put_dec(uint64_t x, int nd, char* dst) { for (int i = nd - 1; i >= 0; --i) { dst[i] = (char)('0' + x % 10); x /= 10; } }

DSX_HD int value_len(const ValueText& t)
{
    if (t.kind == 1) return 3;
    if (t.kind == 2) return 3 + (t.neg ? 1 : 0);
    const int n = t.neg ? 1 : 0;
    if (t.a == 0) return n + 3;
    if (t.a < 100) return n + (t.a < 10 || t.a % 10 == 0 ? 5 : 7);
    uint32_t f = (uint32_t)(t.a % 1000000);
    int fd = 6;
    if (f == 0) fd = 1; else while (f % 10 == 0) { f /= 10; --fd; }
    return n + dec_digits(t.a / 1000000) + 1 + fd;
}

// writes value_len(t) characters at dst
DSX_HD void value_put(const ValueText& t, char* dst)
{
    if (t.kind == 1) { dst[0] = 'n'; dst[1] = 'a'; dst[2] = 'n'; return; }
    if (t.neg) *dst++ = '-';
    if (t.kind == 2) { dst[0] = 'i'; dst[1] = 'n'; dst[2] = 'f'; return; }
    if (t.a == 0) { dst[0] = '0'; dst[1] = '.'; dst[2] = '0'; return; }
    if (t.a < 100) {
        const bool tens = t.a >= 10;
        const int lead = tens ? (int)(t.a / 10) : (int)t.a, frac = tens ? (int)(t.a % 10) : 0;
        *dst++ = (char)('0' + lead);
        if (frac) { *dst++ = '.'; *dst++ = (char)('0' + frac); }
        dst[0] = 'e'; dst[1] = '-'; dst[2] = '0'; dst[3] = tens ? '5' : '6';
        return;
    }
    const uint64_t ip = t.a / 1000000;
    uint32_t f = (uint32_t)(t.a % 1000000);
    const int nd = dec_digits(ip);
    put_dec(ip, nd, dst);
    dst += nd;
    *dst++ = '.';
    int fd = 6;
    if (f == 0) fd = 1; else while (f % 10 == 0) { f /= 10; --fd; }
    put_dec(f, fd, dst);
}

DSX_HD int int_len(int64_t v) { return (v < 0 ? 1 : 0) + dec_digits(v < 0 ? 0 - (uint64_t)v : (uint64_t)v); }
DSX_HD void int_put(int64_t v, char* dst)
{
    const uint64_t a = v < 0 ? 0 - (uint64_t)v : (uint64_t)v;
    if (v < 0) *dst++ = '-';
    put_dec(a, dec_digits(a), dst);
}

// One element of a row's lists, in row order: e in [0, T) means, [T, 2T) stds, [2T, 3T) lens, [3T, 3T + S) signals, 3T + S the
// label; each is followed by sep (',' inside a list, '\t' behind it, '\n' behind the label; 0: nothing follows).
struct RowElem { bool is_int; ValueText v; int64_t i; char sep; };

DSX_HD int row_elems(int T, int S) { return 3 * T + S + 1; }

// vals: the site's float64 values [means T | stds T | signals S]; lens: the k-mer's event lengths
DSX_HD RowElem row_elem(const double* vals, const int32_t* lens, int T, int S, int64_t label, int e)
{
    RowElem el{false, ValueText{0, false, 0}, 0, ','};
    if (e < 2 * T) el.v = value_text(vals[e]);
    else if (e < 3 * T) { el.is_int = true; el.i = lens[e - 2 * T]; }
    else if (e < 3 * T + S) el.v = value_text(vals[e - T]);
    else { el.is_int = true; el.i = label; el.sep = '\n'; }
    if (e == T - 1 || e == 2 * T - 1 || e == 3 * T - 1 || e == 3 * T + S - 1) el.sep = '\t';
    return el;
}

DSX_HD int elem_len(const RowElem& el) { return (el.is_int ? int_len(el.i) : value_len(el.v)) + (el.sep ? 1 : 0); }
DSX_HD void elem_put(const RowElem& el, char* dst)
{
    const int n = el.is_int ? int_len(el.i) : value_len(el.v);
    if (el.is_int) int_put(el.i, dst); else value_put(el.v, dst);
    if (el.sep) dst[n] = el.sep;
}

// most bytes a row can take beside its leading columns: k-mer letters, lists, label, separators
DSX_HD int64_t row_text_max(int T, int S)
{
    return (int64_t)(VALUE_TEXT_MAX + 1) * (2 * T + S) + (int64_t)(INT_TEXT_MAX + 1) * (T + 1) + T + 2;
}

}  // namespace dsx

// ---- host <-> device plumbing (ds_extract.hip; used by ds_engine.cpp) -------------------------------------------------
#include <string>
#include <vector>
#include "../../include/deepsignal_hip.h"

namespace dsx {

// device pointers of one staged batch of reads (ds_reads packed into one block, plus the device-only tail)
struct ExtractArgs {
    const int16_t* raw; const int64_t* raw_off;
    const int64_t* start; const int32_t* len; const int8_t* code; const int64_t* base_off;
    const double* scaling; const double* offset; const uint64_t* key;
    const int32_t* site_read; const int32_t* site_loc;
    const int32_t* vmin; const int64_t* hist_off;
    double* stats;            // [nreads][2]: shift, scale
    int32_t* hist;            // cumulative histograms of the raw values, hist_off[r] .. hist_off[r + 1]
    int32_t T, S, norm, nsites;
    uint64_t seed;
};

// a validated ds_reads: the byte layout of its packed image (copied to the device as one block) and of the device-only tail
struct ExtractPlan {
    int32_t nreads = 0, nsites = 0, T = 0, S = 0;
    int64_t nsamples = 0, nbases = 0;
    std::vector<int32_t> vmin;
    std::vector<int64_t> hist_off;
    size_t o_raw = 0, o_raw_off = 0, o_start = 0, o_len = 0, o_code = 0, o_base_off = 0, o_scaling = 0, o_offset = 0,
           o_key = 0, o_site_read = 0, o_site_loc = 0, o_vmin = 0, o_hist_off = 0, image_bytes = 0;
    size_t o_stats = 0, o_hist = 0, device_bytes = 0;
};

// every check of the ABI (DS_ERR_INVALID + message); max_sites bounds nsites
int plan(const ds_reads* r, int T, int S, int max_sites, ExtractPlan* p, std::string* err);
// the packed image of r at dst (p.image_bytes)
void stage(const ds_reads* r, const ExtractPlan& p, char* dst);
ExtractArgs device_args(const ds_reads* r, const ExtractPlan& p, char* d_block);
// on `stream`: clear the histograms, per-read statistics, per-site features into rows of kmer / means / stds / sanums (pitch
// T) and signals (pitch S). ev (optional, 3 events): recorded before, between and after the two kernels
hipError_t launch(const ExtractPlan& p, const ExtractArgs& a, char* d_block, int32_t* kmer, float* means, float* stds,
                  float* sanums, float* signals, hipStream_t stream, hipEvent_t* ev);
// ds_extract_reference: the same features on the CPU (rows of pitch T / S)
int reference(const ds_reads* r, int T, int S, int32_t* kmer, float* means, float* stds, float* sanums, float* signals,
              std::string* err);

// ---- feature rows (ds_submit_rows / ds_extract_rows): device pointers of the rows path of one batch
struct RowsArgs {
    const char* info; const int64_t* info_off;   // the rows' six leading columns: row i is info[info_off[i] .. info_off[i + 1])
    double* vals;                                // [nsites][2T + S]: means | stds | signals in float64
    int32_t* row_len;                            // [nsites]
    int64_t* row_off;                            // [nsites + 1]
    char* text; int64_t text_cap;                // the rows, back to back in site order
    int64_t label;
};
// the validated info / info_off of a rows call: total bytes, or DS_ERR_INVALID
int64_t check_info(const char* info, const int64_t* info_off, int nsites, std::string* err);
// on `stream`: clear the histograms, per-read statistics, per-site float64 values, row lengths, their scan, the rows' text.
// ev (optional, 5 events): recorded around the four kernels
hipError_t launch_rows(const ExtractPlan& p, const ExtractArgs& a, const RowsArgs& ra, char* d_block, hipStream_t stream,
                       hipEvent_t* ev);
// ds_extract_rows_reference: the same rows on the CPU
int rows_reference(const ds_reads* r, int T, int S, const char* info, const int64_t* info_off, int64_t label, std::string* text,
                   std::vector<int64_t>* off, std::string* err);
// ds_format_values: n values comma-joined; the device form needs (VALUE_TEXT_MAX + 1) * n bytes at d_text and writes the
// byte count to *d_total
std::string format_values_host(const double* v, int64_t n);
hipError_t launch_format_values(const double* d_vals, int64_t n, char* d_text, int64_t* d_total, hipStream_t stream);

}  // namespace dsx
