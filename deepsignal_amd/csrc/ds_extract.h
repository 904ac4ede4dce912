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

}  // namespace dsx
