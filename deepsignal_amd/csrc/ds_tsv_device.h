// ds_tsv_device.h — the token grammar of the feature TSV as the DEVICE parses it (call_mods --parse_on gpu), shared by the gfx950
// kernel (ds_tsv_parse.hip) and the host checker ds_parse_text_reference: every token routine here is __host__ __device__, so
// what the CPU test compares against strtod is the code the kernel runs. The translation unit is compiled with
// -ffp-contract=off and without fast-math (csrc/Makefile): a token is ONE correctly rounded IEEE double multiplication or
// division followed by the narrowing to float32, which the GPU does bit for bit. A row whose form is anything else is not an
// error here: its status says ROW_HOST and the host parser (ds_io.cpp parse_row) takes it. Not part of the public ABI.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace dst {

#define DST_HD __host__ __device__ inline

constexpr int ROW_OK = 0;        // every token parsed on the device
constexpr int ROW_HOST = 1;      // a form outside the device grammar (or a row that was not staged): the host parser decides
constexpr int STEP = 1024;       // bytes of a row one wave looks at per step (64 lanes x 16 bytes); the staged text is padded by one
constexpr int LANE_BYTES = 16;

// numeric tokens of a row: means, stds, lens (kmer_len each), signals (signal_len), label
DST_HD int ntokens(int K, int S) { return 3 * K + S + 1; }

// A, C, G, T, N -> 0 .. 4 (process_utils.py:21), anything else -1
DST_HD int base_code(char c)
{
    switch (c) {
    case 'A': return 0; case 'C': return 1; case 'G': return 2; case 'T': return 3; case 'N': return 4;
    default: return -1;
    }
}

// [-]digits[.digits][e|E[+-]digits], the whole of [p, e): at most 15 significant digits m < 2^53 and a net decimal exponent in
// [-22, 22], so that m and 10^|x| are exact doubles and one multiplication or division gives the correctly rounded double
// strtod / float() return (Clinger's fast path). False: some other form (a leading '+', inf, nan, 1e400, a longer mantissa, an
// empty token, any other byte). double_token keeps the double (the probabilities of call_freq --on gpu, ds_freq.h); float_token
// narrows it to float32 (the feature TSV).
DST_HD bool double_token(const char* p, const char* e, double* out)
{
    const double kPow10[23] = {1e0, 1e1, 1e2, 1e3, 1e4, 1e5, 1e6, 1e7, 1e8, 1e9, 1e10, 1e11, 1e12, 1e13, 1e14, 1e15,
                               1e16, 1e17, 1e18, 1e19, 1e20, 1e21, 1e22};
    const char* q = p;
    const bool neg = q < e && *q == '-';
    if (neg) ++q;
    uint64_t m = 0;
    int nd = 0, frac = 0;
    bool any = false, dot = false;
    for (; q < e; ++q) {
        const unsigned c = (unsigned char)*q;
        if (c - '0' <= 9u) {
            any = true;
            if (nd == 0 && c == '0') { if (dot) ++frac; continue; }     // leading zeros carry no significance
            if (++nd > 15) return false;
            m = m * 10 + (c - '0');
            if (dot) ++frac;
        } else if (c == '.' && !dot) {
            dot = true;
        } else {
            break;
        }
    }
    if (!any) return false;
    int ex = 0;
    if (q < e && (*q == 'e' || *q == 'E')) {
        ++q;
        bool eneg = false;
        if (q < e && (*q == '+' || *q == '-')) { eneg = *q == '-'; ++q; }
        int ned = 0;
        for (; q < e && (unsigned)((unsigned char)*q - '0') <= 9u; ++q) {
            if (ex < 100000) ex = ex * 10 + (*q - '0');
            ++ned;
        }
        if (!ned) return false;
        if (eneg) ex = -ex;
    }
    if (q != e) return false;
    const int net = ex - frac;
    if (net < -22 || net > 22) return false;
    const double v = net < 0 ? (double)m / kPow10[-net] : (double)m * kPow10[net];
    *out = neg ? -v : v;
    return true;
}

DST_HD bool float_token(const char* p, const char* e, float* out)
{
    double v;
    if (!double_token(p, e, &v)) return false;
    *out = (float)v;
    return true;
}

// [-]digits, the whole of [p, e), at most 9 digits (lens, label)
DST_HD bool int_token(const char* p, const char* e, int* out)
{
    const char* q = p;
    const bool neg = q < e && *q == '-';
    if (neg) ++q;
    const int nd = (int)(e - q);
    if (nd < 1 || nd > 9) return false;
    int v = 0;
    for (; q < e; ++q) {
        const unsigned c = (unsigned char)*q;
        if (c - '0' > 9u) return false;
        v = v * 10 + (int)(c - '0');
    }
    *out = neg ? -v : v;
    return true;
}

// [-]digits, the whole of [p, e), at most 18 digits (genome positions)
DST_HD bool int64_token(const char* p, const char* e, int64_t* out)
{
    const char* q = p;
    const bool neg = q < e && *q == '-';
    if (neg) ++q;
    const int nd = (int)(e - q);
    if (nd < 1 || nd > 18) return false;
    int64_t v = 0;
    for (; q < e; ++q) {
        const unsigned c = (unsigned char)*q;
        if (c - '0' > 9u) return false;
        v = v * 10 + (int64_t)(c - '0');
    }
    *out = neg ? -v : v;
    return true;
}

// the label column tolerates trailing '\r' and spaces, as parse_row does
DST_HD bool label_token(const char* p, const char* e, int* out)
{
    while (e > p && (e[-1] == '\r' || e[-1] == ' ')) --e;
    return int_token(p, e, out);
}

// numeric token t of a row (ntokens order) in [p, e) -> its place in the row's arrays; false: host
DST_HD bool store_token(int t, int K, int S, const char* p, const char* e, float* means, float* stds, float* lens, float* signals,
                        int32_t* label)
{
    if (t < 2 * K) {
        float v;
        if (!float_token(p, e, &v)) return false;
        (t < K ? means[t] : stds[t - K]) = v;
    } else if (t < 3 * K) {
        int v;
        if (!int_token(p, e, &v)) return false;
        lens[t - 2 * K] = (float)v;          // the event lengths are integers stored as float
    } else if (t < 3 * K + S) {
        float v;
        if (!float_token(p, e, &v)) return false;
        signals[t - 3 * K] = v;
    } else {
        int v;
        if (!label_token(p, e, &v)) return false;
        *label = v;
    }
    return true;
}

// What the kernel gets: rows staged back to back (16-byte aligned starts) in `text`, padded by one STEP. Row i is
// text[off[i] .. off[i] + len[i]); len[i] < 0: the row was not staged (it did not fit the block) and its status is ROW_HOST.
// Outputs are the slot's forward inputs (row-major, row i of each) plus label, the byte length of columns 0..5 and the status.
struct ParseArgs {
    const char* text;
    const int64_t* off;
    const int32_t* len;
    int32_t* kmer;
    float *means, *stds, *lens, *signals;
    int32_t *label, *info_len, *status;
    int n, K, S;
};
// dynamic LDS of one wave: the token table, a few scalars and (when it fits) the row's text; 0 = the table alone does not fit
size_t parse_lds_bytes(int K, int S, int* text_bytes);
hipError_t launch_parse(const ParseArgs& a, hipStream_t stream);
// the same rows on the CPU, serially, from the token routines above. Rows are spans [begin[i], end[i]) of `text`.
void parse_reference(int K, int S, const char* text, int64_t nrows, const int64_t* begin, const int64_t* end, int32_t* kmer,
                     float* means, float* stds, float* lens, float* signals, int32_t* label, int32_t* info_len, int32_t* status);

}  // namespace dst

// the host reader's own row parser (ds_io.cpp parse_row) on one row: what a ROW_HOST row goes through. False: malformed.
namespace ds_io {
bool parse_row_host(int kmer_len, int signal_len, const char* b, const char* e, int32_t* kmer, float* means, float* stds, float* lens,
                    float* signals, int32_t* label, int64_t* info_len);
}
