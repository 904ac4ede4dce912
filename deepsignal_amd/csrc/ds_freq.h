// ds_freq.h — per-site modification frequency on the device (call_freq --on gpu; ds_freq.hip): the row grammar of a call_mods
// result file as the DEVICE reads it and the host-side state of one run on the site table (ds_site_table.h). The row routine is
// __host__ __device__ and built from the token routines of ds_tsv_device.h, so the CPU checker (dsf::reference, behind
// ds_freq_reference) runs the code freq_parse_kernel runs. Compiled with -ffp-contract=off and without fast-math (csrc/Makefile).
// A row in any form outside the grammar is not an error here: its status says ROW_HOST and the caller supplies its values.
// Not part of the public ABI.
#pragma once
#include "ds_site_table.h"

#include <string.h>

#include <string>

namespace dsf {

constexpr int ROW_OK = 0;          // parsed here
constexpr int ROW_HOST = 1;        // a form outside the device grammar: the caller's parser decides
constexpr int ROW_GIVEN = 2;       // dsf::reference only, on entry: the caller has supplied this row's values

// One row [b, e) of a call_mods result file: chrom \t pos \t strand \t pos_in_strand \t readname \t read_strand \t prob_0 \t prob_1 \t
// label \t k-mer [\t ...]. Columns 1, 3, 6, 7, 8 are parsed, column 9 must exist; column 0 has become `chrom` (ds_freq_locate).
// ROW_OK: what Python's int() / float() give for these tokens, bit for bit. ROW_HOST: anything else.
DST_HD int parse_row(const char* b, const char* e, int32_t chrom, unsigned flags, int64_t* pos, double* p0, double* p1, int32_t* met)
{
    if ((flags & dss::FLAG_HOST) || chrom < 0 || chrom >= dss::CHROM_LIMIT) return ROW_HOST;
    const char* cb[10];        // column c = [cb[c], ce[c])
    const char* ce[10];
    int nc = 0;
    cb[0] = b;
    for (const char* p = b; p < e && nc < 10; ++p)
        if (*p == '\t') {
            ce[nc++] = p;
            if (nc < 10) cb[nc] = p + 1;
        }
    if (nc < 10) ce[nc++] = e;     // the row end closes the last column
    if (nc < 10) return ROW_HOST;
    int64_t v, pis;
    int label;
    if (!dst::int64_token(cb[1], ce[1], &v) || v < 0 || v >= dss::POS_LIMIT) return ROW_HOST;
    if (!dst::int64_token(cb[3], ce[3], &pis)) return ROW_HOST;      // read later from the site's first row: int() must take it
    if (!dst::double_token(cb[6], ce[6], p0) || !dst::double_token(cb[7], ce[7], p1)) return ROW_HOST;
    if (!dst::int_token(cb[8], ce[8], &label)) return ROW_HOST;
    *pos = v;
    *met = label == 1;
    return ROW_OK;
}

// a row is left out when |p0 - p1| < prob_cf, in double (a NaN difference keeps it, as in Python)
DST_HD bool row_used(double p0, double p1, double cf) { return !(fabs(p0 - p1) < cf); }

// ---- a call's two probabilities without their text (call_mods --freq_file) -------------------------------------------------
// A result row holds str(np.float32(q)) -- the shortest decimal digits that read back as the float32 q -- and the frequency
// table sums float() of that text: the double nearest to the DECIMAL, not (double)q. decimal_value gives that double for
// 0 <= |q| <= 1 from integers alone. q = f * 2^e; with t decimal places the scaled value q * 10^t is 4f * 5^t / 2^S, S = 2 - e - t,
// and the float32 values that round to q span (4f - 1 or 2) * 5^t / 2^S .. (4f + 2) * 5^t / 2^S, ends excluded (an end is an odd
// multiple of a power of two below one: never a short decimal). The digits are the integer c at the smallest t for which c / 10^t
// lies in that span -- the floor or the ceiling of the scaled value, whichever lies inside, the nearer when both do, the even one
// on a tie: what Ryu (std::to_chars, format_f32 of ds_io.cpp) and numpy's Dragon4 print. Everything fits 128 bits: 4f < 2^26,
// 5^22 < 2^52, S <= 102. The double is then c / 10^t by dst::double_token's rule: both operands exact, one IEEE division.
// ROW_HOST: NaN, inf, |q| > 1, or digits that need more than 22 decimal places (|q| < ~1e-14 at nine digits; never above).
DST_HD int decimal_value(float q, double* out)
{
    const double kPow10[23] = {1e0, 1e1, 1e2, 1e3, 1e4, 1e5, 1e6, 1e7, 1e8, 1e9, 1e10, 1e11, 1e12, 1e13, 1e14, 1e15,
                               1e16, 1e17, 1e18, 1e19, 1e20, 1e21, 1e22};
    const uint64_t kPow5[23] = {1ull, 5ull, 25ull, 125ull, 625ull, 3125ull, 15625ull, 78125ull, 390625ull, 1953125ull, 9765625ull,
                                48828125ull, 244140625ull, 1220703125ull, 6103515625ull, 30517578125ull, 152587890625ull,
                                762939453125ull, 3814697265625ull, 19073486328125ull, 95367431640625ull, 476837158203125ull,
                                2384185791015625ull};
    uint32_t u;
    memcpy(&u, &q, 4);
    const bool neg = (u >> 31) != 0;
    const uint32_t be = (u >> 23) & 0xff, frac = u & 0x7fffff;
    if (be == 0xff) return ROW_HOST;                       // NaN, inf
    if (be == 0 && frac == 0) { *out = neg ? -0.0 : 0.0; return ROW_OK; }
    const uint32_t f = be ? (frac | 0x800000u) : frac;
    const int e = (be ? (int)be : 1) - 150;                // q = f * 2^e
    if (e > -23 || (e == -23 && f != 0x800000u)) return ROW_HOST;      // |q| > 1
    if (e < -100) return ROW_HOST;                         // |q| < 2^-76: below 1e-22, the smallest value of any digits at 22 places
    const unsigned __int128 v = (unsigned __int128)(4ull * f);
    const unsigned __int128 vp = v + 2, vm = v - ((frac == 0 && be > 1) ? 1 : 2);     // a power of two has the closer lower neighbour
    // c >= 1 needs 10^-t < 2^(e + 24) (1 + 2^-24): no digits before t = floor(-(e + 24) log10 2); 1233 / 4096 is just below log10 2
    for (int t = e < -24 ? ((-(e + 24)) * 1233) >> 12 : 0; t <= 22; ++t) {
        const int S = 2 - e - t;                           // 3 .. 102
        const unsigned __int128 p5 = (unsigned __int128)kPow5[t];
        const unsigned __int128 N = v * p5;
        const unsigned __int128 lo = N >> S;
        const bool lo_in = ((vm * p5) >> S) != lo;         // vm * 5^t < lo * 2^S
        const bool hi_in = ((vp * p5) >> S) != lo;         // (lo + 1) * 2^S < vp * 5^t
        if (!lo_in && !hi_in) continue;
        unsigned __int128 c = lo;
        if (hi_in) {
            if (!lo_in) {
                c = lo + 1;
            } else {
                const unsigned __int128 r = N - (lo << S), half = (unsigned __int128)1 << (S - 1);
                if (r > half || (r == half && (lo & 1))) c = lo + 1;
            }
        }
        if (c >= ((unsigned __int128)1 << 53)) return ROW_HOST;      // never: float32 needs at most nine digits
        const double d = (double)(uint64_t)c / kPow10[t];
        *out = neg ? -d : d;
        return ROW_OK;
    }
    return ROW_HOST;
}

// act row (a0, a1) of the forward -> the doubles call_freq reads from the row call_mods prints for it: the normalisation of
// ds_format_rows in float32, then decimal_value of each. ROW_HOST when either is outside it (the caller formats and parses the row).
DST_HD int call_value(float a0, float a1, double* p0, double* p1)
{
    const float s = a0 + a1;
    const float q0 = a0 / s, q1 = a1 / s;
    if (decimal_value(q0, p0) != ROW_OK) return ROW_HOST;
    return decimal_value(q1, p1);
}

// ---- the CPU checker ------------------------------------------------------------------------------------------------------
// Rows are spans [begin[i], end[i]) of `text`; chrom / flags per row as ds_freq_locate gives them. status (in / out): a row
// whose status is ROW_GIVEN on entry takes chrom[i] / pos[i] / p0[i] / p1[i] / met[i] from the caller (key_ok required); every
// other row is parsed by parse_row and its values and status are written. ROW_HOST rows take no part in the sums. Sites come
// out in the order of their first used row: first_row, site_chrom, site_pos, sum0 / sum1 (added in row order), met, unmet;
// *used = rows that passed the threshold. Returns the number of sites, or -1 with *err set (bad argument, cap too small).
int64_t reference(const char* text, int64_t nrows, const int64_t* begin, const int64_t* end, const int32_t* chrom, const uint8_t* flags,
                  double prob_cf, int32_t* status, int64_t* pos, double* p0, double* p1, int32_t* met, int64_t cap, int64_t* first_row,
                  int32_t* site_chrom, int64_t* site_pos, double* sum0, double* sum1, int32_t* site_met, int32_t* site_unmet,
                  int64_t* used, std::string* err);

// call_value over n act rows on the host, as freq_values_kernel runs it on the device (ds_freq_values_reference)
void values_reference(int64_t n, const float* act, int32_t class_num, double* p0, double* p1, int32_t* status);
// freq_values_kernel alone on `device` over n act rows: what the tests hold against values_reference (ds_freq_values)
int values_device(int device, int64_t n, const float* act, int32_t class_num, double* p0, double* p1, int32_t* status, std::string* err);

// ---- one run on the device ------------------------------------------------------------------------------------------------
// begin() sizes the table for total_rows (load <= 0.5) and the row buffers for batch_rows; parse() copies a batch's text and
// parses it; accumulate() applies the caller's values for ROW_HOST rows, inserts the used rows' keys, sorts (site, row) and
// adds each site's run in row order; result() compacts the occupied slots. Every call blocks; batches go strictly in sequence.
// A streaming run (begin_stream) takes push() in the place of parse(): keys, act rows and labels from the host, the values by
// freq_values_kernel, and before that a doubling of the table (grow) whenever 2 * (sites + rows of the batch) > slots.
// Return codes are the DS_* of the public header; the message goes to *err. Batches go strictly in sequence (dss::Batches). The
// handle holds a Freq from a begin() that succeeded to ds_freq_end: no call here asks whether a run is open.
struct Freq : dss::Batches {
    static constexpr const char* ROUTE = "ds_freq";
    struct Tally {
        dss::Times<4> batch;     // batches: copies, freq_parse_kernel, the sort, insert + accumulate
        dss::Times<2> stream;    // doublings of a streaming run's table: freq_values_kernel, the growths (freq_rehash_kernel and the new table's memsets)
        void add(const Tally& o) { batch.add(o.batch); stream.add(o.stream); }
    };
    dss::Run run;                // the stream, the events and every device allocation of the run
    double cf = 0;
    uint64_t cap = 0;            // table slots, a power of two >= 2 * total_rows
    // table
    uint64_t *t_key = nullptr, *t_first = nullptr;      // t_first: the site's first used row of the run
    double *t_sum0 = nullptr, *t_sum1 = nullptr;
    int32_t *t_met = nullptr, *t_unmet = nullptr;
    unsigned long long* counters = nullptr;       // [0] sites, [1] used rows, [2] probe sequences that found no slot, [3] ROW_HOST rows left
    // batch
    dss::RowText rows;
    int32_t* d_met = nullptr;
    int64_t* d_pos = nullptr;
    double *d_p0 = nullptr, *d_p1 = nullptr;
    uint64_t* d_sort = nullptr;
    dss::Buf over;               // the caller's values of a batch's ROW_HOST rows
    Tally t;

    // streaming (begin_stream / push): the number of rows is not known, the table doubles when a batch might fill it past one half
    bool streaming = false;
    int64_t sites = 0;           // sites in the table after the last accumulated batch
    dss::Buf act;                // a batch's act rows, float32
    int32_t *d_pred = nullptr, *d_opened = nullptr;
    int32_t* opened_out = nullptr;       // the caller's array of the pending push: filled when accumulate() completes it

    int begin(int device, int64_t total_rows, int32_t batch_rows, double prob_cf, std::string* err);
    int begin_stream(int device, int64_t initial_slots, int32_t batch_rows, double prob_cf, std::string* err);
    int push(int32_t nrows, const int32_t* chrom, const int64_t* pos, const float* act, int32_t class_num, const int32_t* pred,
             int32_t* status, int32_t* opened, std::string* err);
    int parse(const char* text, int32_t nrows, const int64_t* row_begin, const int64_t* row_end, const int32_t* chrom, const uint8_t* flags,
              int32_t* status, std::string* err);
    int accumulate(int32_t nover, const int32_t* row, const int32_t* chrom, const int64_t* pos, const double* p0, const double* p1,
                   const int32_t* met, std::string* err);
    int64_t result(int64_t cap_sites, int64_t* first_row, int32_t* chrom, int64_t* pos, double* sum0, double* sum1, int32_t* met,
                   int32_t* unmet, int64_t* rows, int64_t* used, std::string* err);
    void end();
    ~Freq() { end(); }

private:
    int open(int device, int32_t batch_rows, double prob_cf, std::string* err);
    int grow(int32_t nrows, std::string* err);
};

}  // namespace dsf
