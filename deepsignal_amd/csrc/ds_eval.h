// ds_eval.h — call accuracy and AUROC of labelled call_mods result rows on the device (evaluate --on gpu; ds_eval.hip): the row
// grammar as the DEVICE reads it, the order-preserving key of a score, the per-row predicates of the counters, and the host-side
// state of one run on the site table (ds_site_table.h). The row routines are __host__ __device__ and built from the token routines
// of ds_tsv_device.h, so the CPU checker (dse::reference, behind ds_eval_reference) runs the code the kernels run. Every sum of this
// route is an integer: nothing depends on an order of addition. Compiled with -ffp-contract=off and without fast-math
// (csrc/Makefile). A row in any form outside the grammar is not an error here: its status says ROW_HOST and the caller supplies
// its values. Not part of the public ABI.
#pragma once
#include "ds_site_table.h"

#include <string.h>

#include <string>
#include <vector>

namespace dse {

constexpr int ROW_OK = 0;          // parsed here
constexpr int ROW_HOST = 1;        // a form outside the device grammar: the caller's parser decides
constexpr int ROW_GIVEN = 2;       // dse::reference only, on entry: the caller has supplied this row's values

constexpr int MAX_CF = 32;         // cut-offs of a run
constexpr int NSETS = 2;           // tested sets: 0 the sample, 1 all rows
constexpr unsigned SET_BITS = 3;   // a row's byte: bit s = the row is in set s ...
constexpr unsigned TRUTH_BIT = 4;  // ... bit 2 = it comes from the methylated file
// a set's counters: tp, fp, tn, fn, called[MAX_CF], correct[MAX_CF]
constexpr int C_TP = 0, C_FP = 1, C_TN = 2, C_FN = 3, C_CALLED = 4, C_CORRECT = 4 + MAX_CF, SET_COUNTERS = 4 + 2 * MAX_CF;

DST_HD bool is_blank(char c) { return c == ' ' || c == '\t'; }

// One row [b, e) of a call_mods result file as str.split() cuts it: fields separated by runs of space or tab, blanks in front and
// behind are plain. Fields 1, 3, 6, 7, 8 are parsed (int(), int(), float(), float(), int() of the script's ModRecord), field 9 must
// exist. ROW_OK: what Python gives for these tokens, bit for bit; *called = a non-zero label. ROW_HOST: anything else.
DST_HD int parse_row(const char* b, const char* e, unsigned flags, double* p0, double* p1, int32_t* called)
{
    if (flags & dss::FLAG_HOST) return ROW_HOST;
    const char* fb[10];        // field c = [fb[c], fe[c])
    const char* fe[10];
    int nf = 0;
    const char* p = b;
    while (nf < 10) {
        while (p < e && is_blank(*p)) ++p;
        if (p >= e) break;
        fb[nf] = p;
        while (p < e && !is_blank(*p)) ++p;
        fe[nf++] = p;
    }
    if (nf < 10) return ROW_HOST;
    int64_t pos, pis;
    int label;
    if (!dst::int64_token(fb[1], fe[1], &pos) || !dst::int64_token(fb[3], fe[3], &pis)) return ROW_HOST;
    if (!dst::double_token(fb[6], fe[6], p0) || !dst::double_token(fb[7], fe[7], p1)) return ROW_HOST;
    if (!dst::int_token(fb[8], fe[8], &label)) return ROW_HOST;
    *called = label != 0;
    return ROW_OK;
}

// the script's two comparisons at cut-off cf, in double: a NaN difference stands at no cut-off
DST_HD bool row_stands(double p0, double p1, double cf) { return fabs(p1 - p0) >= cf; }
DST_HD bool row_correct(double p0, double p1, double cf, bool truth) { return (p1 - p0 >= cf) == truth; }

DST_HD bool score_finite(double v)
{
    uint64_t u;
    memcpy(&u, &v, 8);
    return ((u >> 52) & 0x7ff) != 0x7ff;
}

// The key of a finite score: its 64 bits with the sign folded so that unsigned order is numeric order, -0.0 as +0.0. The images of
// the finite doubles end below that of +inf (0xfff0...), so neither dss::EMPTY nor dss::SORT_PAD (all ones, a NaN's image) is one.
DST_HD uint64_t score_key(double v)
{
    if (v == 0.0) v = 0.0;
    uint64_t u;
    memcpy(&u, &v, 8);
    return (u >> 63) ? ~u : (u | ((uint64_t)1 << 63));
}

// a slot's four counts: [0] sample positives, [1] sample negatives, [2] all positives, [3] all negatives
DST_HD int count_index(int set, bool truth) { return 2 * set + (truth ? 0 : 1); }

// ---- the multi-level scan of the result -----------------------------------------------------------------------------------
constexpr int SCAN_SPAN = dss::TPB;       // elements one workgroup scans: a level shrinks the problem by this factor
// the block sums of every level of a scan over n elements, back to back
inline size_t scan_scratch(size_t n)
{
    size_t total = 0;
    while (n > 1) { n = (n + SCAN_SPAN - 1) / SCAN_SPAN; total += n; }
    return total + 1;
}

// ---- the CPU checker ------------------------------------------------------------------------------------------------------
// Rows are spans [begin[i], end[i]) of `text`; flags per row as ds_eval_locate gives them; mask per row (SET_BITS | TRUTH_BIT).
// status (in / out): a row whose status is ROW_GIVEN on entry takes p0[i] / p1[i] / called[i] from the caller; every other row is
// parsed by parse_row and its values and status are written. ROW_HOST rows take no part. counts: NSETS x (4 + 2 * ncf) as
// ds_eval_result lays them out; u2 / pn / nn per set over the rows with a finite prob_1. False with *err set: a bad argument.
bool reference(const char* text, int64_t nrows, const int64_t* begin, const int64_t* end, const uint8_t* flags, const uint8_t* mask,
               int32_t ncf, const double* cf, int32_t* status, double* p0, double* p1, int32_t* called, int64_t* counts, uint64_t* u2,
               int64_t* pn, int64_t* nn, std::string* err);

// ---- one run on the device ------------------------------------------------------------------------------------------------
// begin() sizes the table for total_rows (load <= 0.5) and the row buffers for batch_rows; parse() copies a batch's text and parses
// it; accumulate() applies the caller's values for ROW_HOST rows, counts, and adds the rows' scores to the table; result() sorts the
// distinct scores, scans the negatives below each and reduces U2. Every call blocks; batches go strictly in sequence (dss::Batches).
// The handle holds an Eval from a begin() that succeeded to ds_eval_end: no call here asks whether a run is open.
struct Eval : dss::Batches {
    static constexpr const char* ROUTE = "ds_eval";
    typedef dss::Times<4> Tally;     // copies, eval_parse_kernel, eval_count_kernel + eval_insert_kernel, the result (sort, scan, reduce)
    dss::Run run;
    int32_t ncf = 0;
    uint64_t cap = 0;            // table slots, a power of two >= 2 * total_rows
    uint64_t* t_key = nullptr;
    uint32_t* t_cnt = nullptr;   // four counts per slot (count_index)
    unsigned long long* counters = nullptr;       // [0] distinct scores, [1] rows in the table, [2] probes that found no slot, [3] ROW_HOST rows
                                                  // left, [4] U2 / P / N per set (result), [16] the sets' counters
    double* d_cf = nullptr;
    dss::RowText rows;
    std::vector<int32_t> zeros;  // RowText carries a chromosome per row; these rows name none
    uint8_t* d_mask = nullptr;
    int32_t* d_called = nullptr;
    double *d_p0 = nullptr, *d_p1 = nullptr;
    dss::Buf over, res;          // the caller's values of a batch's ROW_HOST rows; the result's sorted keys, counts, scans
    Tally t;

    int begin(int device, int64_t total_rows, int32_t batch_rows, int32_t ncf, const double* cf, std::string* err);
    int parse(const char* text, int32_t nrows, const int64_t* row_begin, const int64_t* row_end, const uint8_t* flags, int32_t* status,
              std::string* err);
    int accumulate(const uint8_t* mask, int32_t nover, const int32_t* row, const double* p0, const double* p1, const int32_t* called,
                   std::string* err);
    int result(int64_t* counts, uint64_t* u2, int64_t* pn, int64_t* nn, int64_t* rows, int64_t* distinct, std::string* err);
    void end();
    ~Eval() { end(); }
};

constexpr int COUNTERS_U2 = 4, COUNTERS_SETS = 16, COUNTERS_TOTAL = COUNTERS_SETS + NSETS * SET_COUNTERS;

}  // namespace dse
