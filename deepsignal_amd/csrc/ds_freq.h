// ds_freq.h — per-site modification frequency on the device (call_freq --on gpu; ds_freq.hip): the row grammar of a call_mods
// result file as the DEVICE reads it, the site key and its hash, and the host-side state of one run. The row routine is
// __host__ __device__ and built from the token routines of ds_tsv_device.h, so the CPU checker (dsf::reference, behind
// ds_freq_reference) runs the code freq_parse_kernel runs. Compiled with -ffp-contract=off and without fast-math (csrc/Makefile).
// A row in any form outside the grammar is not an error here: its status says ROW_HOST and the caller supplies its values.
// Not part of the public ABI.
#pragma once
#include "ds_tsv_device.h"

#include <string>

namespace dsf {

constexpr int ROW_OK = 0;          // parsed here
constexpr int ROW_HOST = 1;        // a form outside the device grammar: the caller's parser decides
constexpr int ROW_GIVEN = 2;       // dsf::reference only, on entry: the caller has supplied this row's values
constexpr int POS_BITS = 40;       // a site key is chrom_id << 40 | pos ...
constexpr int64_t POS_LIMIT = (int64_t)1 << POS_BITS;
constexpr int32_t CHROM_LIMIT = 1 << 23;         // ... with 23 bits of chromosome id, so no key is the empty slot's all-ones
constexpr uint64_t EMPTY = ~(uint64_t)0;
constexpr unsigned FLAG_HOST = 1;  // ds_freq_locate: the row is stripped or decoded differently by Python (leading / trailing whitespace, a
                                   // non-ASCII byte, a carriage return, a blank row)
constexpr int64_t MAX_TOTAL_ROWS = (int64_t)1 << 30;      // table slots and per-site counters are 31-bit

DST_HD uint64_t make_key(int32_t chrom, int64_t pos) { return ((uint64_t)(uint32_t)chrom << POS_BITS) | (uint64_t)pos; }
DST_HD bool key_ok(int32_t chrom, int64_t pos) { return chrom >= 0 && chrom < CHROM_LIMIT && pos >= 0 && pos < POS_LIMIT; }
// splitmix64's finalizer: neighbouring positions of one chromosome land in unrelated slots
DST_HD uint64_t hash_key(uint64_t k)
{
    k ^= k >> 30; k *= 0xbf58476d1ce4e5b9ull;
    k ^= k >> 27; k *= 0x94d049bb133111ebull;
    return k ^ (k >> 31);
}

// One row [b, e) of a call_mods result file: chrom \t pos \t strand \t pos_in_strand \t readname \t read_strand \t prob_0 \t prob_1 \t
// label \t k-mer [\t ...]. Columns 1, 3, 6, 7, 8 are parsed, column 9 must exist; column 0 has become `chrom` (ds_freq_locate).
// ROW_OK: what Python's int() / float() give for these tokens, bit for bit. ROW_HOST: anything else.
DST_HD int parse_row(const char* b, const char* e, int32_t chrom, unsigned flags, int64_t* pos, double* p0, double* p1, int32_t* met)
{
    if ((flags & FLAG_HOST) || chrom < 0 || chrom >= CHROM_LIMIT) return ROW_HOST;
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
    if (!dst::int64_token(cb[1], ce[1], &v) || v < 0 || v >= POS_LIMIT) return ROW_HOST;
    if (!dst::int64_token(cb[3], ce[3], &pis)) return ROW_HOST;      // read later from the site's first row: int() must take it
    if (!dst::double_token(cb[6], ce[6], p0) || !dst::double_token(cb[7], ce[7], p1)) return ROW_HOST;
    if (!dst::int_token(cb[8], ce[8], &label)) return ROW_HOST;
    *pos = v;
    *met = label == 1;
    return ROW_OK;
}

// a row is left out when |p0 - p1| < prob_cf, in double (a NaN difference keeps it, as in Python)
DST_HD bool row_used(double p0, double p1, double cf) { return !(fabs(p0 - p1) < cf); }

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

// ---- one run on the device ------------------------------------------------------------------------------------------------
// begin() sizes the table for total_rows (load <= 0.5) and the row buffers for batch_rows; parse() copies a batch's text and
// parses it; accumulate() applies the caller's values for ROW_HOST rows, inserts the used rows' keys, sorts (site, row) and
// adds each site's run in row order; result() compacts the occupied slots. Every call blocks; batches go strictly in sequence.
// Return codes are the DS_* of the public header; the message goes to *err.
struct Freq {
    int device = 0;
    hipStream_t s = nullptr;
    hipEvent_t ev[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
    int64_t total_rows = 0, rows_done = 0;
    int32_t batch_rows = 0, P = 0, pending = -1;      // P = batch_rows rounded up to a power of two; pending = rows parsed, not accumulated
    double cf = 0;
    uint64_t cap = 0;            // table slots, a power of two >= 2 * total_rows
    // table
    uint64_t *t_key = nullptr, *t_first = nullptr;
    double *t_sum0 = nullptr, *t_sum1 = nullptr;
    int32_t *t_met = nullptr, *t_unmet = nullptr;
    unsigned long long* counters = nullptr;       // [0] sites, [1] used rows, [2] probe sequences that found no slot, [3] ROW_HOST rows left
    // batch
    char* d_text = nullptr;
    size_t text_cap = 0;
    int64_t* d_off = nullptr;
    int32_t *d_len = nullptr, *d_chrom = nullptr, *d_status = nullptr, *d_met = nullptr;
    uint8_t* d_flags = nullptr;
    int64_t* d_pos = nullptr;
    double *d_p0 = nullptr, *d_p1 = nullptr;
    uint64_t* d_sort = nullptr;
    char* d_over = nullptr;      // the caller's values of a batch's ROW_HOST rows
    size_t over_cap = 0;
    int64_t batches = 0;
    double ms[4] = {0, 0, 0, 0};     // copies, freq_parse_kernel, the sort, insert + accumulate

    int begin(int device, int64_t total_rows, int32_t batch_rows, double prob_cf, std::string* err);
    int parse(const char* text, int32_t nrows, const int64_t* row_begin, const int64_t* row_end, const int32_t* chrom, const uint8_t* flags,
              int32_t* status, std::string* err);
    int accumulate(int32_t nover, const int32_t* row, const int32_t* chrom, const int64_t* pos, const double* p0, const double* p1,
                   const int32_t* met, std::string* err);
    int64_t result(int64_t cap_sites, int64_t* first_row, int32_t* chrom, int64_t* pos, double* sum0, double* sum1, int32_t* met,
                   int32_t* unmet, int64_t* rows, int64_t* used, std::string* err);
    void end();
    ~Freq() { end(); }
};

}  // namespace dsf
