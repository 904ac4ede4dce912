// ds_combine.h — both strands of a CpG table folded onto the '+' cytosine (combine_strands --on gpu; ds_combine.hip): the motif
// test of the genome scan, the row grammar of a frequency table / bedMethyl file as the DEVICE reads it, and the host-side state of
// one run. The routines are __host__ __device__ and built from the token routines of ds_tsv_device.h and the site key of ds_site_table.h,
// so the CPU checkers (dsc::motif_reference, dsc::reference, behind ds_motif_reference / ds_combine_reference) run the code the
// kernels run. Compiled with -ffp-contract=off and without fast-math (csrc/Makefile): the bed form's a / 100 * b and the sums after
// it are separate IEEE operations. A row in any form outside the grammar is not an error here: its status says ROW_HOST and the
// caller supplies its values. Not part of the public ABI.
#pragma once
#include "ds_site_table.h"

#include <vector>

namespace dsc {

constexpr int ROW_OK = 0;            // parsed here, its key is a CG of the genome
constexpr int ROW_HOST = 1;          // a form outside the device grammar: the caller's parser decides
constexpr int ROW_SKIP = 2;          // the key is no CG of the genome (unknown record, position outside it, bit clear)
constexpr int ROW_GIVEN = 3;         // dsc::reference only, on entry: the caller has supplied this row's values
constexpr int ROW_GIVEN_SKIP = 4;    // dsc::reference only, on entry: the caller has found this row's key to be no CG
constexpr int FORM_TABLE = 0;        // chrom pos strand pos_in_strand prob0 prob1 met unmet coverage Rmet k-mer
constexpr int FORM_BED = 1;          // chrom start end name score strand thickStart thickEnd rgb coverage percent
constexpr int64_t MAX_GENOME_BITS = (int64_t)1 << 46;      // one bit per base; more than this fits no device
constexpr int64_t MAX_CHUNK_BYTES = (int64_t)1 << 30;
constexpr int LANE_BYTES = 16;       // bytes of a genome chunk one lane of motif_bitmap_kernel looks at

// str.upper() on an ASCII byte
DST_HD unsigned upper(unsigned c) { return c - 'a' <= 25u ? c - 32u : c; }

// Byte j of a segment -- a piece of one stripped sequence line whose first base is base `seg_bit` of the bitmap; `carry` is the
// base in front of the segment in the same record, 0 when the segment opens its record. The bit to set is the C's, one base
// upstream of a G; -1: none. The caller checks 0 <= bit < bits of the bitmap.
DST_HD int64_t motif_bit(const unsigned char* seg, int64_t j, unsigned carry, int64_t seg_bit)
{
    const unsigned prev = j > 0 ? seg[j - 1] : carry;
    return upper(prev) == 'C' && upper(seg[j]) == 'G' ? seg_bit + j - 1 : -1;
}

DST_HD bool bit_set(const uint32_t* bitmap, int64_t bit) { return ((bitmap[bit >> 5] >> (bit & 31)) & 1u) != 0; }

struct Row {
    int64_t pos;         // the key's position: pos - 1 for a '-' row
    int32_t plus;        // not a '-' row
    double a, b;         // table: prob0, prob1. bed: met = percent / 100 * coverage, 0.0
    int64_t c0, c1, c2;  // table: met, unmet, coverage. bed: 0, 0, coverage
};

// One row [b, e) of the input in the order the reference script reads it: the position ([-]digits) and the strand column (table: 2,
// bed: 5; '-' iff that one byte), then the key test -- ROW_SKIP before any number is looked at --, then the numbers (double_token;
// counts of at most nine digits, exact as doubles). A '+' row of the table needs its k-mer column, 10. `chrom` is the row's record of
// the genome, -1 when column 0 names none. ROW_OK: what Python's int() / float() give for these tokens, bit for bit.
DST_HD int parse_row(int form, const char* b, const char* e, int32_t chrom, unsigned flags, int32_t nrec, const int64_t* rec_base,
                     const int64_t* rec_len, const uint32_t* bitmap, Row* r)
{
    if ((flags & dss::FLAG_HOST) || chrom >= nrec) return ROW_HOST;
    const char* cb[11];        // column c = [cb[c], ce[c])
    const char* ce[11];
    int nc = 0;
    cb[0] = b;
    for (const char* p = b; p < e && nc < 11; ++p)
        if (*p == '\t') {
            ce[nc++] = p;
            if (nc < 11) cb[nc] = p + 1;
        }
    if (nc < 11) ce[nc++] = e;     // the row end closes the last column
    const int sc = form == FORM_BED ? 5 : 2;
    if (nc <= sc) return ROW_HOST;
    int64_t v;
    if (!dst::int64_token(cb[1], ce[1], &v)) return ROW_HOST;
    const bool minus = ce[sc] - cb[sc] == 1 && *cb[sc] == '-';
    const int64_t p = v - (minus ? 1 : 0);
    if (chrom < 0 || p < 0 || p >= rec_len[chrom] || !bit_set(bitmap, rec_base[chrom] + p)) return ROW_SKIP;
    r->pos = p;
    r->plus = minus ? 0 : 1;
    if (form == FORM_BED) {
        int cov;
        double pct;
        if (nc < 11 || !dst::int_token(cb[9], ce[9], &cov) || !dst::double_token(cb[10], ce[10], &pct)) return ROW_HOST;
        r->a = pct / 100.0 * (double)cov;
        r->b = 0.0;
        r->c0 = r->c1 = 0;
        r->c2 = cov;
        return ROW_OK;
    }
    if (nc < (minus ? 9 : 11)) return ROW_HOST;
    int m, u, c;
    if (!dst::double_token(cb[4], ce[4], &r->a) || !dst::double_token(cb[5], ce[5], &r->b)) return ROW_HOST;
    if (!dst::int_token(cb[6], ce[6], &m) || !dst::int_token(cb[7], ce[7], &u) || !dst::int_token(cb[8], ce[8], &c)) return ROW_HOST;
    r->c0 = m; r->c1 = u; r->c2 = c;
    return ROW_OK;
}

// the values a caller may give for a row: a count below 2^32 in magnitude keeps every 64-bit sum of 2^30 rows exact
constexpr int64_t COUNT_LIMIT = (int64_t)1 << 32;
inline bool count_ok(int64_t v) { return v > -COUNT_LIMIT && v < COUNT_LIMIT; }

// ---- the CPU checkers -----------------------------------------------------------------------------------------------------
// The genome scan over the segments of one buffer, serially: ORs the motif bits into `bitmap` (nbits bits, the caller zeroes it
// before the first call). Segments are [seg_begin[i], seg_end[i]) of `text`, ascending and disjoint. False: bad argument.
bool motif_reference(const char* text, int64_t nseg, const int64_t* seg_begin, const int64_t* seg_end, const int64_t* seg_bit,
                     const uint8_t* seg_carry, int64_t nbits, uint32_t* bitmap, std::string* err);

// Rows are spans [begin[i], end[i]) of `text`; chrom = the record of the genome per row (-1: none), flags as ds_freq_locate gives
// them. status (in / out): ROW_GIVEN on entry takes chrom[i] / pos[i] / plus[i] / a[i] / b[i] / c0[i] / c1[i] / c2[i] from the
// caller, ROW_GIVEN_SKIP becomes ROW_SKIP, every other row is parsed by parse_row. Sites come out in the order of their first row:
// record, position, the two double sums (added in row order from 0.0), the three count sums, and the greatest row that is a '+' row
// (-1: none). cap == 0: the rows' statuses and values alone. Returns the number of sites, or -1 with *err set.
int64_t reference(int form, const char* text, int64_t nrows, const int64_t* begin, const int64_t* end, int32_t* chrom, const uint8_t* flags,
                  int32_t nrec, const int64_t* rec_len, const uint32_t* bitmap, int32_t* status, int64_t* pos, int32_t* plus, double* a,
                  double* b, int64_t* c0, int64_t* c1, int64_t* c2, int64_t cap, int32_t* site_chrom, int64_t* site_pos, double* sum0,
                  double* sum1, int64_t* met, int64_t* unmet, int64_t* cov, int64_t* last_plus, std::string* err);

// ---- one run on the device ------------------------------------------------------------------------------------------------
// begin() takes the surviving records' lengths (bit record_base + i of the bitmap is base i of a record; records lie back to back,
// so two may share a word), sizes the site table for total_rows (load <= 0.5) and the row buffers for batch_rows. genome() copies one
// chunk of FASTA bytes and ORs its motif bits in; the bytes do not stay. parse() copies a batch's text and parses it; accumulate()
// applies the caller's values for ROW_HOST rows, inserts the ROW_OK rows' keys, sorts (site, row) and adds each site's run in row
// order; result() compacts the occupied slots. Every call blocks; batches go strictly in sequence (dss::Batches), after the last
// genome chunk. The handle holds a Combine from a begin() that succeeded to ds_combine_end: no call here asks whether a run is open.
struct Combine : dss::Batches {
    static constexpr const char* ROUTE = "ds_combine";
    typedef dss::Times<5, 2> Tally;      // n: batches, genome chunks; ms: copies, motif_bitmap_kernel, combine_parse_kernel, the sort, insert + accumulate
    int form = FORM_TABLE;
    dss::Run run;                // the stream, the events and every device allocation of the run
    int64_t nbits = 0;
    int32_t nrec = 0;
    bool rows_begun = false;
    std::vector<int64_t> h_len;
    uint64_t cap = 0;            // table slots, a power of two >= 2 * total_rows
    // genome
    uint32_t* bitmap = nullptr;
    int64_t *d_rec_base = nullptr, *d_rec_len = nullptr;
    dss::Buf seg;                // a chunk's [seg_off | seg_end | seg_bit | seg_carry]
    // table
    uint64_t *t_key = nullptr, *t_plus = nullptr;      // t_plus: the greatest '+' row of the site + 1, 0 = none
    double *t_sum0 = nullptr, *t_sum1 = nullptr;
    int64_t *t_met = nullptr, *t_unmet = nullptr, *t_cov = nullptr;
    unsigned long long* counters = nullptr;       // [0] sites, [1] rows added, [2] probe sequences that found no slot, [3] ROW_HOST rows left
    // batch
    dss::RowText rows;
    int32_t* d_plus = nullptr;
    int64_t *d_pos = nullptr, *d_c0 = nullptr, *d_c1 = nullptr, *d_c2 = nullptr;
    double *d_a = nullptr, *d_b = nullptr;
    uint64_t* d_sort = nullptr;
    dss::Buf over;               // the caller's word on a batch's ROW_HOST rows
    Tally t;

    int begin(int device, int form, int32_t nrec, const int64_t* rec_len, int64_t total_rows, int32_t batch_rows, std::string* err);
    int genome(const char* text, int64_t nseg, const int64_t* seg_begin, const int64_t* seg_end, const int64_t* seg_bit,
               const uint8_t* seg_carry, std::string* err);
    int get_bitmap(int64_t cap_words, uint32_t* out, std::string* err);
    int parse(const char* text, int32_t nrows, const int64_t* row_begin, const int64_t* row_end, const int32_t* chrom, const uint8_t* flags,
              int32_t* status, std::string* err);
    int accumulate(int32_t nover, const int32_t* row, const int32_t* ostatus, const int32_t* chrom, const int64_t* pos, const int32_t* plus,
                   const double* a, const double* b, const int64_t* c0, const int64_t* c1, const int64_t* c2, std::string* err);
    int64_t result(int64_t cap_sites, int32_t* chrom, int64_t* pos, double* sum0, double* sum1, int64_t* met, int64_t* unmet, int64_t* cov,
                   int64_t* last_plus, int64_t* rows, std::string* err);
    void end();
    ~Combine() { end(); }
};

}  // namespace dsc
