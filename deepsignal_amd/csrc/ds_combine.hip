// ds_combine.hip — both strands of a CpG table folded onto the '+' cytosine, on the GPU (combine_strands --on gpu). The genome comes
// first, in chunks of FASTA bytes: motif_bitmap_kernel sets bit record_base + i of a bitmap iff base i of a record is C and base
// i + 1 of the same record is G (ds_combine.h motif_bit; the base in front of a segment is carried in by the host, so the motif is
// found across line breaks and chunk boundaries and never across two records; the C's bit may lie in a word another lane or chunk
// also writes: 32-bit atomicOr). One bit per base stays, the bytes do not. Then the rows, a batch at a time: combine_parse_kernel
// (one row per lane; the key test against the bitmap comes before the numbers, as in the script), combine_insert_kernel (the exact
// keys record << 40 | pos into the site table of ds_site_table.h; the greatest '+' row of a site by atomicMax), the bitonic sort of
// site << 32 | row and combine_accumulate_kernel (the lane at the head of a site's run adds the run IN ROW ORDER: no floating-point
// atomics). Built with -ffp-contract=off and no fast-math (csrc/Makefile).
#include "ds_combine.h"

#include <unordered_map>

namespace dsc {

namespace {

using dss::TPB;
using dss::blocks;
using dss::seterr;
using dss::u64;
using dss::ull;

// lane t looks at bytes [t * LANE_BYTES, (t + 1) * LANE_BYTES) of the chunk: the segment of its first byte by bisection, the next
// ones by walking on. Bytes outside every segment (line ends, what strip() removes, header lines) are passed over.
__global__ __launch_bounds__(TPB) void motif_bitmap_kernel(const unsigned char* text, long long nbytes, const long long* seg_off,
                                                           const long long* seg_end, const long long* seg_bit, const uint8_t* seg_carry,
                                                           int nseg, unsigned int* bitmap, long long nbits)
{
    const long long t = (long long)blockIdx.x * TPB + threadIdx.x;
    const long long p0 = t * LANE_BYTES;
    if (p0 >= nbytes || nseg < 1) return;
    const long long p1 = p0 + LANE_BYTES < nbytes ? p0 + LANE_BYTES : nbytes;
    int lo = 0, hi = nseg;           // the first segment that begins behind p0
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (seg_off[mid] <= p0) lo = mid + 1; else hi = mid;
    }
    int s = lo > 0 ? lo - 1 : 0;
    for (long long p = p0; p < p1; ++p) {
        while (s + 1 < nseg && seg_off[s + 1] <= p) ++s;
        const long long so = seg_off[s];
        if (p < so || p >= seg_end[s]) continue;
        const long long bit = motif_bit(text + so, p - so, seg_carry[s], seg_bit[s]);
        if (bit >= 0 && bit < nbits) atomicOr(&bitmap[bit >> 5], 1u << (bit & 31));
    }
}

struct RowArrays {
    int32_t *chrom, *plus, *status;
    int64_t *pos, *c0, *c1, *c2;
    double *a, *b;
};

__global__ __launch_bounds__(TPB) void combine_parse_kernel(int form, const char* text, const int64_t* off, const int32_t* len, const uint8_t* flags,
                                                            int n, int32_t nrec, const int64_t* rec_base, const int64_t* rec_len,
                                                            const uint32_t* bitmap, RowArrays r)
{
    const int i = blockIdx.x * TPB + threadIdx.x;
    if (i >= n) return;
    const char* b = text + off[i];
    Row v = {0, 0, 0.0, 0.0, 0, 0, 0};
    const int st = parse_row(form, b, b + len[i], r.chrom[i], flags[i], nrec, rec_base, rec_len, bitmap, &v);
    r.pos[i] = v.pos; r.plus[i] = v.plus; r.a[i] = v.a; r.b[i] = v.b; r.c0[i] = v.c0; r.c1[i] = v.c1; r.c2[i] = v.c2;
    r.status[i] = st;
}

// the caller's word on the rows the device left to it: values (ROW_OK) or "no CG of the genome" (ROW_SKIP)
__global__ __launch_bounds__(TPB) void combine_override_kernel(int m, const int32_t* row, const int32_t* ostatus, RowArrays o, RowArrays r)
{
    const int k = blockIdx.x * TPB + threadIdx.x;
    if (k >= m) return;
    const int i = row[k];
    r.chrom[i] = o.chrom[k]; r.pos[i] = o.pos[k]; r.plus[i] = o.plus[k]; r.a[i] = o.a[k]; r.b[i] = o.b[k];
    r.c0[i] = o.c0[k]; r.c1[i] = o.c1[k]; r.c2[i] = o.c2[k];
    r.status[i] = ostatus[k];
}

__global__ __launch_bounds__(TPB) void combine_insert_kernel(int n, int P, ull row_base, const int32_t* chrom, const int64_t* pos, const int32_t* plus,
                                                             const int32_t* status, ull* t_key, ull* t_plus, ull mask, ull* sort, ull* counters)
{
    const int i = blockIdx.x * TPB + threadIdx.x;
    if (i >= P) return;
    ull sk = dss::SORT_PAD;
    if (i < n && status[i] != ROW_SKIP) {
        if (status[i] != ROW_OK || !dss::key_ok(chrom[i], pos[i])) {
            atomicAdd(&counters[3], 1ull);
        } else {
            const ull s = dss::insert_row(t_key, mask, dss::make_key(chrom[i], pos[i]), i, counters, &sk);
            if (s != dss::NO_SLOT && plus[i]) atomicMax(&t_plus[s], row_base + (ull)i + 1ull);
        }
    }
    sort[i] = sk;
}

__global__ __launch_bounds__(TPB) void combine_accumulate_kernel(int P, const ull* sorted, const double* a, const double* b, const int64_t* c0,
                                                                 const int64_t* c1, const int64_t* c2, double* t_sum0, double* t_sum1, int64_t* t_met,
                                                                 int64_t* t_unmet, int64_t* t_cov)
{
    const int t = blockIdx.x * TPB + threadIdx.x;
    ull site;
    if (!dss::run_head(sorted, P, t, &site)) return;
    double x = t_sum0[site], y = t_sum1[site];
    int64_t m = t_met[site], u = t_unmet[site], c = t_cov[site];
    dss::walk_run(sorted, P, t, site, [&](unsigned i) {
        x += a[i];
        y += b[i];
        m += c0[i]; u += c1[i]; c += c2[i];
    });
    t_sum0[site] = x; t_sum1[site] = y; t_met[site] = m; t_unmet[site] = u; t_cov[site] = c;
}

__global__ __launch_bounds__(TPB) void combine_result_kernel(ull cap, const ull* t_key, const ull* t_plus, const double* t_sum0, const double* t_sum1,
                                                             const int64_t* t_met, const int64_t* t_unmet, const int64_t* t_cov, ull* cursor, ull out_cap,
                                                             int32_t* chrom, int64_t* pos, double* sum0, double* sum1, int64_t* met, int64_t* unmet,
                                                             int64_t* cov, int64_t* last_plus)
{
    const ull s = (ull)blockIdx.x * TPB + threadIdx.x;
    ull o;
    if (!dss::compact_slot(cap, t_key, s, cursor, out_cap, chrom, pos, &o)) return;
    sum0[o] = t_sum0[s]; sum1[o] = t_sum1[s]; met[o] = t_met[s]; unmet[o] = t_unmet[s]; cov[o] = t_cov[s];
    last_plus[o] = (int64_t)t_plus[s] - 1;
}

// ascending, disjoint, inside [0, limit) and landing inside the bitmap; a carried base needs a base in front of it
bool segments_ok(int64_t nseg, const int64_t* sb, const int64_t* se, const int64_t* bit, const uint8_t* carry, int64_t nbits, std::string* err)
{
    for (int64_t i = 0; i < nseg; ++i) {
        const bool bad = sb[i] < 0 || se[i] <= sb[i] || (i > 0 && sb[i] < se[i - 1]) || bit[i] < 0 || bit[i] > nbits || se[i] - sb[i] > nbits - bit[i] ||
                         (carry[i] != 0 && bit[i] < 1);
        if (bad) {
            seterr(err, -1, "segment " + std::to_string(i) + " is empty, out of order or outside the bitmap");
            return false;
        }
    }
    return true;
}

}  // namespace

int Combine::begin(int dev, int fm, int32_t nr, const int64_t* rec_len, int64_t total, int32_t batch, std::string* err)
{
    if (fm != FORM_TABLE && fm != FORM_BED) return seterr(err, DS_ERR_INVALID, "ds_combine_begin: form must be DS_COMBINE_TABLE or DS_COMBINE_BED");
    if (nr < 1 || nr > dss::CHROM_LIMIT || !rec_len) return seterr(err, DS_ERR_INVALID, "ds_combine_begin: 1 .. 2^23 records");
    const int rc = sizes(ROUTE, 0, total, batch, err);
    if (rc) return rc;
    std::vector<int64_t> base((size_t)nr);
    int64_t bits = 0;
    for (int32_t i = 0; i < nr; ++i) {
        if (rec_len[i] < 0 || rec_len[i] > dss::POS_LIMIT) return seterr(err, DS_ERR_INVALID, "ds_combine_begin: a record's length must be in [0, 2^40]");
        base[(size_t)i] = bits;
        bits += rec_len[i];
        if (bits > MAX_GENOME_BITS) return seterr(err, DS_ERR_NOMEM, "ds_combine_begin: a genome of more than 2^46 bases");
    }
    form = fm; nrec = nr; nbits = bits;
    h_len.assign(rec_len, rec_len + nr);
    cap = 64;
    while (cap < 2 * (uint64_t)total) cap <<= 1;
    size_t P = 1;                 // the sort's keys: batch_rows rounded up to a power of two
    while (P < (size_t)batch) P <<= 1;
    const size_t words = (size_t)((bits + 31) >> 5) + 1;
    const size_t B = (size_t)batch;
    DSS_TRY(run.open(dev));
    hipStream_t s = run.s;
    DSS_TRY(run.alloc(&bitmap, words * 4, 0));
    DSS_TRY(run.alloc(&d_rec_base, (size_t)nr * 8));
    DSS_TRY(run.alloc(&d_rec_len, (size_t)nr * 8));
    DSS_TRY(run.alloc(&t_key, cap * 8, 0xff));
    DSS_TRY(run.alloc(&t_plus, cap * 8, 0));
    DSS_TRY(run.alloc(&t_sum0, cap * 8, 0));
    DSS_TRY(run.alloc(&t_sum1, cap * 8, 0));
    DSS_TRY(run.alloc(&t_met, cap * 8, 0));
    DSS_TRY(run.alloc(&t_unmet, cap * 8, 0));
    DSS_TRY(run.alloc(&t_cov, cap * 8, 0));
    DSS_TRY(run.alloc(&counters, 8 * 8, 0));
    DSS_TRY(rows.alloc(&run, B));
    DSS_TRY(run.alloc(&d_plus, B * 4));
    DSS_TRY(run.alloc(&d_pos, B * 8));
    DSS_TRY(run.alloc(&d_c0, B * 8));
    DSS_TRY(run.alloc(&d_c1, B * 8));
    DSS_TRY(run.alloc(&d_c2, B * 8));
    DSS_TRY(run.alloc(&d_a, B * 8));
    DSS_TRY(run.alloc(&d_b, B * 8));
    DSS_TRY(run.alloc(&d_sort, P * 8));
    DSS_TRY(hipMemcpyAsync(d_rec_base, base.data(), (size_t)nr * 8, hipMemcpyHostToDevice, s));
    DSS_TRY(hipMemcpyAsync(d_rec_len, h_len.data(), (size_t)nr * 8, hipMemcpyHostToDevice, s));
    DSS_TRY(hipStreamSynchronize(s));      // also: `base` may go away now
    return DS_OK;
}

int Combine::genome(const char* text, int64_t nseg, const int64_t* sb, const int64_t* se, const int64_t* bit, const uint8_t* carry, std::string* err)
{
    if (rows_begun) return seterr(err, DS_ERR_INVALID, "ds_combine_genome: the rows have begun; the genome comes first");
    if (!text || !sb || !se || !bit || !carry) return seterr(err, DS_ERR_INVALID, "ds_combine_genome: null argument");
    if (nseg < 1 || nseg > 0x7fffffff) return seterr(err, DS_ERR_INVALID, "ds_combine_genome: 1 .. 2^31 - 1 segments in a chunk");
    std::string why;
    if (!segments_ok(nseg, sb, se, bit, carry, nbits, &why)) return seterr(err, DS_ERR_INVALID, "ds_combine_genome: " + why);
    const int64_t base = sb[0];
    const int64_t bytes = se[nseg - 1] - base;
    if (bytes > MAX_CHUNK_BYTES) return seterr(err, DS_ERR_INVALID, "ds_combine_genome: a chunk spans at most 2^30 bytes");
    const size_t N = (size_t)nseg;
    std::vector<int64_t> off(N), end(N);
    for (size_t i = 0; i < N; ++i) { off[i] = sb[i] - base; end[i] = se[i] - base; }
    hipStream_t s = run.s;
    DSS_TRY(hipSetDevice(run.device));
    DSS_TRY(rows.text.grow(&run, (size_t)bytes));
    DSS_TRY(seg.grow(&run, N * 25));
    long long* g_off = reinterpret_cast<long long*>(seg.p);
    long long* g_end = g_off + N;
    long long* g_bit = g_end + N;
    uint8_t* g_carry = reinterpret_cast<uint8_t*>(g_bit + N);
    DSS_TRY(hipEventRecord(run.ev[0], s));
    DSS_TRY(hipMemcpyAsync(rows.text.p, text + base, (size_t)bytes, hipMemcpyHostToDevice, s));
    DSS_TRY(hipMemcpyAsync(g_off, off.data(), N * 8, hipMemcpyHostToDevice, s));
    DSS_TRY(hipMemcpyAsync(g_end, end.data(), N * 8, hipMemcpyHostToDevice, s));
    DSS_TRY(hipMemcpyAsync(g_bit, bit, N * 8, hipMemcpyHostToDevice, s));
    DSS_TRY(hipMemcpyAsync(g_carry, carry, N, hipMemcpyHostToDevice, s));
    DSS_TRY(hipEventRecord(run.ev[1], s));
    const uint64_t lanes = ((uint64_t)bytes + LANE_BYTES - 1) / LANE_BYTES;
    hipLaunchKernelGGL(motif_bitmap_kernel, dim3(blocks(lanes)), dim3(TPB), 0, s, reinterpret_cast<const unsigned char*>(rows.text.p), (long long)bytes,
                       g_off, g_end, g_bit, g_carry, (int)nseg, bitmap, (long long)nbits);
    DSS_TRY(hipGetLastError());
    DSS_TRY(hipEventRecord(run.ev[2], s));
    DSS_TRY(hipStreamSynchronize(s));      // also: off / end and the caller's arrays may go away now
    dss::book(&t.ms[0], run.ev[0], run.ev[1]);
    dss::book(&t.ms[1], run.ev[1], run.ev[2]);
    t.n[1] += 1;
    return DS_OK;
}

int Combine::get_bitmap(int64_t cap_words, uint32_t* out, std::string* err)
{
    const int64_t words = (nbits + 31) >> 5;
    if (cap_words < words || (words > 0 && !out)) return seterr(err, DS_ERR_INVALID, "ds_combine_bitmap: " + std::to_string(words) + " words, the array holds fewer");
    DSS_TRY(hipSetDevice(run.device));
    if (words) DSS_TRY(hipMemcpyAsync(out, bitmap, (size_t)words * 4, hipMemcpyDeviceToHost, run.s));
    DSS_TRY(hipStreamSynchronize(run.s));
    return DS_OK;
}

int Combine::parse(const char* text, int32_t n, const int64_t* rb, const int64_t* re, const int32_t* chrom, const uint8_t* flags, int32_t* status,
                   std::string* err)
{
    int rc = can_parse(ROUTE, n, text && rb && re && chrom && flags && status, err);
    if (rc) return rc;
    rc = rows.upload("ds_combine_parse", &run, text, n, rb, re, chrom, flags, err);
    if (rc) return rc;
    rows_begun = true;
    const RowArrays r = {rows.d_chrom, d_plus, rows.d_status, d_pos, d_c0, d_c1, d_c2, d_a, d_b};
    hipLaunchKernelGGL(combine_parse_kernel, dim3(blocks(n)), dim3(TPB), 0, run.s, form, rows.text.p, rows.d_off, rows.d_len, rows.d_flags, n, nrec, d_rec_base,
                       d_rec_len, bitmap, r);
    rc = rows.finish(&run, n, status, &t.ms[0], &t.ms[2], err);
    if (rc) return rc;
    pending = n;
    return DS_OK;
}

int Combine::accumulate(int32_t m, const int32_t* row, const int32_t* ostatus, const int32_t* chrom, const int64_t* pos, const int32_t* plus,
                        const double* a, const double* b, const int64_t* c0, const int64_t* c1, const int64_t* c2, std::string* err)
{
    const int ready = can_accumulate(ROUTE, err);
    if (ready) return ready;
    const int n = pending;
    if (m < 0 || m > n) return seterr(err, DS_ERR_INVALID, "ds_combine_accumulate: nover must be in [0, rows of the batch]");
    if (m > 0 && (!row || !ostatus || !chrom || !pos || !plus || !a || !b || !c0 || !c1 || !c2))
        return seterr(err, DS_ERR_INVALID, "ds_combine_accumulate: null argument");
    for (int k = 0; k < m; ++k) {
        if (!dss::override_row_ok(row, k, n))
            return seterr(err, DS_ERR_INVALID, "ds_combine_accumulate: override rows must be ascending indices of the batch");
        if (ostatus[k] == ROW_SKIP) continue;
        if (ostatus[k] != ROW_OK || chrom[k] < 0 || chrom[k] >= nrec || pos[k] < 0 || pos[k] >= h_len[(size_t)chrom[k]] || !count_ok(c0[k]) ||
            !count_ok(c1[k]) || !count_ok(c2[k]))
            return seterr(err, DS_ERR_INVALID, "ds_combine_accumulate: override " + std::to_string(k) + " has a status, record, position or count outside its range");
    }
    const dss::Column in[10] = {dss::col(pos), dss::col(a), dss::col(b), dss::col(c0), dss::col(c1), dss::col(c2), dss::col(row), dss::col(ostatus),
                                dss::col(chrom), dss::col(plus)};
    dss::Columns o;
    DSS_TRY(o.stage(&run, &over, (size_t)m, in, 10));
    hipStream_t s = run.s;
    if (m > 0) {
        const RowArrays r = {rows.d_chrom, d_plus, rows.d_status, d_pos, d_c0, d_c1, d_c2, d_a, d_b};
        const RowArrays g = {o.at<int32_t>(8), o.at<int32_t>(9), o.at<int32_t>(7), o.at<int64_t>(0), o.at<int64_t>(3), o.at<int64_t>(4), o.at<int64_t>(5),
                             o.at<double>(1), o.at<double>(2)};
        hipLaunchKernelGGL(combine_override_kernel, dim3(blocks(m)), dim3(TPB), 0, s, m, o.at<int32_t>(6), o.at<int32_t>(7), g, r);
        DSS_TRY(hipGetLastError());
    }
    DSS_TRY(hipEventRecord(run.ev[1], s));
    int Pn = 1;                   // the network sorts the smallest power of two that holds the batch
    while (Pn < n) Pn <<= 1;
    hipLaunchKernelGGL(combine_insert_kernel, dim3(blocks(Pn)), dim3(TPB), 0, s, n, Pn, (ull)rows_done, rows.d_chrom, d_pos, d_plus, rows.d_status, u64(t_key),
                       u64(t_plus), (ull)(cap - 1), u64(d_sort), counters);
    DSS_TRY(hipGetLastError());
    DSS_TRY(hipEventRecord(run.ev[2], s));
    DSS_TRY(dss::bitonic_sort(d_sort, Pn, s));
    DSS_TRY(hipEventRecord(run.ev[3], s));
    hipLaunchKernelGGL(combine_accumulate_kernel, dim3(blocks(Pn)), dim3(TPB), 0, s, Pn, u64(d_sort), d_a, d_b, d_c0, d_c1, d_c2, t_sum0, t_sum1, t_met,
                       t_unmet, t_cov);
    ull c[4] = {0, 0, 0, 0};
    const int rc = dss::finish_batch(&run, counters, c, &t.ms[0], &t.ms[3], &t.ms[4], err);
    if (rc) return rc;
    t.n[0] += 1;
    pending = -1;
    rows_done += n;
    return dss::batch_verdict("ds_combine_accumulate", c, err);
}

int64_t Combine::result(int64_t cap_sites, int32_t* chrom, int64_t* pos, double* sum0, double* sum1, int64_t* met, int64_t* unmet, int64_t* cov,
                        int64_t* last_plus, int64_t* nrows, std::string* err)
{
    const int ready = can_result(ROUTE, err);
    if (ready) return ready;
    DSS_TRY(hipSetDevice(run.device));
    ull c[4] = {0, 0, 0, 0};
    DSS_TRY(hipMemcpy(c, counters, sizeof(c), hipMemcpyDeviceToHost));
    const int64_t nsites = (int64_t)c[0];
    if (nrows) *nrows = rows_done;
    if (cap_sites == 0 && !chrom) return nsites;        // the size query
    if (!chrom || !pos || !sum0 || !sum1 || !met || !unmet || !cov || !last_plus) return seterr(err, DS_ERR_INVALID, "ds_combine_result: null argument");
    if (cap_sites < nsites) return seterr(err, DS_ERR_INVALID, "ds_combine_result: " + std::to_string(nsites) + " sites, the arrays hold fewer");
    if (nsites == 0) return 0;
    const dss::Column out[8] = {dss::col(pos), dss::col(sum0), dss::col(sum1), dss::col(met), dss::col(unmet), dss::col(cov), dss::col(last_plus),
                                dss::col(chrom)};
    dss::Columns o;
    DSS_TRY(o.carve(&run, (size_t)nsites, out, 8));
    hipLaunchKernelGGL(combine_result_kernel, dim3(blocks(cap)), dim3(TPB), 0, run.s, (ull)cap, u64(t_key), u64(t_plus), t_sum0, t_sum1, t_met, t_unmet, t_cov,
                       o.cursor(), (ull)nsites, o.at<int32_t>(7), o.at<int64_t>(0), o.at<double>(1), o.at<double>(2), o.at<int64_t>(3), o.at<int64_t>(4),
                       o.at<int64_t>(5), o.at<int64_t>(6));
    const hipError_t e = o.fetch(&run, hipGetLastError(), (size_t)nsites, out, 8);
    if (e != hipSuccess) return seterr(err, DS_ERR_HIP, std::string("ds_combine_result: ") + hipGetErrorString(e));
    return nsites;
}

void Combine::end()
{
    if (run.close()) pending = -1;
}

bool motif_reference(const char* text, int64_t nseg, const int64_t* sb, const int64_t* se, const int64_t* bit, const uint8_t* carry, int64_t nbits,
                     uint32_t* bitmap, std::string* err)
{
    if (nseg == 0) return true;
    if (nseg < 0 || nbits < 0 || !text || !sb || !se || !bit || !carry || (nbits > 0 && !bitmap)) {
        seterr(err, -1, "bad argument");
        return false;
    }
    if (!segments_ok(nseg, sb, se, bit, carry, nbits, err)) return false;
    for (int64_t i = 0; i < nseg; ++i) {
        const unsigned char* seg = reinterpret_cast<const unsigned char*>(text) + sb[i];
        for (int64_t j = 0; j < se[i] - sb[i]; ++j) {
            const int64_t hit = motif_bit(seg, j, carry[i], bit[i]);
            if (hit >= 0 && hit < nbits) bitmap[hit >> 5] |= 1u << (hit & 31);
        }
    }
    return true;
}

int64_t reference(int form, const char* text, int64_t nrows, const int64_t* begin, const int64_t* end, int32_t* chrom, const uint8_t* flags,
                  int32_t nrec, const int64_t* rec_len, const uint32_t* bitmap, int32_t* status, int64_t* pos, int32_t* plus, double* a, double* b,
                  int64_t* c0, int64_t* c1, int64_t* c2, int64_t cap, int32_t* site_chrom, int64_t* site_pos, double* sum0, double* sum1,
                  int64_t* met, int64_t* unmet, int64_t* cov, int64_t* last_plus, std::string* err)
{
    if (nrows == 0) return 0;
    if (nrows < 0 || (form != FORM_TABLE && form != FORM_BED) || !text || !begin || !end || !chrom || !flags || nrec < 1 || nrec > dss::CHROM_LIMIT ||
        !rec_len || !bitmap || !status || !pos || !plus || !a || !b || !c0 || !c1 || !c2 || cap < 0 ||
        (cap > 0 && (!site_chrom || !site_pos || !sum0 || !sum1 || !met || !unmet || !cov || !last_plus))) {
        seterr(err, -1, "ds_combine_reference: bad argument");
        return -1;
    }
    std::vector<int64_t> base((size_t)nrec);
    int64_t bits = 0;
    for (int32_t i = 0; i < nrec; ++i) {
        if (rec_len[i] < 0 || rec_len[i] > dss::POS_LIMIT || bits + rec_len[i] > MAX_GENOME_BITS) {
            seterr(err, -1, "ds_combine_reference: a record's length is outside [0, 2^40], or more than 2^46 bases in all");
            return -1;
        }
        base[(size_t)i] = bits;
        bits += rec_len[i];
    }
    std::unordered_map<uint64_t, int64_t> index;      // key -> site, sites numbered by first row
    int64_t nsites = 0;
    for (int64_t r = 0; r < nrows; ++r) {
        if (begin[r] < 0 || end[r] < begin[r]) {
            seterr(err, -1, "ds_combine_reference: row " + std::to_string(r) + " has a bad span");
            return -1;
        }
        if (status[r] == ROW_GIVEN) {
            if (chrom[r] < 0 || chrom[r] >= nrec || pos[r] < 0 || pos[r] >= rec_len[chrom[r]] || !count_ok(c0[r]) || !count_ok(c1[r]) || !count_ok(c2[r])) {
                seterr(err, -1, "ds_combine_reference: row " + std::to_string(r) + " was given a record, position or count outside its range");
                return -1;
            }
            status[r] = ROW_OK;
        } else if (status[r] == ROW_GIVEN_SKIP) {
            status[r] = ROW_SKIP;
        } else {
            Row v = {0, 0, 0.0, 0.0, 0, 0, 0};
            status[r] = parse_row(form, text + begin[r], text + end[r], chrom[r], flags[r], nrec, base.data(), rec_len, bitmap, &v);
            pos[r] = v.pos; plus[r] = v.plus; a[r] = v.a; b[r] = v.b; c0[r] = v.c0; c1[r] = v.c1; c2[r] = v.c2;
        }
        if (status[r] != ROW_OK || cap == 0) continue;
        const uint64_t k = dss::make_key(chrom[r], pos[r]);
        auto it = index.find(k);
        int64_t sidx;
        if (it == index.end()) {
            sidx = nsites++;
            index.emplace(k, sidx);
            if (sidx < cap) {
                site_chrom[sidx] = chrom[r]; site_pos[sidx] = pos[r];
                sum0[sidx] = 0.0; sum1[sidx] = 0.0; met[sidx] = 0; unmet[sidx] = 0; cov[sidx] = 0; last_plus[sidx] = -1;
            }
        } else {
            sidx = it->second;
        }
        if (sidx < cap) {
            sum0[sidx] += a[r];
            sum1[sidx] += b[r];
            met[sidx] += c0[r]; unmet[sidx] += c1[r]; cov[sidx] += c2[r];
            if (plus[r]) last_plus[sidx] = r;
        }
    }
    if (nsites > cap) {
        seterr(err, -1, "ds_combine_reference: " + std::to_string(nsites) + " sites, the arrays hold fewer");
        return -1;
    }
    return nsites;
}

}  // namespace dsc
