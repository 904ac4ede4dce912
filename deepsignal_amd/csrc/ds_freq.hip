// ds_freq.hip — per-site modification frequency on the GPU (call_freq --on gpu). A batch of result rows goes through four steps:
// freq_parse_kernel (one row per lane: ten columns tokenised, position, label and the two probabilities by the routines of
// ds_freq.h, the code the host checker runs), freq_insert_kernel (the used rows' exact keys chrom_id << 40 | pos into the site
// table of ds_site_table.h; the slot is the site id, its first global row kept by atomicMin), the bitonic sort of the unique 64-bit
// keys site << 32 | row over the batch, and freq_accumulate_kernel (the lane at the head of a site's run adds the run's
// probabilities IN ROW ORDER into the site's running double sums: no floating-point atomics, the order of addition is the
// contract). The table lives across the batches of a run. Built with -ffp-contract=off and no fast-math (csrc/Makefile).
#include "ds_freq.h"

#include <unordered_map>

namespace dsf {

namespace {

using dss::TPB;
using dss::blocks;
using dss::seterr;
using dss::u64;
using dss::ull;

__global__ __launch_bounds__(TPB) void freq_parse_kernel(const char* text, const int64_t* off, const int32_t* len, const int32_t* chrom,
                                                         const uint8_t* flags, int n, int64_t* pos, double* p0, double* p1, int32_t* met,
                                                         int32_t* status)
{
    const int i = blockIdx.x * TPB + threadIdx.x;
    if (i >= n) return;
    const char* b = text + off[i];
    int64_t v = 0;
    double a = 0, c = 0;
    int32_t m = 0;
    const int st = parse_row(b, b + len[i], chrom[i], flags[i], &v, &a, &c, &m);
    pos[i] = v; p0[i] = a; p1[i] = c; met[i] = m;
    status[i] = st;
}

// the caller's values for the rows the device left to it
__global__ __launch_bounds__(TPB) void freq_override_kernel(int m, const int32_t* row, const int32_t* ochrom, const int64_t* opos,
                                                            const double* op0, const double* op1, const int32_t* omet, int32_t* chrom,
                                                            int64_t* pos, double* p0, double* p1, int32_t* met, int32_t* status)
{
    const int k = blockIdx.x * TPB + threadIdx.x;
    if (k >= m) return;
    const int i = row[k];
    chrom[i] = ochrom[k]; pos[i] = opos[k]; p0[i] = op0[k]; p1[i] = op1[k]; met[i] = omet[k];
    status[i] = ROW_OK;
}

__global__ __launch_bounds__(TPB) void freq_insert_kernel(int n, int P, double cf, ull row_base, const int32_t* chrom, const int64_t* pos,
                                                          const double* p0, const double* p1, const int32_t* status, ull* t_key, ull* t_first,
                                                          ull mask, ull* sort, ull* counters)
{
    const int i = blockIdx.x * TPB + threadIdx.x;
    if (i >= P) return;
    ull sk = dss::SORT_PAD;
    if (i < n) {
        if (status[i] != ROW_OK || !dss::key_ok(chrom[i], pos[i])) {
            atomicAdd(&counters[3], 1ull);
        } else if (row_used(p0[i], p1[i], cf)) {
            const ull s = dss::insert_row(t_key, mask, dss::make_key(chrom[i], pos[i]), i, counters, &sk);
            if (s != dss::NO_SLOT) atomicMin(&t_first[s], row_base + (ull)i);
        }
    }
    sort[i] = sk;
}

__global__ __launch_bounds__(TPB) void freq_accumulate_kernel(int P, const ull* sorted, const double* p0, const double* p1, const int32_t* met,
                                                              double* t_sum0, double* t_sum1, int32_t* t_met, int32_t* t_unmet)
{
    const int t = blockIdx.x * TPB + threadIdx.x;
    ull site;
    if (!dss::run_head(sorted, P, t, &site)) return;
    double a = t_sum0[site], b = t_sum1[site];
    int32_t m = t_met[site], u = t_unmet[site];
    dss::walk_run(sorted, P, t, site, [&](unsigned i) {
        a += p0[i];
        b += p1[i];
        if (met[i]) ++m; else ++u;
    });
    t_sum0[site] = a; t_sum1[site] = b; t_met[site] = m; t_unmet[site] = u;
}

__global__ __launch_bounds__(TPB) void freq_result_kernel(ull cap, const ull* t_key, const ull* t_first, const double* t_sum0, const double* t_sum1,
                                                          const int32_t* t_met, const int32_t* t_unmet, ull* cursor, ull out_cap, int64_t* first_row,
                                                          int32_t* chrom, int64_t* pos, double* sum0, double* sum1, int32_t* met, int32_t* unmet)
{
    const ull s = (ull)blockIdx.x * TPB + threadIdx.x;
    ull o;
    if (!dss::compact_slot(cap, t_key, s, cursor, out_cap, chrom, pos, &o)) return;
    first_row[o] = (int64_t)t_first[s];
    sum0[o] = t_sum0[s]; sum1[o] = t_sum1[s]; met[o] = t_met[s]; unmet[o] = t_unmet[s];
}

// call_mods --freq_file: a batch's values straight from the forward's act rows (call_value of ds_freq.h, the code the host
// checker runs). chrom == nullptr: no key to check (ds_freq_values)
__global__ __launch_bounds__(TPB) void freq_values_kernel(int n, const int32_t* chrom, const int64_t* pos, const float* act, int class_num,
                                                          const int32_t* pred, double* p0, double* p1, int32_t* met, int32_t* status)
{
    const int i = blockIdx.x * TPB + threadIdx.x;
    if (i >= n) return;
    double a = 0, c = 0;
    int st = ROW_HOST;
    if (!chrom || dss::key_ok(chrom[i], pos[i])) st = call_value(act[(size_t)i * class_num], act[(size_t)i * class_num + 1], &a, &c);
    p0[i] = a; p1[i] = c;
    if (met) met[i] = pred[i] == 1;
    status[i] = st;
}

// after freq_insert_kernel, before the sort permutes `sort`: row i opened its site when it is the site's first row of the run
__global__ __launch_bounds__(TPB) void freq_opened_kernel(int n, ull row_base, const ull* sort, const ull* t_first, int32_t* opened)
{
    const int i = blockIdx.x * TPB + threadIdx.x;
    if (i >= n) return;
    const ull sk = sort[i];
    opened[i] = sk != dss::SORT_PAD && t_first[sk >> 32] == row_base + (ull)i;
}

// the table doubles: every occupied slot of the old table finds its slot in the new one (the keys are distinct and the new table is
// at most a quarter full) and takes its sums and counts along
__global__ __launch_bounds__(TPB) void freq_rehash_kernel(ull old_cap, const ull* o_key, const ull* o_first, const double* o_sum0, const double* o_sum1,
                                                          const int32_t* o_met, const int32_t* o_unmet, ull mask, ull* t_key, ull* t_first,
                                                          double* t_sum0, double* t_sum1, int32_t* t_met, int32_t* t_unmet, ull* counters)
{
    const ull o = (ull)blockIdx.x * TPB + threadIdx.x;
    if (o >= old_cap) return;
    const ull k = o_key[o];
    if (k == dss::EMPTY) return;
    bool opened;
    const ull s = dss::find_slot(t_key, mask, k, &opened);
    if (s == dss::NO_SLOT) {
        atomicAdd(&counters[2], 1ull);      // cannot happen below a load of one half; the next accumulate reports it
        return;
    }
    t_first[s] = o_first[o]; t_sum0[s] = o_sum0[o]; t_sum1[s] = o_sum1[o]; t_met[s] = o_met[o]; t_unmet[s] = o_unmet[o];
}

}  // namespace

int Freq::begin(int dev, int64_t total, int32_t batch, double prob_cf, std::string* err)
{
    const int rc = sizes(ROUTE, 1, total, batch, err);
    if (rc) return rc;
    if (prob_cf != prob_cf) return seterr(err, DS_ERR_INVALID, "ds_freq_begin: prob_cf is NaN");
    cap = 64;
    while (cap < 2 * (uint64_t)total) cap <<= 1;
    return open(dev, batch, prob_cf, err);
}

int Freq::begin_stream(int dev, int64_t initial_slots, int32_t batch, double prob_cf, std::string* err)
{
    if (initial_slots < 1 || initial_slots > 2 * dss::MAX_TOTAL_ROWS) return seterr(err, DS_ERR_INVALID, "ds_freq_begin_stream: initial_slots must be in [1, 2^31]");
    if (batch < 1 || batch > (1 << 24)) return seterr(err, DS_ERR_INVALID, "ds_freq_begin_stream: batch_rows must be in [1, 2^24]");
    if (prob_cf != prob_cf) return seterr(err, DS_ERR_INVALID, "ds_freq_begin_stream: prob_cf is NaN");
    total_rows = dss::MAX_TOTAL_ROWS;
    streaming = true;
    cap = 1;
    while (cap < (uint64_t)initial_slots) cap <<= 1;
    const int rc = open(dev, batch, prob_cf, err);
    if (rc) return rc;
    DSS_TRY(run.alloc(&d_pred, (size_t)batch * 4));
    DSS_TRY(run.alloc(&d_opened, (size_t)batch * 4));
    return DS_OK;
}

int Freq::open(int dev, int32_t batch, double prob_cf, std::string* err)
{
    batch_rows = batch; cf = prob_cf;
    size_t P = 1;                 // the sort's keys: batch_rows rounded up to a power of two
    while (P < (size_t)batch) P <<= 1;
    DSS_TRY(run.open(dev));
    const size_t B = (size_t)batch;
    DSS_TRY(run.alloc(&t_key, cap * 8, 0xff));
    DSS_TRY(run.alloc(&t_first, cap * 8, 0xff));
    DSS_TRY(run.alloc(&t_sum0, cap * 8, 0));
    DSS_TRY(run.alloc(&t_sum1, cap * 8, 0));
    DSS_TRY(run.alloc(&t_met, cap * 4, 0));
    DSS_TRY(run.alloc(&t_unmet, cap * 4, 0));
    DSS_TRY(run.alloc(&counters, 8 * 8, 0));
    DSS_TRY(rows.alloc(&run, B));
    DSS_TRY(run.alloc(&d_met, B * 4));
    DSS_TRY(run.alloc(&d_pos, B * 8));
    DSS_TRY(run.alloc(&d_p0, B * 8));
    DSS_TRY(run.alloc(&d_p1, B * 8));
    DSS_TRY(run.alloc(&d_sort, P * 8));
    DSS_TRY(hipStreamSynchronize(run.s));
    return DS_OK;
}

// the table doubles until the batch's rows, were each a new site, leave it at most half full. The new table is complete before the
// old one goes: a growth that does not fit the device leaves the run as it was (DS_ERR_NOMEM)
int Freq::grow(int32_t n, std::string* err)
{
    uint64_t want = cap;
    int doublings = 0;
    while (2 * ((uint64_t)sites + (uint64_t)n) > want) { want <<= 1; ++doublings; }
    if (want == cap) return DS_OK;
    void** const col[6] = {(void**)&t_key, (void**)&t_first, (void**)&t_sum0, (void**)&t_sum1, (void**)&t_met, (void**)&t_unmet};
    void* fresh[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    const size_t width[6] = {8, 8, 8, 8, 4, 4};
    const int fill[6] = {0xff, 0xff, 0, 0, 0, 0};
    hipStream_t s = run.s;
    hipError_t e = hipSuccess;
    for (int i = 0; i < 6 && e == hipSuccess; ++i) e = hipMalloc(&fresh[i], want * width[i]);
    if (e == hipSuccess) e = hipEventRecord(run.ev[0], s);
    for (int i = 0; i < 6 && e == hipSuccess; ++i) e = hipMemsetAsync(fresh[i], fill[i], want * width[i], s);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(freq_rehash_kernel, dim3(blocks(cap)), dim3(TPB), 0, s, (ull)cap, u64(t_key), u64(t_first), t_sum0, t_sum1, t_met, t_unmet,
                           (ull)(want - 1), static_cast<ull*>(fresh[0]), static_cast<ull*>(fresh[1]), static_cast<double*>(fresh[2]),
                           static_cast<double*>(fresh[3]), static_cast<int32_t*>(fresh[4]), static_cast<int32_t*>(fresh[5]), counters);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipEventRecord(run.ev[1], s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        for (void* p : fresh) if (p) (void)hipFree(p);
        return seterr(err, e == hipErrorOutOfMemory ? DS_ERR_NOMEM : DS_ERR_HIP,
                      "ds_freq_push: growing the site table to " + std::to_string(want) + " slots: " + hipGetErrorString(e));
    }
    dss::book(&t.stream.ms[1], run.ev[0], run.ev[1]);
    for (int i = 0; i < 6; ++i) { (void)hipFree(*col[i]); *col[i] = fresh[i]; }      // `run` holds the members' addresses: the new table is its own now
    cap = want;
    t.stream.n[0] += doublings;       // several doublings at once are one rehash
    return DS_OK;
}

int Freq::push(int32_t n, const int32_t* chrom, const int64_t* pos, const float* act_rows, int32_t class_num, const int32_t* pred, int32_t* status,
               int32_t* opened, std::string* err)
{
    if (!streaming) return seterr(err, DS_ERR_INVALID, "ds_freq_push: no streaming run is open (ds_freq_begin_stream first)");
    if (pending >= 0) return seterr(err, DS_ERR_INVALID, "ds_freq_push: the previous batch has not been accumulated");
    if (!chrom || !pos || !act_rows || !pred || !status || !opened) return seterr(err, DS_ERR_INVALID, "ds_freq_push: null argument");
    if (n < 1 || n > batch_rows) return seterr(err, DS_ERR_INVALID, "ds_freq_push: nrows must be in [1, batch_rows]");
    if (class_num < 2 || class_num > 1024) return seterr(err, DS_ERR_INVALID, "ds_freq_push: class_num must be in [2, 1024]");
    if (rows_done + n > total_rows) return seterr(err, DS_ERR_INVALID, "ds_freq_push: more than 2^30 rows in one run");
    DSS_TRY(hipSetDevice(run.device));
    const int rc = grow(n, err);
    if (rc) return rc;
    DSS_TRY(act.grow(&run, (size_t)batch_rows * (size_t)class_num * 4));      // a whole batch's worth: grows when class_num does
    float* d_act = reinterpret_cast<float*>(act.p);
    hipStream_t s = run.s;
    DSS_TRY(hipEventRecord(run.ev[0], s));
    DSS_TRY(hipMemcpyAsync(rows.d_chrom, chrom, (size_t)n * 4, hipMemcpyHostToDevice, s));
    DSS_TRY(hipMemcpyAsync(d_pos, pos, (size_t)n * 8, hipMemcpyHostToDevice, s));
    DSS_TRY(hipMemcpyAsync(d_act, act_rows, (size_t)n * (size_t)class_num * 4, hipMemcpyHostToDevice, s));
    DSS_TRY(hipMemcpyAsync(d_pred, pred, (size_t)n * 4, hipMemcpyHostToDevice, s));
    DSS_TRY(hipEventRecord(run.ev[1], s));
    hipLaunchKernelGGL(freq_values_kernel, dim3(blocks(n)), dim3(TPB), 0, s, n, rows.d_chrom, d_pos, d_act, class_num, d_pred, d_p0, d_p1, d_met,
                       rows.d_status);
    const int rc2 = rows.finish(&run, n, status, &t.batch.ms[0], &t.stream.ms[0], err);
    if (rc2) return rc2;
    pending = n;
    opened_out = opened;
    return DS_OK;
}

int Freq::parse(const char* text, int32_t n, const int64_t* rb, const int64_t* re, const int32_t* chrom, const uint8_t* flags, int32_t* status,
                std::string* err)
{
    if (streaming) return seterr(err, DS_ERR_INVALID, "ds_freq_parse: the open run is a streaming one (ds_freq_push)");
    int rc = can_parse(ROUTE, n, text && rb && re && chrom && flags && status, err);
    if (rc) return rc;
    rc = rows.upload("ds_freq_parse", &run, text, n, rb, re, chrom, flags, err);
    if (rc) return rc;
    hipLaunchKernelGGL(freq_parse_kernel, dim3(blocks(n)), dim3(TPB), 0, run.s, rows.text.p, rows.d_off, rows.d_len, rows.d_chrom, rows.d_flags, n, d_pos,
                       d_p0, d_p1, d_met, rows.d_status);
    rc = rows.finish(&run, n, status, &t.batch.ms[0], &t.batch.ms[1], err);
    if (rc) return rc;
    pending = n;
    return DS_OK;
}

int Freq::accumulate(int32_t m, const int32_t* row, const int32_t* chrom, const int64_t* pos, const double* p0, const double* p1,
                     const int32_t* met, std::string* err)
{
    const int ready = can_accumulate(ROUTE, err);
    if (ready) return ready;
    const int n = pending;
    if (m < 0 || m > n) return seterr(err, DS_ERR_INVALID, "ds_freq_accumulate: nover must be in [0, rows of the batch]");
    if (m > 0 && (!row || !chrom || !pos || !p0 || !p1 || !met)) return seterr(err, DS_ERR_INVALID, "ds_freq_accumulate: null argument");
    for (int k = 0; k < m; ++k) {
        if (!dss::override_row_ok(row, k, n))
            return seterr(err, DS_ERR_INVALID, "ds_freq_accumulate: override rows must be ascending indices of the batch");
        if (!dss::key_ok(chrom[k], pos[k]))
            return seterr(err, DS_ERR_INVALID, "ds_freq_accumulate: override " + std::to_string(k) + " has a chromosome id or position outside the key");
    }
    const dss::Column in[6] = {dss::col(pos), dss::col(p0), dss::col(p1), dss::col(row), dss::col(chrom), dss::col(met)};
    dss::Columns o;
    DSS_TRY(o.stage(&run, &over, (size_t)m, in, 6));
    hipStream_t s = run.s;
    if (m > 0) {
        hipLaunchKernelGGL(freq_override_kernel, dim3(blocks(m)), dim3(TPB), 0, s, m, o.at<int32_t>(3), o.at<int32_t>(4), o.at<int64_t>(0), o.at<double>(1),
                           o.at<double>(2), o.at<int32_t>(5), rows.d_chrom, d_pos, d_p0, d_p1, d_met, rows.d_status);
        DSS_TRY(hipGetLastError());
    }
    DSS_TRY(hipEventRecord(run.ev[1], s));
    // the network sorts the smallest power of two that holds the batch
    int Pn = 1;
    while (Pn < n) Pn <<= 1;
    hipLaunchKernelGGL(freq_insert_kernel, dim3(blocks(Pn)), dim3(TPB), 0, s, n, Pn, cf, (ull)rows_done, rows.d_chrom, d_pos, d_p0, d_p1, rows.d_status,
                       u64(t_key), u64(t_first), (ull)(cap - 1), u64(d_sort), counters);
    DSS_TRY(hipGetLastError());
    if (streaming) {
        hipLaunchKernelGGL(freq_opened_kernel, dim3(blocks(n)), dim3(TPB), 0, s, n, (ull)rows_done, u64(d_sort), u64(t_first), d_opened);
        DSS_TRY(hipGetLastError());
        DSS_TRY(hipMemcpyAsync(opened_out, d_opened, (size_t)n * 4, hipMemcpyDeviceToHost, s));
    }
    DSS_TRY(hipEventRecord(run.ev[2], s));
    DSS_TRY(dss::bitonic_sort(d_sort, Pn, s));
    DSS_TRY(hipEventRecord(run.ev[3], s));
    hipLaunchKernelGGL(freq_accumulate_kernel, dim3(blocks(Pn)), dim3(TPB), 0, s, Pn, u64(d_sort), d_p0, d_p1, d_met, t_sum0, t_sum1, t_met, t_unmet);
    ull c[4] = {0, 0, 0, 0};
    const int rc = dss::finish_batch(&run, counters, c, &t.batch.ms[0], &t.batch.ms[2], &t.batch.ms[3], err);
    if (rc) return rc;
    t.batch.n[0] += 1;
    pending = -1;
    opened_out = nullptr;
    rows_done += n;
    sites = (int64_t)c[0];
    return dss::batch_verdict("ds_freq_accumulate", c, err);
}

int64_t Freq::result(int64_t cap_sites, int64_t* first_row, int32_t* chrom, int64_t* pos, double* sum0, double* sum1, int32_t* met, int32_t* unmet,
                     int64_t* nrows, int64_t* used, std::string* err)
{
    const int ready = can_result(ROUTE, err);
    if (ready) return ready;
    DSS_TRY(hipSetDevice(run.device));
    ull c[4] = {0, 0, 0, 0};
    DSS_TRY(hipMemcpy(c, counters, sizeof(c), hipMemcpyDeviceToHost));
    const int64_t nsites = (int64_t)c[0];
    if (nrows) *nrows = rows_done;
    if (used) *used = (int64_t)c[1];
    if (cap_sites == 0 && !first_row) return nsites;        // the size query
    if (!first_row || !chrom || !pos || !sum0 || !sum1 || !met || !unmet) return seterr(err, DS_ERR_INVALID, "ds_freq_result: null argument");
    if (cap_sites < nsites) return seterr(err, DS_ERR_INVALID, "ds_freq_result: " + std::to_string(nsites) + " sites, the arrays hold fewer");
    if (nsites == 0) return 0;
    const dss::Column out[7] = {dss::col(first_row), dss::col(pos), dss::col(sum0), dss::col(sum1), dss::col(chrom), dss::col(met), dss::col(unmet)};
    dss::Columns o;
    DSS_TRY(o.carve(&run, (size_t)nsites, out, 7));
    hipLaunchKernelGGL(freq_result_kernel, dim3(blocks(cap)), dim3(TPB), 0, run.s, (ull)cap, u64(t_key), u64(t_first), t_sum0, t_sum1, t_met, t_unmet,
                       o.cursor(), (ull)nsites, o.at<int64_t>(0), o.at<int32_t>(4), o.at<int64_t>(1), o.at<double>(2), o.at<double>(3), o.at<int32_t>(5),
                       o.at<int32_t>(6));
    const hipError_t e = o.fetch(&run, hipGetLastError(), (size_t)nsites, out, 7);
    if (e != hipSuccess) return seterr(err, DS_ERR_HIP, std::string("ds_freq_result: ") + hipGetErrorString(e));
    return nsites;
}

void Freq::end()
{
    if (!run.close()) return;
    opened_out = nullptr;
    pending = -1;
}

void values_reference(int64_t n, const float* act, int32_t class_num, double* p0, double* p1, int32_t* status)
{
    for (int64_t i = 0; i < n; ++i) {
        double a = 0, c = 0;
        status[i] = call_value(act[i * class_num], act[i * class_num + 1], &a, &c);
        p0[i] = a; p1[i] = c;
    }
}

int values_device(int device, int64_t n, const float* act, int32_t class_num, double* p0, double* p1, int32_t* status, std::string* err)
{
    if (n < 1 || n > (1 << 24) || class_num < 2 || class_num > 1024 || !act || !p0 || !p1 || !status)
        return seterr(err, DS_ERR_INVALID, "ds_freq_values: bad argument (1 <= n <= 2^24 rows of 2 <= class_num <= 1024 floats)");
    DSS_TRY(hipSetDevice(device));
    const size_t N = (size_t)n;
    char* d = nullptr;
    DSS_TRY(hipMalloc((void**)&d, N * (16 + 4 + 4 * (size_t)class_num)));
    double* d_a = reinterpret_cast<double*>(d);
    double* d_c = d_a + N;
    int32_t* d_st = reinterpret_cast<int32_t*>(d_c + N);
    float* d_in = reinterpret_cast<float*>(d_st + N);
    hipError_t e = hipMemcpy(d_in, act, N * 4 * (size_t)class_num, hipMemcpyHostToDevice);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(freq_values_kernel, dim3(blocks(N)), dim3(TPB), 0, nullptr, (int)n, nullptr, nullptr, d_in, class_num, nullptr, d_a, d_c,
                           nullptr, d_st);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpy(p0, d_a, N * 8, hipMemcpyDeviceToHost);
    if (e == hipSuccess) e = hipMemcpy(p1, d_c, N * 8, hipMemcpyDeviceToHost);
    if (e == hipSuccess) e = hipMemcpy(status, d_st, N * 4, hipMemcpyDeviceToHost);
    (void)hipFree(d);
    if (e != hipSuccess) { (void)hipGetLastError(); return seterr(err, DS_ERR_HIP, std::string("ds_freq_values: ") + hipGetErrorString(e)); }
    return DS_OK;
}

int64_t reference(const char* text, int64_t nrows, const int64_t* begin, const int64_t* end, const int32_t* chrom, const uint8_t* flags, double cf,
                  int32_t* status, int64_t* pos, double* p0, double* p1, int32_t* met, int64_t cap, int64_t* first_row, int32_t* site_chrom,
                  int64_t* site_pos, double* sum0, double* sum1, int32_t* site_met, int32_t* site_unmet, int64_t* used, std::string* err)
{
    if (used) *used = 0;
    if (nrows == 0) return 0;
    if (nrows < 0 || !text || !begin || !end || !chrom || !flags || !status || !pos || !p0 || !p1 || !met || cap < 0 ||
        (cap > 0 && (!first_row || !site_chrom || !site_pos || !sum0 || !sum1 || !site_met || !site_unmet))) {
        seterr(err, -1, "ds_freq_reference: bad argument");
        return -1;
    }
    std::unordered_map<uint64_t, int64_t> index;      // key -> site, sites numbered by first used row
    int64_t nsites = 0, nused = 0;
    for (int64_t r = 0; r < nrows; ++r) {
        if (begin[r] < 0 || end[r] < begin[r]) {
            seterr(err, -1, "ds_freq_reference: row " + std::to_string(r) + " has a bad span");
            return -1;
        }
        if (status[r] == ROW_GIVEN) {
            if (!dss::key_ok(chrom[r], pos[r])) {
                seterr(err, -1, "ds_freq_reference: row " + std::to_string(r) + " was given a chromosome id or position outside the key");
                return -1;
            }
            status[r] = ROW_OK;
        } else {
            int64_t v = 0;
            double a = 0, c = 0;
            int32_t m = 0;
            status[r] = parse_row(text + begin[r], text + end[r], chrom[r], flags[r], &v, &a, &c, &m);
            pos[r] = v; p0[r] = a; p1[r] = c; met[r] = m;
        }
        if (status[r] != ROW_OK || !row_used(p0[r], p1[r], cf)) continue;
        ++nused;
        const uint64_t k = dss::make_key(chrom[r], pos[r]);
        auto it = index.find(k);
        int64_t sidx;
        if (it == index.end()) {
            sidx = nsites++;
            index.emplace(k, sidx);
            if (sidx < cap) {
                first_row[sidx] = r; site_chrom[sidx] = chrom[r]; site_pos[sidx] = pos[r];
                sum0[sidx] = 0.0; sum1[sidx] = 0.0; site_met[sidx] = 0; site_unmet[sidx] = 0;
            }
        } else {
            sidx = it->second;
        }
        if (sidx < cap) {
            sum0[sidx] += p0[r];
            sum1[sidx] += p1[r];
            if (met[r]) ++site_met[sidx]; else ++site_unmet[sidx];
        }
    }
    if (used) *used = nused;
    if (nsites > cap) {
        seterr(err, -1, "ds_freq_reference: " + std::to_string(nsites) + " sites, the arrays hold fewer");
        return -1;
    }
    return nsites;
}

}  // namespace dsf
