// ds_eval.hip — call accuracy and AUROC of labelled call_mods result rows on the GPU (evaluate --on gpu). A batch at a time:
// eval_parse_kernel (one row per lane, ds_eval.h parse_row), eval_count_kernel (per tested set the confusion matrix and per cut-off
// called / correct: every term is a predicate, so a wave counts it with one ballot, the workgroup sums its waves in LDS and adds
// once per counter) and eval_insert_kernel (the row's score into the site table of ds_site_table.h under its order-preserving key;
// four 32-bit counts per slot by integer atomicAdd). At the end the occupied keys are compacted, padded and sorted by the bitonic
// network, each sorted key's counts are looked up again, the negatives below each score come from a multi-level workgroup scan and
// pos * (2 * below + neg) is reduced into one 64-bit U2 per set. All integers: no floating-point atomics, no order of addition.
// Built with -ffp-contract=off and no fast-math (csrc/Makefile).
#include "ds_eval.h"

#include <array>
#include <map>

namespace dse {

namespace {

using dss::TPB;
using dss::blocks;
using dss::seterr;
using dss::u64;
using dss::ull;

static_assert(ROW_OK == DS_TEXT_ROW_OK && ROW_HOST == DS_TEXT_ROW_HOST && ROW_GIVEN == DS_EVAL_ROW_GIVEN, "the public header's status codes");
static_assert(SET_BITS == (DS_EVAL_SET_SAMPLE | DS_EVAL_SET_ALL) && TRUTH_BIT == DS_EVAL_TRUTH, "the public header's bits of a row's byte");

constexpr int WAVE = 64;
constexpr int WAVES = TPB / WAVE;
constexpr int NCOUNT = NSETS * SET_COUNTERS;

__global__ __launch_bounds__(TPB) void eval_parse_kernel(const char* text, const int64_t* off, const int32_t* len, const uint8_t* flags, int n,
                                                         double* p0, double* p1, int32_t* called, int32_t* status)
{
    const int i = blockIdx.x * TPB + threadIdx.x;
    if (i >= n) return;
    const char* b = text + off[i];
    double a = 0.0, c = 0.0;
    int32_t lab = 0;
    status[i] = parse_row(b, b + len[i], flags[i], &a, &c, &lab);
    p0[i] = a; p1[i] = c; called[i] = lab;
}

// the caller's values for the rows the device left to it
__global__ __launch_bounds__(TPB) void eval_override_kernel(int m, const int32_t* row, const double* o_p0, const double* o_p1, const int32_t* o_called,
                                                            double* p0, double* p1, int32_t* called, int32_t* status)
{
    const int k = blockIdx.x * TPB + threadIdx.x;
    if (k >= m) return;
    const int i = row[k];
    p0[i] = o_p0[k]; p1[i] = o_p1[k]; called[i] = o_called[k] != 0;
    status[i] = ROW_OK;
}

// Every lane of a wave reaches every ballot (no early return). The wave's count of a predicate goes to the wave's row of `part`
// through lane 0; after the barrier thread t adds the rows of counter t and makes the workgroup's one atomic for it.
__global__ __launch_bounds__(TPB) void eval_count_kernel(int n, int ncf, const double* cf, const uint8_t* mask, const double* p0, const double* p1,
                                                         const int32_t* called, const int32_t* status, ull* counters)
{
    __shared__ unsigned part[WAVES][NCOUNT];
    const int i = blockIdx.x * TPB + threadIdx.x;
    const int wave = threadIdx.x / WAVE;
    const bool lead = (threadIdx.x % WAVE) == 0;
    for (int t = threadIdx.x; t < WAVES * NCOUNT; t += TPB) (&part[0][0])[t] = 0;
    __syncthreads();
    const bool in = i < n;
    const bool ok = in && status[i] == ROW_OK;
    const unsigned left = (unsigned)__popcll(__ballot(in && !ok));
    if (lead && left) atomicAdd(&counters[3], (ull)left);
    const unsigned m = ok ? mask[i] : 0u;
    const bool truth = (m & TRUTH_BIT) != 0;
    const bool lab = ok && called[i] != 0;
    const double a = ok ? p0[i] : 0.0, b = ok ? p1[i] : 0.0;
    for (int s = 0; s < NSETS; ++s) {
        const bool member = ok && ((m >> s) & 1u);
        unsigned* c = &part[wave][s * SET_COUNTERS];
        const unsigned tp = (unsigned)__popcll(__ballot(member && lab && truth));
        const unsigned fp = (unsigned)__popcll(__ballot(member && lab && !truth));
        const unsigned tn = (unsigned)__popcll(__ballot(member && !lab && !truth));
        const unsigned fn = (unsigned)__popcll(__ballot(member && !lab && truth));
        if (lead) { c[C_TP] = tp; c[C_FP] = fp; c[C_TN] = tn; c[C_FN] = fn; }
        for (int k = 0; k < ncf; ++k) {
            const double cut = cf[k];
            const bool stands = member && row_stands(a, b, cut);
            const unsigned nc = (unsigned)__popcll(__ballot(stands));
            const unsigned nr = (unsigned)__popcll(__ballot(stands && row_correct(a, b, cut, truth)));
            if (lead) { c[C_CALLED + k] = nc; c[C_CORRECT + k] = nr; }
        }
    }
    __syncthreads();
    for (int t = threadIdx.x; t < NCOUNT; t += TPB) {
        unsigned v = 0;
        for (int w = 0; w < WAVES; ++w) v += part[w][t];
        if (v) atomicAdd(&counters[COUNTERS_SETS + t], (ull)v);
    }
}

__global__ __launch_bounds__(TPB) void eval_insert_kernel(int n, const uint8_t* mask, const double* p1, const int32_t* status, ull* t_key, uint32_t* t_cnt,
                                                          ull slot_mask, ull* counters)
{
    const int i = blockIdx.x * TPB + threadIdx.x;
    if (i >= n || status[i] != ROW_OK) return;
    const unsigned m = mask[i];
    const double v = p1[i];
    if (!(m & SET_BITS) || !score_finite(v)) return;       // a non-finite score makes the set's AUROC 0: the caller knows, it gave the row
    bool opened;
    const ull s = dss::find_slot(t_key, slot_mask, score_key(v), &opened);
    // uniform addresses: the compiler folds a wave's additions into one atomic (the note in dss::insert_row)
    if (opened) atomicAdd(&counters[0], 1ull);
    if (s == dss::NO_SLOT) { atomicAdd(&counters[2], 1ull); return; }
    atomicAdd(&counters[1], 1ull);
    const bool truth = (m & TRUTH_BIT) != 0;
    for (int set = 0; set < NSETS; ++set)
        if ((m >> set) & 1u) atomicAdd(&t_cnt[4 * s + count_index(set, truth)], 1u);
}

// ---- the result -----------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(TPB) void eval_compact_kernel(ull cap, const ull* t_key, ull* cursor, ull out_cap, ull* keys)
{
    const ull s = (ull)blockIdx.x * TPB + threadIdx.x;
    if (s >= cap) return;
    const ull k = t_key[s];
    if (k == dss::EMPTY) return;
    const ull o = atomicAdd(cursor, 1ull);
    if (o < out_cap) keys[o] = k;
}

// sorted key t -> its slot again, read-only, and the slot's counts in sorted order; the two columns the scans run over start as neg
__global__ __launch_bounds__(TPB) void eval_lookup_kernel(ull nd, const ull* sorted, const ull* t_key, const uint32_t* t_cnt, ull slot_mask, uint32_t* cnt,
                                                          ull* below0, ull* below1)
{
    const ull t = (ull)blockIdx.x * TPB + threadIdx.x;
    if (t >= nd) return;
    const ull k = sorted[t];
    ull s = dss::hash_key(k) & slot_mask;
    bool found = false;
    for (ull probe = 0; probe <= slot_mask; ++probe) {
        const ull have = t_key[s];
        if (have == k) { found = true; break; }
        if (have == dss::EMPTY) break;
        s = (s + 1) & slot_mask;
    }
    uint32_t c[4] = {0, 0, 0, 0};
    if (found)
        for (int q = 0; q < 4; ++q) c[q] = t_cnt[4 * s + q];
    for (int q = 0; q < 4; ++q) cnt[4 * t + q] = c[q];
    below0[t] = c[1];
    below1[t] = c[3];
}

// one level of the scan: a workgroup's SCAN_SPAN elements become their exclusive prefix sums, the span's total goes to sums[block]
__global__ __launch_bounds__(TPB) void eval_scan_span_kernel(ull* data, ull n, ull* sums)
{
    __shared__ ull sh[SCAN_SPAN];
    const ull i = (ull)blockIdx.x * SCAN_SPAN + threadIdx.x;
    const int t = threadIdx.x;
    const ull v = i < n ? data[i] : 0ull;
    sh[t] = v;
    __syncthreads();
    for (int d = 1; d < SCAN_SPAN; d <<= 1) {
        const ull x = t >= d ? sh[t - d] : 0ull;
        __syncthreads();
        sh[t] += x;
        __syncthreads();
    }
    if (i < n) data[i] = sh[t] - v;
    if (t == SCAN_SPAN - 1) sums[blockIdx.x] = sh[t];
}

// ... and the scanned totals of the spans in front are added back
__global__ __launch_bounds__(TPB) void eval_scan_add_kernel(ull* data, ull n, const ull* sums)
{
    const ull i = (ull)blockIdx.x * SCAN_SPAN + threadIdx.x;
    if (i < n) data[i] += sums[blockIdx.x];
}

// data[0 .. n) -> exclusive prefix sums in place; scratch holds scan_scratch(n) elements
hipError_t exclusive_scan(ull* data, size_t n, ull* scratch, hipStream_t s)
{
    const size_t nb = (n + SCAN_SPAN - 1) / SCAN_SPAN;
    hipLaunchKernelGGL(eval_scan_span_kernel, dim3((unsigned)nb), dim3(TPB), 0, s, data, (ull)n, scratch);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess || nb <= 1) return e;
    e = exclusive_scan(scratch, nb, scratch + nb, s);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(eval_scan_add_kernel, dim3((unsigned)nb), dim3(TPB), 0, s, data, (ull)n, scratch);
    return hipGetLastError();
}

// the workgroup's sum of v at thread 0
__device__ __forceinline__ ull block_sum(ull v, ull* sh)
{
    __syncthreads();
    sh[threadIdx.x] = v;
    __syncthreads();
    for (int d = TPB / 2; d > 0; d >>= 1) {
        if ((int)threadIdx.x < d) sh[threadIdx.x] += sh[threadIdx.x + d];
        __syncthreads();
    }
    return sh[0];
}

// out[3 * set + 0 .. 2] += U2, P, N of the set over this workgroup's scores
__global__ __launch_bounds__(TPB) void eval_u2_kernel(ull nd, const uint32_t* cnt, const ull* below0, const ull* below1, ull* out)
{
    __shared__ ull sh[TPB];
    const ull t = (ull)blockIdx.x * TPB + threadIdx.x;
    const bool in = t < nd;
    for (int set = 0; set < NSETS; ++set) {
        const ull pos = in ? cnt[4 * t + 2 * set] : 0ull, neg = in ? cnt[4 * t + 2 * set + 1] : 0ull;
        const ull below = in ? (set ? below1[t] : below0[t]) : 0ull;
        const ull u2 = block_sum(pos * (2ull * below + neg), sh);
        const ull p = block_sum(pos, sh);
        const ull q = block_sum(neg, sh);
        if (threadIdx.x == 0) {
            if (u2) atomicAdd(&out[3 * set + 0], u2);
            if (p) atomicAdd(&out[3 * set + 1], p);
            if (q) atomicAdd(&out[3 * set + 2], q);
        }
    }
}

bool cutoffs_ok(int32_t ncf, const double* cf) { return ncf >= 1 && ncf <= MAX_CF && cf != nullptr; }

}  // namespace

int Eval::begin(int dev, int64_t total, int32_t batch, int32_t n_cf, const double* cf, std::string* err)
{
    const int rc = sizes(ROUTE, 1, total, batch, err);
    if (rc) return rc;
    if (!cutoffs_ok(n_cf, cf)) return seterr(err, DS_ERR_INVALID, "ds_eval_begin: 1 .. 32 cut-offs");
    ncf = n_cf;
    cap = 64;
    while (cap < 2 * (uint64_t)total) cap <<= 1;
    const size_t B = (size_t)batch;
    zeros.assign(B, 0);
    DSS_TRY(run.open(dev));
    DSS_TRY(run.alloc(&t_key, cap * 8, 0xff));
    DSS_TRY(run.alloc(&t_cnt, cap * 16, 0));
    DSS_TRY(run.alloc(&counters, (size_t)COUNTERS_TOTAL * 8, 0));
    DSS_TRY(run.alloc(&d_cf, (size_t)MAX_CF * 8, 0));
    DSS_TRY(rows.alloc(&run, B));
    DSS_TRY(run.alloc(&d_mask, B));
    DSS_TRY(run.alloc(&d_called, B * 4));
    DSS_TRY(run.alloc(&d_p0, B * 8));
    DSS_TRY(run.alloc(&d_p1, B * 8));
    DSS_TRY(hipMemcpyAsync(d_cf, cf, (size_t)n_cf * 8, hipMemcpyHostToDevice, run.s));
    DSS_TRY(hipStreamSynchronize(run.s));      // also: the caller's cut-offs may go away now
    return DS_OK;
}

int Eval::parse(const char* text, int32_t n, const int64_t* rb, const int64_t* re, const uint8_t* flags, int32_t* status, std::string* err)
{
    int rc = can_parse(ROUTE, n, text && rb && re && flags && status, err);
    if (rc) return rc;
    rc = rows.upload("ds_eval_parse", &run, text, n, rb, re, zeros.data(), flags, err);      // the rows name no chromosome here
    if (rc) return rc;
    hipLaunchKernelGGL(eval_parse_kernel, dim3(blocks(n)), dim3(TPB), 0, run.s, rows.text.p, rows.d_off, rows.d_len, rows.d_flags, n, d_p0, d_p1, d_called,
                       rows.d_status);
    rc = rows.finish(&run, n, status, &t.ms[0], &t.ms[1], err);
    if (rc) return rc;
    pending = n;
    return DS_OK;
}

int Eval::accumulate(const uint8_t* mask, int32_t m, const int32_t* row, const double* p0, const double* p1, const int32_t* called, std::string* err)
{
    const int ready = can_accumulate(ROUTE, err);
    if (ready) return ready;
    const int n = pending;
    if (!mask) return seterr(err, DS_ERR_INVALID, "ds_eval_accumulate: null argument");
    if (m < 0 || m > n) return seterr(err, DS_ERR_INVALID, "ds_eval_accumulate: nover must be in [0, rows of the batch]");
    if (m > 0 && (!row || !p0 || !p1 || !called)) return seterr(err, DS_ERR_INVALID, "ds_eval_accumulate: null argument");
    for (int i = 0; i < n; ++i)
        if (mask[i] & ~(SET_BITS | TRUTH_BIT)) return seterr(err, DS_ERR_INVALID, "ds_eval_accumulate: a row's byte holds bits 0 .. 2 only");
    for (int k = 0; k < m; ++k)
        if (!dss::override_row_ok(row, k, n)) return seterr(err, DS_ERR_INVALID, "ds_eval_accumulate: override rows must be ascending indices of the batch");
    const dss::Column in[4] = {dss::col(p0), dss::col(p1), dss::col(row), dss::col(called)};
    dss::Columns o;
    DSS_TRY(o.stage(&run, &over, (size_t)m, in, 4));
    hipStream_t s = run.s;
    DSS_TRY(hipMemcpyAsync(d_mask, mask, (size_t)n, hipMemcpyHostToDevice, s));
    if (m > 0) {
        hipLaunchKernelGGL(eval_override_kernel, dim3(blocks(m)), dim3(TPB), 0, s, m, o.at<int32_t>(2), o.at<double>(0), o.at<double>(1), o.at<int32_t>(3), d_p0,
                           d_p1, d_called, rows.d_status);
        DSS_TRY(hipGetLastError());
    }
    DSS_TRY(hipEventRecord(run.ev[1], s));
    hipLaunchKernelGGL(eval_count_kernel, dim3(blocks(n)), dim3(TPB), 0, s, n, (int)ncf, d_cf, d_mask, d_p0, d_p1, d_called, rows.d_status, counters);
    DSS_TRY(hipGetLastError());
    hipLaunchKernelGGL(eval_insert_kernel, dim3(blocks(n)), dim3(TPB), 0, s, n, d_mask, d_p1, rows.d_status, u64(t_key), t_cnt, (ull)(cap - 1), counters);
    DSS_TRY(hipGetLastError());
    DSS_TRY(hipEventRecord(run.ev[2], s));
    ull c[4] = {0, 0, 0, 0};
    DSS_TRY(hipMemcpyAsync(c, counters, sizeof(c), hipMemcpyDeviceToHost, s));
    DSS_TRY(hipStreamSynchronize(s));          // also: the caller's arrays may go away now
    dss::book(&t.ms[0], run.ev[0], run.ev[1]);
    dss::book(&t.ms[2], run.ev[1], run.ev[2]);
    t.n[0] += 1;
    pending = -1;
    rows_done += n;
    return dss::batch_verdict("ds_eval_accumulate", c, err);
}

int Eval::result(int64_t* counts, uint64_t* u2, int64_t* pn, int64_t* nn, int64_t* nrows, int64_t* distinct, std::string* err)
{
    const int ready = can_result(ROUTE, err);
    if (ready) return ready;
    if (!counts || !u2 || !pn || !nn) return seterr(err, DS_ERR_INVALID, "ds_eval_result: null argument");
    hipStream_t s = run.s;
    DSS_TRY(hipSetDevice(run.device));
    ull c[COUNTERS_TOTAL];
    DSS_TRY(hipMemcpyAsync(c, counters, sizeof(c), hipMemcpyDeviceToHost, s));
    DSS_TRY(hipStreamSynchronize(s));
    const size_t nd = (size_t)c[0];
    if (nd > cap) return seterr(err, DS_ERR_INVALID, "ds_eval_result: more distinct scores than table slots");
    if (nd > 0) {
        size_t Pn = 1;                // the network sorts the smallest power of two that holds the distinct scores
        while (Pn < nd) Pn <<= 1;
        const size_t scratch = scan_scratch(nd);
        DSS_TRY(res.grow(&run, Pn * 8 + nd * 16 + 2 * nd * 8 + scratch * 8 + 8));
        ull* keys = reinterpret_cast<ull*>(res.p);
        ull* below0 = keys + Pn;
        ull* below1 = below0 + nd;
        ull* scr = below1 + nd;
        ull* cursor = scr + scratch;
        uint32_t* cnt = reinterpret_cast<uint32_t*>(cursor + 1);
        DSS_TRY(hipEventRecord(run.ev[0], s));
        DSS_TRY(hipMemsetAsync(keys, 0xff, Pn * 8, s));          // dss::SORT_PAD behind the scores
        DSS_TRY(hipMemsetAsync(cursor, 0, 8, s));
        DSS_TRY(hipMemsetAsync(counters + COUNTERS_U2, 0, 3 * NSETS * 8, s));
        hipLaunchKernelGGL(eval_compact_kernel, dim3(blocks(cap)), dim3(TPB), 0, s, (ull)cap, u64(t_key), cursor, (ull)nd, keys);
        DSS_TRY(hipGetLastError());
        DSS_TRY(dss::bitonic_sort(reinterpret_cast<uint64_t*>(keys), (int)Pn, s));
        hipLaunchKernelGGL(eval_lookup_kernel, dim3(blocks(nd)), dim3(TPB), 0, s, (ull)nd, keys, u64(t_key), t_cnt, (ull)(cap - 1), cnt, below0, below1);
        DSS_TRY(hipGetLastError());
        DSS_TRY(exclusive_scan(below0, nd, scr, s));
        DSS_TRY(exclusive_scan(below1, nd, scr, s));
        hipLaunchKernelGGL(eval_u2_kernel, dim3(blocks(nd)), dim3(TPB), 0, s, (ull)nd, cnt, below0, below1, counters + COUNTERS_U2);
        DSS_TRY(hipGetLastError());
        DSS_TRY(hipEventRecord(run.ev[1], s));
        DSS_TRY(hipMemcpyAsync(c + COUNTERS_U2, counters + COUNTERS_U2, 3 * NSETS * 8, hipMemcpyDeviceToHost, s));
        DSS_TRY(hipStreamSynchronize(s));
        dss::book(&t.ms[3], run.ev[0], run.ev[1]);
    } else {
        for (int k = 0; k < 3 * NSETS; ++k) c[COUNTERS_U2 + k] = 0;
    }
    const int width = 4 + 2 * ncf;
    for (int set = 0; set < NSETS; ++set) {
        const ull* sc = c + COUNTERS_SETS + set * SET_COUNTERS;
        int64_t* out = counts + (size_t)set * width;
        for (int k = 0; k < 4; ++k) out[k] = (int64_t)sc[k];
        for (int k = 0; k < ncf; ++k) { out[4 + k] = (int64_t)sc[C_CALLED + k]; out[4 + ncf + k] = (int64_t)sc[C_CORRECT + k]; }
        u2[set] = c[COUNTERS_U2 + 3 * set];
        pn[set] = (int64_t)c[COUNTERS_U2 + 3 * set + 1];
        nn[set] = (int64_t)c[COUNTERS_U2 + 3 * set + 2];
    }
    if (nrows) *nrows = rows_done;
    if (distinct) *distinct = (int64_t)nd;
    return DS_OK;
}

void Eval::end()
{
    if (run.close()) pending = -1;
}

bool reference(const char* text, int64_t nrows, const int64_t* begin, const int64_t* end, const uint8_t* flags, const uint8_t* mask, int32_t ncf,
               const double* cf, int32_t* status, double* p0, double* p1, int32_t* called, int64_t* counts, uint64_t* u2, int64_t* pn, int64_t* nn,
               std::string* err)
{
    if (nrows < 0 || !cutoffs_ok(ncf, cf) || !counts || !u2 || !pn || !nn ||
        (nrows > 0 && (!text || !begin || !end || !flags || !mask || !status || !p0 || !p1 || !called))) {
        seterr(err, -1, "ds_eval_reference: bad argument");
        return false;
    }
    const int width = 4 + 2 * ncf;
    for (int k = 0; k < NSETS * width; ++k) counts[k] = 0;
    std::map<uint64_t, std::array<uint32_t, 4>> scores;      // ascending keys are ascending scores
    for (int64_t r = 0; r < nrows; ++r) {
        if (begin[r] < 0 || end[r] < begin[r] || (mask[r] & ~(SET_BITS | TRUTH_BIT))) {
            seterr(err, -1, "ds_eval_reference: row " + std::to_string(r) + " has a bad span or byte");
            return false;
        }
        if (status[r] == ROW_GIVEN) {
            status[r] = ROW_OK;
            called[r] = called[r] != 0;
        } else {
            double a = 0.0, b = 0.0;
            int32_t lab = 0;
            status[r] = parse_row(text + begin[r], text + end[r], flags[r], &a, &b, &lab);
            p0[r] = a; p1[r] = b; called[r] = lab;
        }
        if (status[r] != ROW_OK) continue;
        const unsigned m = mask[r];
        const bool truth = (m & TRUTH_BIT) != 0, lab = called[r] != 0;
        for (int set = 0; set < NSETS; ++set) {
            if (!((m >> set) & 1u)) continue;
            int64_t* c = counts + (size_t)set * width;
            c[lab ? (truth ? C_TP : C_FP) : (truth ? C_FN : C_TN)] += 1;
            for (int k = 0; k < ncf; ++k) {
                if (!row_stands(p0[r], p1[r], cf[k])) continue;
                c[4 + k] += 1;
                if (row_correct(p0[r], p1[r], cf[k], truth)) c[4 + ncf + k] += 1;
            }
            if (score_finite(p1[r])) scores[score_key(p1[r])][count_index(set, truth)] += 1;
        }
    }
    for (int set = 0; set < NSETS; ++set) {
        uint64_t below = 0, sum = 0, p = 0, n = 0;
        for (const auto& kv : scores) {
            const uint64_t pos = kv.second[2 * set], neg = kv.second[2 * set + 1];
            sum += pos * (2 * below + neg);
            below += neg; p += pos; n += neg;
        }
        u2[set] = sum; pn[set] = (int64_t)p; nn[set] = (int64_t)n;
    }
    return true;
}

}  // namespace dse
