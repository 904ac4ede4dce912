// ds_freq.hip — per-site modification frequency on the GPU (call_freq --on gpu). A batch of result rows goes through four steps:
// freq_parse_kernel (one row per lane: ten columns tokenised, position, label and the two probabilities by the routines of
// ds_freq.h, the code the host checker runs), freq_insert_kernel (the used rows' exact keys chrom_id << 40 | pos into an
// open-addressing table by 64-bit atomicCAS; the slot is the site id, its first global row kept by atomicMin), a bitonic sort of
// the unique 64-bit keys site << 32 | row over the batch, and freq_accumulate_kernel (the lane at the head of a site's run adds
// the run's probabilities IN ROW ORDER into the site's running double sums: no floating-point atomics, the order of addition is
// the contract). The table lives across the batches of a run. Built with -ffp-contract=off and no fast-math (csrc/Makefile).
#include "ds_freq.h"
#include "../../include/deepsignal_hip.h"

#include <string.h>

#include <unordered_map>
#include <vector>

namespace dsf {

namespace {

constexpr int TPB = 256;
constexpr uint64_t SORT_PAD = ~(uint64_t)0;      // rows that take no part (unused, or past the batch) sort behind every site

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

__global__ __launch_bounds__(TPB) void freq_insert_kernel(int n, int P, double cf, unsigned long long row_base, const int32_t* chrom,
                                                          const int64_t* pos, const double* p0, const double* p1, const int32_t* status,
                                                          unsigned long long* t_key, unsigned long long* t_first, unsigned long long mask,
                                                          unsigned long long* sort, unsigned long long* counters)
{
    const int i = blockIdx.x * TPB + threadIdx.x;
    if (i >= P) return;
    unsigned long long sk = SORT_PAD;
    if (i < n) {
        if (status[i] != ROW_OK || !key_ok(chrom[i], pos[i])) {
            atomicAdd(&counters[3], 1ull);
        } else if (row_used(p0[i], p1[i], cf)) {
            const unsigned long long k = make_key(chrom[i], pos[i]);
            unsigned long long s = hash_key(k) & mask;
            bool found = false;
            for (unsigned long long probe = 0; probe <= mask; ++probe) {
                const unsigned long long prev = atomicCAS(&t_key[s], (unsigned long long)EMPTY, k);
                if (prev == EMPTY) { atomicAdd(&counters[0], 1ull); found = true; break; }
                if (prev == k) { found = true; break; }
                s = (s + 1) & mask;
            }
            if (found) {
                atomicMin(&t_first[s], row_base + (unsigned long long)i);
                atomicAdd(&counters[1], 1ull);
                sk = (s << 32) | (unsigned long long)i;
            } else {
                atomicAdd(&counters[2], 1ull);
            }
        }
    }
    sort[i] = sk;
}

// one compare-exchange step of the bitonic network over P = 2^q keys: partner distance j inside blocks of k
__global__ __launch_bounds__(TPB) void freq_bitonic_kernel(unsigned long long* a, int P, int j, int k)
{
    const int i = blockIdx.x * TPB + threadIdx.x;
    if (i >= P) return;
    const int l = i ^ j;
    if (l <= i) return;
    const unsigned long long x = a[i], y = a[l];
    const bool up = (i & k) == 0;
    if ((x > y) == up) { a[i] = y; a[l] = x; }
}

// the lane that sees the first key of a site's run walks the run in row order
__global__ __launch_bounds__(TPB) void freq_accumulate_kernel(int P, const unsigned long long* sorted, const double* p0, const double* p1,
                                                              const int32_t* met, double* t_sum0, double* t_sum1, int32_t* t_met,
                                                              int32_t* t_unmet)
{
    const int t = blockIdx.x * TPB + threadIdx.x;
    if (t >= P) return;
    const unsigned long long v = sorted[t];
    if (v == SORT_PAD) return;
    const unsigned long long site = v >> 32;
    if (t > 0 && (sorted[t - 1] >> 32) == site) return;
    double a = t_sum0[site], b = t_sum1[site];
    int32_t m = t_met[site], u = t_unmet[site];
    for (int q = t; q < P; ++q) {
        const unsigned long long w = sorted[q];
        if (w == SORT_PAD || (w >> 32) != site) break;
        const unsigned i = (unsigned)(w & 0xffffffffull);
        a += p0[i];
        b += p1[i];
        if (met[i]) ++m; else ++u;
    }
    t_sum0[site] = a; t_sum1[site] = b; t_met[site] = m; t_unmet[site] = u;
}

__global__ __launch_bounds__(TPB) void freq_result_kernel(unsigned long long cap, const unsigned long long* t_key, const unsigned long long* t_first,
                                                          const double* t_sum0, const double* t_sum1, const int32_t* t_met, const int32_t* t_unmet,
                                                          unsigned long long* cursor, unsigned long long out_cap, int64_t* first_row,
                                                          int32_t* chrom, int64_t* pos, double* sum0, double* sum1, int32_t* met, int32_t* unmet)
{
    const unsigned long long s = (unsigned long long)blockIdx.x * TPB + threadIdx.x;
    if (s >= cap) return;
    const unsigned long long k = t_key[s];
    if (k == EMPTY) return;
    const unsigned long long o = atomicAdd(cursor, 1ull);
    if (o >= out_cap) return;
    first_row[o] = (int64_t)t_first[s];
    chrom[o] = (int32_t)(k >> POS_BITS);
    pos[o] = (int64_t)(k & (((unsigned long long)1 << POS_BITS) - 1));
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
    if (!chrom || key_ok(chrom[i], pos[i])) st = call_value(act[(size_t)i * class_num], act[(size_t)i * class_num + 1], &a, &c);
    p0[i] = a; p1[i] = c;
    if (met) met[i] = pred[i] == 1;
    status[i] = st;
}

// after freq_insert_kernel, before the sort permutes `sort`: row i opened its site when it is the site's first row of the run
__global__ __launch_bounds__(TPB) void freq_opened_kernel(int n, unsigned long long row_base, const unsigned long long* sort,
                                                          const unsigned long long* t_first, int32_t* opened)
{
    const int i = blockIdx.x * TPB + threadIdx.x;
    if (i >= n) return;
    const unsigned long long sk = sort[i];
    opened[i] = sk != SORT_PAD && t_first[sk >> 32] == row_base + (unsigned long long)i;
}

// the table doubles: every occupied slot of the old table finds its slot in the new one (the same exact-key atomicCAS probe as
// freq_insert_kernel; the keys are distinct and the new table is at most a quarter full) and takes its sums and counts along
__global__ __launch_bounds__(TPB) void freq_rehash_kernel(unsigned long long old_cap, const unsigned long long* o_key, const unsigned long long* o_first,
                                                          const double* o_sum0, const double* o_sum1, const int32_t* o_met, const int32_t* o_unmet,
                                                          unsigned long long mask, unsigned long long* t_key, unsigned long long* t_first,
                                                          double* t_sum0, double* t_sum1, int32_t* t_met, int32_t* t_unmet,
                                                          unsigned long long* counters)
{
    const unsigned long long o = (unsigned long long)blockIdx.x * TPB + threadIdx.x;
    if (o >= old_cap) return;
    const unsigned long long k = o_key[o];
    if (k == EMPTY) return;
    unsigned long long s = hash_key(k) & mask;
    for (unsigned long long probe = 0; probe <= mask; ++probe) {
        if (atomicCAS(&t_key[s], (unsigned long long)EMPTY, k) == EMPTY) {
            t_first[s] = o_first[o]; t_sum0[s] = o_sum0[o]; t_sum1[s] = o_sum1[o]; t_met[s] = o_met[o]; t_unmet[s] = o_unmet[o];
            return;
        }
        s = (s + 1) & mask;
    }
    atomicAdd(&counters[2], 1ull);      // no slot: cannot happen below a load of one half; the next accumulate reports it
}

int blocks(uint64_t n) { return (int)((n + TPB - 1) / TPB); }

int seterr(std::string* err, int code, const std::string& msg)
{
    if (err) *err = msg;
    return code;
}

#define FQ(expr)                                                                                     \
    do {                                                                                             \
        hipError_t e_ = (expr);                                                                      \
        if (e_ != hipSuccess) {                                                                      \
            (void)hipGetLastError();                                                                 \
            return seterr(err, e_ == hipErrorOutOfMemory ? DS_ERR_NOMEM : DS_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(e_)); \
        }                                                                                            \
    } while (0)

void book(Freq* f, int slot, hipEvent_t a, hipEvent_t b)
{
    float ms = 0;
    if (hipEventElapsedTime(&ms, a, b) == hipSuccess) f->ms[slot] += ms; else (void)hipGetLastError();
}

double span(hipEvent_t a, hipEvent_t b)
{
    float ms = 0;
    if (hipEventElapsedTime(&ms, a, b) == hipSuccess) return ms;
    (void)hipGetLastError();
    return 0;
}

}  // namespace

hipError_t bitonic_sort(uint64_t* keys, int Pn, hipStream_t s)
{
    for (int k = 2; k <= Pn; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            hipLaunchKernelGGL(freq_bitonic_kernel, dim3(blocks(Pn)), dim3(TPB), 0, s, reinterpret_cast<unsigned long long*>(keys), Pn, j, k);
            const hipError_t e = hipGetLastError();
            if (e != hipSuccess) return e;
        }
    return hipSuccess;
}

int Freq::begin(int dev, int64_t total, int32_t batch, double prob_cf, std::string* err)
{
    if (s) return seterr(err, DS_ERR_INVALID, "ds_freq_begin: a run is open on this handle (ds_freq_end first)");
    if (total < 1 || total > MAX_TOTAL_ROWS) return seterr(err, DS_ERR_INVALID, "ds_freq_begin: total_rows must be in [1, 2^30]");
    if (batch < 1 || batch > (1 << 24)) return seterr(err, DS_ERR_INVALID, "ds_freq_begin: batch_rows must be in [1, 2^24]");
    if (prob_cf != prob_cf) return seterr(err, DS_ERR_INVALID, "ds_freq_begin: prob_cf is NaN");
    total_rows = total;
    streaming = false;
    cap = 64;
    while (cap < 2 * (uint64_t)total) cap <<= 1;
    return open(dev, batch, prob_cf, err);
}

int Freq::begin_stream(int dev, int64_t initial_slots, int32_t batch, double prob_cf, std::string* err)
{
    if (s) return seterr(err, DS_ERR_INVALID, "ds_freq_begin_stream: a run is open on this handle (ds_freq_end first)");
    if (initial_slots < 1 || initial_slots > 2 * MAX_TOTAL_ROWS) return seterr(err, DS_ERR_INVALID, "ds_freq_begin_stream: initial_slots must be in [1, 2^31]");
    if (batch < 1 || batch > (1 << 24)) return seterr(err, DS_ERR_INVALID, "ds_freq_begin_stream: batch_rows must be in [1, 2^24]");
    if (prob_cf != prob_cf) return seterr(err, DS_ERR_INVALID, "ds_freq_begin_stream: prob_cf is NaN");
    total_rows = MAX_TOTAL_ROWS;
    streaming = true;
    cap = 1;
    while (cap < (uint64_t)initial_slots) cap <<= 1;
    const int rc = open(dev, batch, prob_cf, err);
    if (rc) return rc;
    const size_t B = (size_t)batch;
    FQ(hipMalloc((void**)&d_pred, B * 4));
    FQ(hipMalloc((void**)&d_opened, B * 4));
    return DS_OK;
}

int Freq::open(int dev, int32_t batch, double prob_cf, std::string* err)
{
    device = dev;
    rows_done = 0; batch_rows = batch; pending = -1; cf = prob_cf;
    batches = 0; sites = 0; growths = 0; opened_out = nullptr;
    for (double& v : ms) v = 0;
    for (double& v : sms) v = 0;
    P = 1;
    while (P < batch) P <<= 1;
    FQ(hipSetDevice(device));
    FQ(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
    for (hipEvent_t& e : ev) FQ(hipEventCreate(&e));
    const size_t B = (size_t)batch;
    FQ(hipMalloc((void**)&t_key, cap * 8));
    FQ(hipMalloc((void**)&t_first, cap * 8));
    FQ(hipMalloc((void**)&t_sum0, cap * 8));
    FQ(hipMalloc((void**)&t_sum1, cap * 8));
    FQ(hipMalloc((void**)&t_met, cap * 4));
    FQ(hipMalloc((void**)&t_unmet, cap * 4));
    FQ(hipMalloc((void**)&counters, 8 * 8));
    FQ(hipMalloc((void**)&d_off, B * 8));
    FQ(hipMalloc((void**)&d_len, B * 4));
    FQ(hipMalloc((void**)&d_chrom, B * 4));
    FQ(hipMalloc((void**)&d_flags, B));
    FQ(hipMalloc((void**)&d_status, B * 4));
    FQ(hipMalloc((void**)&d_met, B * 4));
    FQ(hipMalloc((void**)&d_pos, B * 8));
    FQ(hipMalloc((void**)&d_p0, B * 8));
    FQ(hipMalloc((void**)&d_p1, B * 8));
    FQ(hipMalloc((void**)&d_sort, (size_t)P * 8));
    FQ(hipMemsetAsync(t_key, 0xff, cap * 8, s));
    FQ(hipMemsetAsync(t_first, 0xff, cap * 8, s));
    FQ(hipMemsetAsync(t_sum0, 0, cap * 8, s));
    FQ(hipMemsetAsync(t_sum1, 0, cap * 8, s));
    FQ(hipMemsetAsync(t_met, 0, cap * 4, s));
    FQ(hipMemsetAsync(t_unmet, 0, cap * 4, s));
    FQ(hipMemsetAsync(counters, 0, 8 * 8, s));
    FQ(hipStreamSynchronize(s));
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
    void* fresh[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    const size_t width[6] = {8, 8, 8, 8, 4, 4};
    const int fill[6] = {0xff, 0xff, 0, 0, 0, 0};
    hipError_t e = hipSuccess;
    for (int i = 0; i < 6 && e == hipSuccess; ++i) e = hipMalloc(&fresh[i], want * width[i]);
    if (e == hipSuccess) e = hipEventRecord(ev[0], s);
    for (int i = 0; i < 6 && e == hipSuccess; ++i) e = hipMemsetAsync(fresh[i], fill[i], want * width[i], s);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(freq_rehash_kernel, dim3(blocks(cap)), dim3(TPB), 0, s, (unsigned long long)cap, reinterpret_cast<const unsigned long long*>(t_key),
                           reinterpret_cast<const unsigned long long*>(t_first), t_sum0, t_sum1, t_met, t_unmet, (unsigned long long)(want - 1),
                           static_cast<unsigned long long*>(fresh[0]), static_cast<unsigned long long*>(fresh[1]), static_cast<double*>(fresh[2]),
                           static_cast<double*>(fresh[3]), static_cast<int32_t*>(fresh[4]), static_cast<int32_t*>(fresh[5]), counters);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipEventRecord(ev[1], s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        for (void* p : fresh) if (p) (void)hipFree(p);
        return seterr(err, e == hipErrorOutOfMemory ? DS_ERR_NOMEM : DS_ERR_HIP,
                      "ds_freq_push: growing the site table to " + std::to_string(want) + " slots: " + hipGetErrorString(e));
    }
    sms[1] += span(ev[0], ev[1]);
    void* old[6] = {t_key, t_first, t_sum0, t_sum1, t_met, t_unmet};
    for (void* p : old) (void)hipFree(p);
    t_key = static_cast<uint64_t*>(fresh[0]); t_first = static_cast<uint64_t*>(fresh[1]);
    t_sum0 = static_cast<double*>(fresh[2]); t_sum1 = static_cast<double*>(fresh[3]);
    t_met = static_cast<int32_t*>(fresh[4]); t_unmet = static_cast<int32_t*>(fresh[5]);
    cap = want;
    growths += doublings;       // several doublings at once are one rehash
    return DS_OK;
}

int Freq::push(int32_t n, const int32_t* chrom, const int64_t* pos, const float* act, int32_t class_num, const int32_t* pred, int32_t* status,
               int32_t* opened, std::string* err)
{
    if (!s || !streaming) return seterr(err, DS_ERR_INVALID, "ds_freq_push: no streaming run is open (ds_freq_begin_stream first)");
    if (pending >= 0) return seterr(err, DS_ERR_INVALID, "ds_freq_push: the previous batch has not been accumulated");
    if (!chrom || !pos || !act || !pred || !status || !opened) return seterr(err, DS_ERR_INVALID, "ds_freq_push: null argument");
    if (n < 1 || n > batch_rows) return seterr(err, DS_ERR_INVALID, "ds_freq_push: nrows must be in [1, batch_rows]");
    if (class_num < 2 || class_num > 1024) return seterr(err, DS_ERR_INVALID, "ds_freq_push: class_num must be in [2, 1024]");
    if (rows_done + n > total_rows) return seterr(err, DS_ERR_INVALID, "ds_freq_push: more than 2^30 rows in one run");
    FQ(hipSetDevice(device));
    const int rc = grow(n, err);
    if (rc) return rc;
    const size_t need = (size_t)n * (size_t)class_num;
    if (need > act_cap) {
        if (d_act) { FQ(hipFree(d_act)); d_act = nullptr; act_cap = 0; }
        const size_t want = (size_t)batch_rows * (size_t)class_num;
        FQ(hipMalloc((void**)&d_act, want * 4));
        act_cap = want;
    }
    FQ(hipEventRecord(ev[0], s));
    FQ(hipMemcpyAsync(d_chrom, chrom, (size_t)n * 4, hipMemcpyHostToDevice, s));
    FQ(hipMemcpyAsync(d_pos, pos, (size_t)n * 8, hipMemcpyHostToDevice, s));
    FQ(hipMemcpyAsync(d_act, act, need * 4, hipMemcpyHostToDevice, s));
    FQ(hipMemcpyAsync(d_pred, pred, (size_t)n * 4, hipMemcpyHostToDevice, s));
    FQ(hipEventRecord(ev[1], s));
    hipLaunchKernelGGL(freq_values_kernel, dim3(blocks(n)), dim3(TPB), 0, s, n, d_chrom, d_pos, d_act, class_num, d_pred, d_p0, d_p1, d_met, d_status);
    FQ(hipGetLastError());
    FQ(hipEventRecord(ev[2], s));
    FQ(hipMemcpyAsync(status, d_status, (size_t)n * 4, hipMemcpyDeviceToHost, s));
    FQ(hipEventRecord(ev[3], s));
    FQ(hipStreamSynchronize(s));
    book(this, 0, ev[0], ev[1]);
    sms[0] += span(ev[1], ev[2]);
    book(this, 0, ev[2], ev[3]);
    pending = n;
    opened_out = opened;
    return DS_OK;
}

int Freq::parse(const char* text, int32_t n, const int64_t* rb, const int64_t* re, const int32_t* chrom, const uint8_t* flags, int32_t* status,
                std::string* err)
{
    if (!s) return seterr(err, DS_ERR_INVALID, "ds_freq_parse: no run is open (ds_freq_begin first)");
    if (streaming) return seterr(err, DS_ERR_INVALID, "ds_freq_parse: the open run is a streaming one (ds_freq_push)");
    if (pending >= 0) return seterr(err, DS_ERR_INVALID, "ds_freq_parse: the previous batch has not been accumulated");
    if (!text || !rb || !re || !chrom || !flags || !status) return seterr(err, DS_ERR_INVALID, "ds_freq_parse: null argument");
    if (n < 1 || n > batch_rows) return seterr(err, DS_ERR_INVALID, "ds_freq_parse: nrows must be in [1, batch_rows]");
    if (rows_done + n > total_rows) return seterr(err, DS_ERR_INVALID, "ds_freq_parse: more rows than ds_freq_begin was told of");
    // the rows of a batch lie in file order inside one buffer: the bytes from the first row's begin to the last row's end travel as one copy
    if (rb[0] < 0) return seterr(err, DS_ERR_INVALID, "ds_freq_parse: row 0 has a bad span");
    std::vector<int64_t> off((size_t)n);
    std::vector<int32_t> len((size_t)n);
    const int64_t base = rb[0];
    for (int i = 0; i < n; ++i) {
        if (re[i] < rb[i] || (i > 0 && rb[i] < re[i - 1]) || re[i] - rb[i] > 0x7fffffff)
            return seterr(err, DS_ERR_INVALID, "ds_freq_parse: row " + std::to_string(i) + " has a bad span (rows must be ascending and disjoint)");
        off[(size_t)i] = rb[i] - base;
        len[(size_t)i] = (int32_t)(re[i] - rb[i]);
    }
    const size_t bytes = (size_t)(re[n - 1] - base);
    FQ(hipSetDevice(device));
    if (bytes > text_cap) {
        if (d_text) { FQ(hipFree(d_text)); d_text = nullptr; text_cap = 0; }
        const size_t want = bytes + bytes / 4 + 4096;
        FQ(hipMalloc((void**)&d_text, want));
        text_cap = want;
    }
    FQ(hipEventRecord(ev[0], s));
    if (bytes) FQ(hipMemcpyAsync(d_text, text + base, bytes, hipMemcpyHostToDevice, s));
    FQ(hipMemcpyAsync(d_off, off.data(), (size_t)n * 8, hipMemcpyHostToDevice, s));
    FQ(hipMemcpyAsync(d_len, len.data(), (size_t)n * 4, hipMemcpyHostToDevice, s));
    FQ(hipMemcpyAsync(d_chrom, chrom, (size_t)n * 4, hipMemcpyHostToDevice, s));
    FQ(hipMemcpyAsync(d_flags, flags, (size_t)n, hipMemcpyHostToDevice, s));
    FQ(hipEventRecord(ev[1], s));
    hipLaunchKernelGGL(freq_parse_kernel, dim3(blocks(n)), dim3(TPB), 0, s, d_text, d_off, d_len, d_chrom, d_flags, n, d_pos, d_p0, d_p1, d_met,
                       d_status);
    FQ(hipGetLastError());
    FQ(hipEventRecord(ev[2], s));
    FQ(hipMemcpyAsync(status, d_status, (size_t)n * 4, hipMemcpyDeviceToHost, s));
    FQ(hipEventRecord(ev[3], s));
    FQ(hipStreamSynchronize(s));      // also: off / len and the caller's arrays may go away now
    book(this, 0, ev[0], ev[1]);
    book(this, 1, ev[1], ev[2]);
    book(this, 0, ev[2], ev[3]);
    pending = n;
    return DS_OK;
}

int Freq::accumulate(int32_t m, const int32_t* row, const int32_t* chrom, const int64_t* pos, const double* p0, const double* p1,
                     const int32_t* met, std::string* err)
{
    if (!s) return seterr(err, DS_ERR_INVALID, "ds_freq_accumulate: no run is open (ds_freq_begin first)");
    if (pending < 0) return seterr(err, DS_ERR_INVALID, "ds_freq_accumulate: no parsed batch (ds_freq_parse first)");
    const int n = pending;
    if (m < 0 || m > n) return seterr(err, DS_ERR_INVALID, "ds_freq_accumulate: nover must be in [0, rows of the batch]");
    if (m > 0 && (!row || !chrom || !pos || !p0 || !p1 || !met)) return seterr(err, DS_ERR_INVALID, "ds_freq_accumulate: null argument");
    for (int k = 0; k < m; ++k) {
        if (row[k] < 0 || row[k] >= n || (k > 0 && row[k] <= row[k - 1]))
            return seterr(err, DS_ERR_INVALID, "ds_freq_accumulate: override rows must be ascending indices of the batch");
        if (!key_ok(chrom[k], pos[k]))
            return seterr(err, DS_ERR_INVALID, "ds_freq_accumulate: override " + std::to_string(k) + " has a chromosome id or position outside the key");
    }
    FQ(hipSetDevice(device));
    const size_t M = (size_t)m;
    // [pos | p0 | p1 | row | chrom | met], eight-byte arrays first
    const size_t need = M * (8 * 3 + 4 * 3);
    if (need > over_cap) {
        if (d_over) { FQ(hipFree(d_over)); d_over = nullptr; over_cap = 0; }
        FQ(hipMalloc((void**)&d_over, need + 4096));
        over_cap = need + 4096;
    }
    FQ(hipEventRecord(ev[0], s));
    if (m > 0) {
        int64_t* o_pos = reinterpret_cast<int64_t*>(d_over);
        double* o_p0 = reinterpret_cast<double*>(d_over + M * 8);
        double* o_p1 = reinterpret_cast<double*>(d_over + M * 16);
        int32_t* o_row = reinterpret_cast<int32_t*>(d_over + M * 24);
        int32_t* o_chrom = o_row + M;
        int32_t* o_met = o_chrom + M;
        FQ(hipMemcpyAsync(o_pos, pos, M * 8, hipMemcpyHostToDevice, s));
        FQ(hipMemcpyAsync(o_p0, p0, M * 8, hipMemcpyHostToDevice, s));
        FQ(hipMemcpyAsync(o_p1, p1, M * 8, hipMemcpyHostToDevice, s));
        FQ(hipMemcpyAsync(o_row, row, M * 4, hipMemcpyHostToDevice, s));
        FQ(hipMemcpyAsync(o_chrom, chrom, M * 4, hipMemcpyHostToDevice, s));
        FQ(hipMemcpyAsync(o_met, met, M * 4, hipMemcpyHostToDevice, s));
        hipLaunchKernelGGL(freq_override_kernel, dim3(blocks(M)), dim3(TPB), 0, s, m, o_row, o_chrom, o_pos, o_p0, o_p1, o_met, d_chrom, d_pos,
                           d_p0, d_p1, d_met, d_status);
        FQ(hipGetLastError());
    }
    FQ(hipEventRecord(ev[1], s));
    // the network sorts the smallest power of two that holds the batch
    int Pn = 1;
    while (Pn < n) Pn <<= 1;
    hipLaunchKernelGGL(freq_insert_kernel, dim3(blocks(Pn)), dim3(TPB), 0, s, n, Pn, cf, (unsigned long long)rows_done, d_chrom, d_pos, d_p0, d_p1,
                       d_status, reinterpret_cast<unsigned long long*>(t_key), reinterpret_cast<unsigned long long*>(t_first),
                       (unsigned long long)(cap - 1), reinterpret_cast<unsigned long long*>(d_sort), counters);
    FQ(hipGetLastError());
    if (streaming) {
        hipLaunchKernelGGL(freq_opened_kernel, dim3(blocks(n)), dim3(TPB), 0, s, n, (unsigned long long)rows_done, reinterpret_cast<const unsigned long long*>(d_sort),
                           reinterpret_cast<const unsigned long long*>(t_first), d_opened);
        FQ(hipGetLastError());
        FQ(hipMemcpyAsync(opened_out, d_opened, (size_t)n * 4, hipMemcpyDeviceToHost, s));
    }
    FQ(hipEventRecord(ev[2], s));
    FQ(bitonic_sort(d_sort, Pn, s));
    FQ(hipEventRecord(ev[3], s));
    hipLaunchKernelGGL(freq_accumulate_kernel, dim3(blocks(Pn)), dim3(TPB), 0, s, Pn, reinterpret_cast<const unsigned long long*>(d_sort), d_p0, d_p1,
                       d_met, t_sum0, t_sum1, t_met, t_unmet);
    FQ(hipGetLastError());
    FQ(hipEventRecord(ev[4], s));
    unsigned long long c[4] = {0, 0, 0, 0};
    FQ(hipMemcpyAsync(c, counters, sizeof(c), hipMemcpyDeviceToHost, s));
    FQ(hipStreamSynchronize(s));
    book(this, 0, ev[0], ev[1]);
    book(this, 3, ev[1], ev[2]);
    book(this, 2, ev[2], ev[3]);
    book(this, 3, ev[3], ev[4]);
    batches += 1;
    pending = -1;
    opened_out = nullptr;
    rows_done += n;
    sites = (int64_t)c[0];
    if (c[3]) return seterr(err, DS_ERR_INVALID, "ds_freq_accumulate: " + std::to_string(c[3]) + " row(s) of the batch were left to the caller and got no values");
    if (c[2]) return seterr(err, DS_ERR_INVALID, "ds_freq_accumulate: the site table is full");
    return DS_OK;
}

int64_t Freq::result(int64_t cap_sites, int64_t* first_row, int32_t* chrom, int64_t* pos, double* sum0, double* sum1, int32_t* met, int32_t* unmet,
                     int64_t* rows, int64_t* used, std::string* err)
{
    if (!s) return seterr(err, DS_ERR_INVALID, "ds_freq_result: no run is open (ds_freq_begin first)");
    if (pending >= 0) return seterr(err, DS_ERR_INVALID, "ds_freq_result: a parsed batch has not been accumulated");
    FQ(hipSetDevice(device));
    unsigned long long c[4] = {0, 0, 0, 0};
    FQ(hipMemcpy(c, counters, sizeof(c), hipMemcpyDeviceToHost));
    const int64_t nsites = (int64_t)c[0];
    if (rows) *rows = rows_done;
    if (used) *used = (int64_t)c[1];
    if (cap_sites == 0 && !first_row) return nsites;        // the size query
    if (!first_row || !chrom || !pos || !sum0 || !sum1 || !met || !unmet) return seterr(err, DS_ERR_INVALID, "ds_freq_result: null argument");
    if (cap_sites < nsites) return seterr(err, DS_ERR_INVALID, "ds_freq_result: " + std::to_string(nsites) + " sites, the arrays hold fewer");
    if (nsites == 0) return 0;
    const size_t N = (size_t)nsites;
    char* d_out = nullptr;
    FQ(hipMalloc((void**)&d_out, N * (8 * 4 + 4 * 3) + 8));
    unsigned long long* cursor = reinterpret_cast<unsigned long long*>(d_out);
    int64_t* o_first = reinterpret_cast<int64_t*>(d_out + 8);
    int64_t* o_pos = o_first + N;
    double* o_s0 = reinterpret_cast<double*>(o_pos + N);
    double* o_s1 = o_s0 + N;
    int32_t* o_chrom = reinterpret_cast<int32_t*>(o_s1 + N);
    int32_t* o_met = o_chrom + N;
    int32_t* o_unmet = o_met + N;
    hipError_t e = hipMemsetAsync(cursor, 0, 8, s);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(freq_result_kernel, dim3(blocks(cap)), dim3(TPB), 0, s, (unsigned long long)cap, reinterpret_cast<const unsigned long long*>(t_key),
                           reinterpret_cast<const unsigned long long*>(t_first), t_sum0, t_sum1, t_met, t_unmet, cursor, (unsigned long long)nsites,
                           o_first, o_chrom, o_pos, o_s0, o_s1, o_met, o_unmet);
        e = hipGetLastError();
    }
    auto d2h = [&](void* dst, const void* src, size_t b) { return hipMemcpyAsync(dst, src, b, hipMemcpyDeviceToHost, s); };
    if (e == hipSuccess) e = d2h(first_row, o_first, N * 8);
    if (e == hipSuccess) e = d2h(pos, o_pos, N * 8);
    if (e == hipSuccess) e = d2h(sum0, o_s0, N * 8);
    if (e == hipSuccess) e = d2h(sum1, o_s1, N * 8);
    if (e == hipSuccess) e = d2h(chrom, o_chrom, N * 4);
    if (e == hipSuccess) e = d2h(met, o_met, N * 4);
    if (e == hipSuccess) e = d2h(unmet, o_unmet, N * 4);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    (void)hipFree(d_out);
    if (e != hipSuccess) { (void)hipGetLastError(); return seterr(err, DS_ERR_HIP, std::string("ds_freq_result: ") + hipGetErrorString(e)); }
    return nsites;
}

void Freq::end()
{
    if (!s && !t_key) return;
    (void)hipSetDevice(device);
    if (s) (void)hipStreamSynchronize(s);
    void* ptrs[] = {t_key, t_first, t_sum0, t_sum1, t_met, t_unmet, counters, d_text, d_off, d_len, d_chrom, d_status, d_met, d_flags, d_pos,
                    d_p0, d_p1, d_sort, d_over, d_act, d_pred, d_opened};
    for (void* p : ptrs) if (p) (void)hipFree(p);
    t_key = t_first = nullptr; t_sum0 = t_sum1 = nullptr; t_met = t_unmet = nullptr; counters = nullptr;
    d_text = nullptr; d_off = nullptr; d_len = d_chrom = d_status = d_met = nullptr; d_flags = nullptr; d_pos = nullptr;
    d_p0 = d_p1 = nullptr; d_sort = nullptr; d_over = nullptr;
    d_act = nullptr; d_pred = d_opened = nullptr; opened_out = nullptr;
    text_cap = over_cap = act_cap = 0;
    for (hipEvent_t& e : ev) if (e) { (void)hipEventDestroy(e); e = nullptr; }
    if (s) { (void)hipStreamDestroy(s); s = nullptr; }
    (void)hipGetLastError();
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
    FQ(hipSetDevice(device));
    const size_t N = (size_t)n;
    char* d = nullptr;
    FQ(hipMalloc((void**)&d, N * (16 + 4 + 4 * (size_t)class_num)));
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
            if (!key_ok(chrom[r], pos[r])) {
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
        const uint64_t k = make_key(chrom[r], pos[r]);
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
