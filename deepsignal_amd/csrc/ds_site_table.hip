// ds_site_table.hip — the parts of the site table (ds_site_table.h) that are code of their own: the bitonic network's kernel and
// the host pieces of a run. Built with -ffp-contract=off and no fast-math like its users (csrc/Makefile).
#include "ds_site_table.h"

#include <algorithm>

namespace dss {

// one compare-exchange step of the bitonic network over P = 2^q keys: partner distance j inside blocks of k
__global__ __launch_bounds__(TPB) void site_bitonic_kernel(ull* a, int P, int j, int k)
{
    const int i = blockIdx.x * TPB + threadIdx.x;
    if (i >= P) return;
    const int l = i ^ j;
    if (l <= i) return;
    const ull x = a[i], y = a[l];
    const bool up = (i & k) == 0;
    if ((x > y) == up) { a[i] = y; a[l] = x; }
}

hipError_t bitonic_sort(uint64_t* keys, int Pn, hipStream_t s)
{
    for (int k = 2; k <= Pn; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            hipLaunchKernelGGL(site_bitonic_kernel, dim3(blocks(Pn)), dim3(TPB), 0, s, reinterpret_cast<ull*>(keys), Pn, j, k);
            const hipError_t e = hipGetLastError();
            if (e != hipSuccess) return e;
        }
    return hipSuccess;
}

hipError_t Run::open(int dev)
{
    device = dev;
    hipError_t e = hipSetDevice(device);
    if (e == hipSuccess) e = hipStreamCreateWithFlags(&s, hipStreamNonBlocking);
    for (hipEvent_t& v : ev)
        if (e == hipSuccess) e = hipEventCreate(&v);
    return e;
}

hipError_t Run::alloc(void** p, size_t bytes)
{
    if (std::find(held.begin(), held.end(), p) == held.end()) held.push_back(p);
    return hipMalloc(p, bytes);
}

bool Run::close()
{
    if (!s && held.empty()) return false;
    (void)hipSetDevice(device);
    if (s) (void)hipStreamSynchronize(s);
    for (void** p : held)
        if (*p) { (void)hipFree(*p); *p = nullptr; }
    held.clear();
    for (hipEvent_t& e : ev) if (e) { (void)hipEventDestroy(e); e = nullptr; }
    if (s) { (void)hipStreamDestroy(s); s = nullptr; }
    (void)hipGetLastError();
    return true;
}

hipError_t Buf::grow(Run* run, size_t need)
{
    if (need == 0 || (p && need <= cap)) return hipSuccess;      // p is null again after Run::close()
    if (p) {
        const hipError_t e = hipFree(p);
        if (e != hipSuccess) return e;
        p = nullptr;
    }
    cap = 0;
    const size_t want = need + need / 4 + 4096;
    const hipError_t e = run->alloc(&p, want);
    if (e == hipSuccess) cap = want;
    return e;
}

void book(double* ms, hipEvent_t a, hipEvent_t b)
{
    float v = 0;
    if (hipEventElapsedTime(&v, a, b) == hipSuccess) *ms += v; else (void)hipGetLastError();
}

int Batches::sizes(const char* route, int64_t min_total, int64_t total, int32_t batch, std::string* err)
{
    const std::string who = std::string(route) + "_begin: ";
    if (total < min_total || total > MAX_TOTAL_ROWS) return seterr(err, DS_ERR_INVALID, who + "total_rows must be in [" + std::to_string(min_total) + ", 2^30]");
    if (batch < 1 || batch > (1 << 24)) return seterr(err, DS_ERR_INVALID, who + "batch_rows must be in [1, 2^24]");
    total_rows = total; batch_rows = batch;
    return DS_OK;
}

int Batches::can_parse(const char* route, int32_t n, bool args_ok, std::string* err) const
{
    const std::string who = std::string(route) + "_parse: ";
    if (pending >= 0) return seterr(err, DS_ERR_INVALID, who + "the previous batch has not been accumulated");
    if (!args_ok) return seterr(err, DS_ERR_INVALID, who + "null argument");
    if (n < 1 || n > batch_rows) return seterr(err, DS_ERR_INVALID, who + "nrows must be in [1, batch_rows]");
    if (rows_done + n > total_rows) return seterr(err, DS_ERR_INVALID, who + "more rows than " + route + "_begin was told of");
    return DS_OK;
}

int Batches::can_accumulate(const char* route, std::string* err) const
{
    if (pending < 0) return seterr(err, DS_ERR_INVALID, std::string(route) + "_accumulate: no parsed batch (" + route + "_parse first)");
    return DS_OK;
}

int Batches::can_result(const char* route, std::string* err) const
{
    if (pending >= 0) return seterr(err, DS_ERR_INVALID, std::string(route) + "_result: a parsed batch has not been accumulated");
    return DS_OK;
}

hipError_t RowText::alloc(Run* run, size_t B)
{
    hipError_t e = run->alloc(&d_off, B * 8);
    if (e == hipSuccess) e = run->alloc(&d_len, B * 4);
    if (e == hipSuccess) e = run->alloc(&d_chrom, B * 4);
    if (e == hipSuccess) e = run->alloc(&d_flags, B);
    if (e == hipSuccess) e = run->alloc(&d_status, B * 4);
    return e;
}

// false: row *bad has a bad span. The rows of a batch lie in file order inside one buffer, ascending and disjoint, none of 2^31 bytes
bool row_spans(int32_t n, const int64_t* rb, const int64_t* re, std::vector<int64_t>* off, std::vector<int32_t>* len, int* bad)
{
    off->resize((size_t)n);
    len->resize((size_t)n);
    const int64_t base = rb[0];
    for (int i = 0; i < n; ++i) {
        if (re[i] < rb[i] || (i > 0 && rb[i] < re[i - 1]) || re[i] - rb[i] > 0x7fffffff) { *bad = i; return false; }
        (*off)[(size_t)i] = rb[i] - base;
        (*len)[(size_t)i] = (int32_t)(re[i] - rb[i]);
    }
    return true;
}

int RowText::upload(const char* who, Run* run, const char* src, int32_t n, const int64_t* rb, const int64_t* re, const int32_t* chrom,
                    const uint8_t* flags, std::string* err)
{
    if (rb[0] < 0) return seterr(err, DS_ERR_INVALID, std::string(who) + ": row 0 has a bad span");
    int bad = 0;
    if (!row_spans(n, rb, re, &off, &len, &bad))
        return seterr(err, DS_ERR_INVALID, std::string(who) + ": row " + std::to_string(bad) + " has a bad span (rows must be ascending and disjoint)");
    const int64_t base = rb[0];
    const size_t bytes = (size_t)(re[n - 1] - base);
    DSS_TRY(hipSetDevice(run->device));
    DSS_TRY(text.grow(run, bytes));
    DSS_TRY(hipEventRecord(run->ev[0], run->s));
    if (bytes) DSS_TRY(hipMemcpyAsync(text.p, src + base, bytes, hipMemcpyHostToDevice, run->s));
    DSS_TRY(hipMemcpyAsync(d_off, off.data(), (size_t)n * 8, hipMemcpyHostToDevice, run->s));
    DSS_TRY(hipMemcpyAsync(d_len, len.data(), (size_t)n * 4, hipMemcpyHostToDevice, run->s));
    DSS_TRY(hipMemcpyAsync(d_chrom, chrom, (size_t)n * 4, hipMemcpyHostToDevice, run->s));
    DSS_TRY(hipMemcpyAsync(d_flags, flags, (size_t)n, hipMemcpyHostToDevice, run->s));
    DSS_TRY(hipEventRecord(run->ev[1], run->s));
    return DS_OK;
}

int RowText::finish(Run* run, int32_t n, int32_t* status, double* copy_ms, double* kernel_ms, std::string* err)
{
    DSS_TRY(hipGetLastError());
    DSS_TRY(hipEventRecord(run->ev[2], run->s));
    DSS_TRY(hipMemcpyAsync(status, d_status, (size_t)n * 4, hipMemcpyDeviceToHost, run->s));
    DSS_TRY(hipEventRecord(run->ev[3], run->s));
    DSS_TRY(hipStreamSynchronize(run->s));      // also: off / len and the caller's arrays may go away now
    book(copy_ms, run->ev[0], run->ev[1]);
    book(kernel_ms, run->ev[1], run->ev[2]);
    book(copy_ms, run->ev[2], run->ev[3]);
    return DS_OK;
}

size_t Columns::lay(char* base, size_t n, const Column* cols, int ncols)
{
    size_t at = 0;
    for (int c = 0; c < ncols; ++c) { dev[c] = base ? base + at : nullptr; at += n * cols[c].width; }
    return at;
}

hipError_t Columns::carve(Run* run, size_t n, const Column* cols, int ncols)
{
    hipError_t e = hipMalloc((void**)&d_out, 8 + lay(nullptr, n, cols, ncols));
    if (e != hipSuccess) { d_out = nullptr; return e; }
    lay(d_out + 8, n, cols, ncols);
    e = hipMemsetAsync(d_out, 0, 8, run->s);
    if (e != hipSuccess) { (void)hipFree(d_out); d_out = nullptr; }
    return e;
}

hipError_t Columns::fetch(Run* run, hipError_t e, size_t n, const Column* cols, int ncols)
{
    for (int c = 0; c < ncols && e == hipSuccess; ++c) e = hipMemcpyAsync(cols[c].host, dev[c], n * cols[c].width, hipMemcpyDeviceToHost, run->s);
    if (e == hipSuccess) e = hipStreamSynchronize(run->s);
    (void)hipFree(d_out);
    d_out = nullptr;
    if (e != hipSuccess) (void)hipGetLastError();
    return e;
}

hipError_t Columns::stage(Run* run, Buf* buf, size_t n, const Column* cols, int ncols)
{
    hipError_t e = hipSetDevice(run->device);
    if (e == hipSuccess) e = buf->grow(run, lay(nullptr, n, cols, ncols));
    if (e == hipSuccess) e = hipEventRecord(run->ev[0], run->s);
    lay(buf->p, n, cols, ncols);
    for (int c = 0; c < ncols && e == hipSuccess && n > 0; ++c) e = hipMemcpyAsync(dev[c], cols[c].host, n * cols[c].width, hipMemcpyHostToDevice, run->s);
    return e;
}

int finish_batch(Run* run, const ull* counters, ull* c, double* copy_ms, double* sort_ms, double* table_ms, std::string* err)
{
    DSS_TRY(hipGetLastError());
    DSS_TRY(hipEventRecord(run->ev[4], run->s));
    DSS_TRY(hipMemcpyAsync(c, counters, 4 * sizeof(ull), hipMemcpyDeviceToHost, run->s));
    DSS_TRY(hipStreamSynchronize(run->s));
    book(copy_ms, run->ev[0], run->ev[1]);
    book(table_ms, run->ev[1], run->ev[2]);
    book(sort_ms, run->ev[2], run->ev[3]);
    book(table_ms, run->ev[3], run->ev[4]);
    return DS_OK;
}

int batch_verdict(const char* who, const ull* c, std::string* err)
{
    if (c[3]) return seterr(err, DS_ERR_INVALID, std::string(who) + ": " + std::to_string(c[3]) + " row(s) of the batch were left to the caller and got no values");
    if (c[2]) return seterr(err, DS_ERR_INVALID, std::string(who) + ": the site table is full");
    return DS_OK;
}

}  // namespace dss
