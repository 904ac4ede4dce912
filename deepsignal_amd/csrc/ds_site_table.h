// ds_site_table.h — the keyed accumulation under call_freq --on gpu (ds_freq.hip) and combine_strands --on gpu (ds_combine.hip): an
// open-addressing table of exact 64-bit site keys whose slot is the site id, a bitonic sort of site << 32 | row over a batch, and a
// walk in which the lane at the head of a site's run adds the run IN ROW ORDER (no floating-point atomics: the order of addition is
// the contract). Here: the key, the device routines both routes' kernels are built from, and the plain host pieces of a run (its
// device allocations, its stream and events, the call order of its batches, its time tally, a batch's row text, the result's
// columns); evaluate --on gpu (ds_eval.hip) takes the table, the sort and the host pieces. What a site holds is the route's own.
// Not part of the public ABI.
#pragma once
#include "ds_tsv_device.h"
#include "../../include/deepsignal_hip.h"

#include <string>
#include <vector>

namespace dss {

// ---- the key --------------------------------------------------------------------------------------------------------------
constexpr int POS_BITS = 40;       // a site key is chrom_id << 40 | pos ...
constexpr int64_t POS_LIMIT = (int64_t)1 << POS_BITS;
constexpr int32_t CHROM_LIMIT = 1 << 23;         // ... with 23 bits of chromosome id, so no key is the empty slot's all-ones
constexpr uint64_t EMPTY = ~(uint64_t)0;
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

// ---- device side ----------------------------------------------------------------------------------------------------------
constexpr int TPB = 256;
constexpr uint64_t SORT_PAD = ~(uint64_t)0;      // rows that take no part (unused, or past the batch) sort behind every site
typedef unsigned long long ull;
constexpr ull NO_SLOT = ~0ull;
inline ull* u64(uint64_t* p) { return reinterpret_cast<ull*>(p); }
inline int blocks(uint64_t n) { return (int)((n + TPB - 1) / TPB); }

// The slot of key k in t_key (mask + 1 slots, a power of two), claimed by 64-bit atomicCAS when no lane has yet: NO_SLOT when the
// probe sequence has gone round the table. *opened: this lane is the one that claimed it.
__device__ __forceinline__ ull find_slot(ull* t_key, ull mask, ull k, bool* opened)
{
    ull s = hash_key(k) & mask;
    for (ull probe = 0; probe <= mask; ++probe) {
        const ull prev = atomicCAS(&t_key[s], (ull)EMPTY, k);
        if (prev == EMPTY || prev == k) { *opened = prev == EMPTY; return s; }
        s = (s + 1) & mask;
    }
    *opened = false;
    return NO_SLOT;
}

// Row i of the batch with key k goes into the table: counters[0] sites, [1] rows added, [2] probe sequences that found no slot.
// Returns the row's slot (NO_SLOT: none) and its sort key slot << 32 | row (SORT_PAD: none).
__device__ __forceinline__ ull insert_row(ull* t_key, ull mask, ull k, int i, ull* counters, ull* sort_key)
{
    bool opened;
    const ull s = find_slot(t_key, mask, k, &opened);
    // each counter at an address the whole wave shares: the compiler folds a wave's additions into one atomic. An index computed
    // per lane would cost one atomic per row on one address (measured: 12 ms for a batch of a million rows against 0.3)
    if (opened) atomicAdd(&counters[0], 1ull);
    if (s == NO_SLOT) {
        atomicAdd(&counters[2], 1ull);
        *sort_key = SORT_PAD;
    } else {
        atomicAdd(&counters[1], 1ull);
        *sort_key = (s << 32) | (ull)i;
    }
    return s;
}

// Lane t of the walk over P sorted keys: when sorted[t] is the first key of a site's run, *site is that site and add(i) is called
// for the run's rows i in ascending sorted order, which is row order. The route loads the site's sums before and stores them after.
__device__ __forceinline__ bool run_head(const ull* sorted, int P, int t, ull* site)
{
    if (t >= P) return false;
    const ull v = sorted[t];
    if (v == SORT_PAD) return false;
    *site = v >> 32;
    return t == 0 || (sorted[t - 1] >> 32) != *site;
}

template <typename Add>
__device__ __forceinline__ void walk_run(const ull* sorted, int P, int t, ull site, Add add)
{
    for (int q = t; q < P; ++q) {
        const ull w = sorted[q];
        if (w == SORT_PAD || (w >> 32) != site) break;
        add((unsigned)(w & 0xffffffffull));
    }
}

// Slot s of a table of cap slots into the result: false for an empty slot or when the arrays are full, else *o is the site's row
// of the result and its key is unpacked there.
__device__ __forceinline__ bool compact_slot(ull cap, const ull* t_key, ull s, ull* cursor, ull out_cap, int32_t* chrom, int64_t* pos, ull* o)
{
    if (s >= cap) return false;
    const ull k = t_key[s];
    if (k == EMPTY) return false;
    *o = atomicAdd(cursor, 1ull);
    if (*o >= out_cap) return false;
    chrom[*o] = (int32_t)(k >> POS_BITS);
    pos[*o] = (int64_t)(k & (((ull)1 << POS_BITS) - 1));
    return true;
}

// site_bitonic_kernel's network over Pn = 2^q keys on stream s, ascending: the first launch error, or hipSuccess
hipError_t bitonic_sort(uint64_t* keys, int Pn, hipStream_t s);

// ---- host side ------------------------------------------------------------------------------------------------------------
inline int seterr(std::string* err, int code, const std::string& msg) { if (err) *err = msg; return code; }

// inside a function that has `std::string* err` and returns a DS_* code
#define DSS_TRY(expr)                                                                                \
    do {                                                                                             \
        hipError_t e_ = (expr);                                                                      \
        if (e_ != hipSuccess) {                                                                      \
            (void)hipGetLastError();                                                                 \
            return dss::seterr(err, e_ == hipErrorOutOfMemory ? DS_ERR_NOMEM : DS_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(e_)); \
        }                                                                                            \
    } while (0)

// One run's stream, the events its device times are read from, and its device allocations. alloc() keeps the address of the
// caller's pointer, so close() frees whatever each pointer holds by then and leaves it null: safe after a begin() that stopped half
// way, and twice. close() also waits for the stream and destroys it and the events; false: nothing was open.
struct Run {
    int device = 0;
    hipStream_t s = nullptr;
    hipEvent_t ev[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
    std::vector<void**> held;
    hipError_t open(int device);
    hipError_t alloc(void** p, size_t bytes);
    template <typename T> hipError_t alloc(T** p, size_t bytes) { return alloc(reinterpret_cast<void**>(p), bytes); }
    // ... and filled with the byte `fill` on the stream
    template <typename T> hipError_t alloc(T** p, size_t bytes, int fill)
    {
        const hipError_t e = alloc(p, bytes);
        return e == hipSuccess ? hipMemsetAsync(*p, fill, bytes, s) : e;
    }
    bool close();
};
// *ms += the device milliseconds from a to b
void book(double* ms, hipEvent_t a, hipEvent_t b);

// What a ds_get_*_times getter reports: n[0] = the batches timed (n[1], where there is one, what else was counted) and their summed
// device milliseconds. A run owns one; the handle owns the sum of the runs ended. take(): this tally with the open run's on top, and
// on reset both are cleared.
template <int K, int C = 1>
struct Times {
    int64_t n[C] = {};
    double ms[K] = {};
    void add(const Times& o)
    {
        for (int i = 0; i < C; ++i) n[i] += o.n[i];
        for (int i = 0; i < K; ++i) ms[i] += o.ms[i];
    }
    Times take(int32_t reset, Times* open = nullptr)
    {
        Times sum = *this;
        if (open) sum.add(*open);
        if (reset) {
            *this = Times();
            if (open) *open = Times();
        }
        return sum;
    }
    int get(int32_t reset, int64_t* count, double* out, Times* open = nullptr)
    {
        if (!count || !out) return DS_ERR_INVALID;
        const Times t = take(reset, open);
        *count = t.n[0];
        for (int i = 0; i < K; ++i) out[i] = t.ms[i];
        return DS_OK;
    }
};

// The call order of a run's batches: parse, accumulate, parse, ... and a result only between batches. The checks that open the three
// calls of `route` ("ds_freq"): DS_OK, or DS_ERR_INVALID with the refusal in *err and nothing changed.
struct Batches {
    int64_t total_rows = 0, rows_done = 0;
    int32_t batch_rows = 0, pending = -1;      // pending = rows parsed, not accumulated
    // begin(): total_rows in [min_total, 2^30] and batch_rows in [1, 2^24]; no row of the run has been seen
    int sizes(const char* route, int64_t min_total, int64_t total, int32_t batch, std::string* err);
    // parse() of n rows; args_ok: none of the call's arrays is null
    int can_parse(const char* route, int32_t n, bool args_ok, std::string* err) const;
    int can_accumulate(const char* route, std::string* err) const;
    int can_result(const char* route, std::string* err) const;
};

// a buffer that grows to at least `need` bytes, with a quarter of slack; what it held is gone after a growth
struct Buf {
    char* p = nullptr;
    size_t cap = 0;
    hipError_t grow(Run* run, size_t need);
};

constexpr unsigned FLAG_HOST = 1;  // ds_freq_locate: the row is stripped or decoded differently by Python (leading / trailing whitespace, a
                                   // non-ASCII byte, a carriage return, a blank row)
// the span check alone, no device needed: each row's offset from rb[0] and its length; false with *bad = the first row whose span is
// reversed, overlaps the row before it or holds 2^31 bytes or more
bool row_spans(int32_t n, const int64_t* rb, const int64_t* re, std::vector<int64_t>* off, std::vector<int32_t>* len, int* bad);

// A batch's rows as text: the bytes from the first row's begin to the last row's end in one copy, each row's offset and length, and
// chrom / flags per row. upload() checks the spans (`who` opens its messages), records ev[0], copies, records ev[1]; the host
// vectors stay until the caller has synchronised. finish(), after the route's kernel: its launch status, ev[2], the status column
// copied back, ev[3], a wait for the stream; the copies are booked under *copy_ms and ev[1] .. ev[2] under *kernel_ms.
struct RowText {
    Buf text;
    int64_t* d_off = nullptr;
    int32_t *d_len = nullptr, *d_chrom = nullptr, *d_status = nullptr;
    uint8_t* d_flags = nullptr;
    std::vector<int64_t> off;
    std::vector<int32_t> len;
    hipError_t alloc(Run* run, size_t batch_rows);
    int upload(const char* who, Run* run, const char* text, int32_t n, const int64_t* rb, const int64_t* re, const int32_t* chrom, const uint8_t* flags,
               std::string* err);
    int finish(Run* run, int32_t n, int32_t* status, double* copy_ms, double* kernel_ms, std::string* err);
};

// Host columns of n elements each and their places on the device, back to back in the given order: widths descending, so that every
// column is aligned. The result: carve() allocates [cursor | columns] and zeroes the cursor; fetch() -- after the route's result
// kernel, `launched` its launch status -- copies each column to its host array, waits, and frees the allocation whatever happened.
// The caller's values of a batch's ROW_HOST rows: stage() grows `buf` to hold the columns, records ev[0] and copies them in.
struct Column {
    void* host;
    size_t width;
};
template <typename T> Column col(const T* host) { return {const_cast<T*>(host), sizeof(T)}; }
struct Columns {
    char* d_out = nullptr;
    void* dev[10];
    ull* cursor() const { return reinterpret_cast<ull*>(d_out); }
    template <typename T> T* at(int c) const { return static_cast<T*>(dev[c]); }
    size_t lay(char* base, size_t n, const Column* cols, int ncols);      // dev[c] = column c's place from `base` on; returns the bytes of all
    hipError_t carve(Run* run, size_t n, const Column* cols, int ncols);
    hipError_t fetch(Run* run, hipError_t launched, size_t n, const Column* cols, int ncols);
    hipError_t stage(Run* run, Buf* buf, size_t n, const Column* cols, int ncols);
};

// override k of a batch of n rows names a row of the batch behind the one before it
inline bool override_row_ok(const int32_t* row, int k, int n) { return row[k] >= 0 && row[k] < n && (k == 0 || row[k] > row[k - 1]); }

// The end of accumulate(), after the walk's launch: its launch status, ev[4], counters[0 .. 3] copied to c, a wait for the stream; ev[0]
// .. ev[1] is booked under *copy_ms, the sort ev[2] .. ev[3] under *sort_ms, the insert and the walk on either side of it under *table_ms.
int finish_batch(Run* run, const ull* counters, ull* c, double* copy_ms, double* sort_ms, double* table_ms, std::string* err);
// what the counters say of the batch: rows left to the caller that got no values, a full table; `who` opens the message
int batch_verdict(const char* who, const ull* c, std::string* err);

}  // namespace dss
