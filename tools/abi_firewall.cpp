// abi_firewall.cpp — fault injection at the C ABI (include/deepsignal_hip.h: no entry point throws; csrc/ds_abi.h).
//
// The program replaces the global operator new with one that counts and can fail its N-th call after arming, with
// std::bad_alloc or with a std::runtime_error (the handler's second arm). libdeepsignal_hip.so takes operator new from
// the program it is loaded into, so every allocation its entry points make goes through the counter. For each entry point that
// needs no GPU: one plain call counts the allocations and keeps the results; then the call is repeated once per allocation and
// per exception kind with that allocation failing -- a fresh reader per repetition -- and must return the handler's code and,
// where the entry has an error text, the handler's text, and its reader must close; a last plain call must give the first
// call's bytes again. An entry whose plain call allocates nothing fails the program unless it is on NO_ALLOC below: a sweep
// that injects nowhere would pass without testing anything (interposition into the library did not take).
// Host code only: no GPU call, no sanitizer. tests/test_abi_firewall.py builds and runs it:
//   g++ -O1 -g -std=c++17 -pthread tools/abi_firewall.cpp deepsignal_amd/libdeepsignal_hip.so -Wl,-rpath,$PWD/deepsignal_amd -o abi_firewall
//   ./abi_firewall <scratch directory>
// ABI_FIREWALL_NO_INJECT (compile-time): the same calls with the allocator left alone, for the stand-alone ASan / UBSan build of
// the ds_io.cpp half (ABI_FIREWALL_IO_ONLY leaves the entry points of ds_engine.cpp out, so that no .so is needed):
//   hipcc --offload-arch=gfx950 -std=c++17 -O1 -g -Xarch_host -fsanitize=address,undefined -DABI_FIREWALL_NO_INJECT -DABI_FIREWALL_IO_ONLY \
//         -x hip tools/abi_firewall.cpp deepsignal_amd/csrc/ds_io.cpp -o abi_firewall_asan && ./abi_firewall_asan <scratch directory>
#include "../include/deepsignal_hip.h"

#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <new>
#include <stdexcept>
#include <string>
#include <vector>

// ---- the allocator ------------------------------------------------------------------------------------------------------------
enum Kind { BAD_ALLOC = 0, RUNTIME_ERROR = 1 };
static std::atomic<bool> g_armed(false), g_fired(false);
static std::atomic<long> g_count(0), g_fail_at(-1);      // allocations since arming; the one that fails (-1: none)
static std::atomic<int> g_kind(BAD_ALLOC);

#ifndef ABI_FIREWALL_NO_INJECT
void* operator new(size_t n)
{
    if (g_armed.load()) {
        const long k = g_count.fetch_add(1);
        if (k == g_fail_at.load()) {
            g_fired = true;
            if (g_kind.load() == RUNTIME_ERROR) throw std::runtime_error("injected");      // (its own string allocates: counted, never failed)
            throw std::bad_alloc();
        }
    }
    if (void* p = malloc(n ? n : 1)) return p;
    throw std::bad_alloc();
}
void* operator new[](size_t n) { return operator new(n); }
void operator delete(void* p) noexcept { free(p); }
void operator delete[](void* p) noexcept { free(p); }
void operator delete(void* p, size_t) noexcept { free(p); }
void operator delete[](void* p, size_t) noexcept { free(p); }
#endif

static void arm() { g_count = 0; g_fired = false; g_armed = true; }
static void disarm() { g_armed = false; }

// ---- the cases ----------------------------------------------------------------------------------------------------------------
typedef std::vector<unsigned char> Bytes;
template <class T>
static void put(Bytes& out, const T* p, size_t n) { const unsigned char* b = (const unsigned char*)p; out.insert(out.end(), b, b + n * sizeof(T)); }
template <class T>
static void put(Bytes& out, const std::vector<T>& v) { put(out, v.data(), v.size()); }

enum Sink { NONE, READER, THREAD };      // where the entry leaves its text: nowhere, ds_tsv_error, ds_last_error(NULL)
struct Case {
    const char* name;
    Sink sink;
    // arms just before the entry point under test and disarms just behind it; everything the call wrote goes to *out, the
    // text of its sink to *err (read before the reader is closed)
    std::function<int64_t(Bytes* out, std::string* err)> call;
};

// entry points whose plain call is known to allocate nothing (they write into the caller's arrays only)
static const char* const NO_ALLOC[] = {"ds_tsv_take_lines", "ds_tsv_set_range", "ds_format_rows", "ds_fasta_locate", "ds_eval_locate",
                                       "ds_parse_text_reference", "ds_motif_reference"};
static bool no_alloc_listed(const char* name)
{
    for (const char* n : NO_ALLOC)
        if (strcmp(name, n) == 0) return true;
    return false;
}

static const int K = 3, S = 4;      // kmer_len, signal_len of the feature files

// a feature TSV of `rows` rows in 2 reads
static std::string feature_file(const std::string& dir, const char* name, int rows)
{
    const std::string path = dir + "/" + name;
    FILE* f = fopen(path.c_str(), "wb");
    if (!f) { printf("cannot write %s\n", path.c_str()); exit(2); }
    for (int i = 0; i < rows; ++i)
        fprintf(f, "chr1\t%d\t+\t%d\tread%d\tt\tACG\t0.1,0.2,0.3\t0.01,0.02,0.03\t3,4,5\t0.5,-0.5,0.25,1.5\t%d\n", 100 + i, 100 + i, i < rows / 2 ? 0 : 1, i & 1);
    fclose(f);
    return path;
}

// a reader on `path` with `located` = the rows of its first item, opened and located without injection
static ds_tsv* located_reader(const std::string& path, int nthreads, int64_t* located)
{
    ds_tsv* t = nullptr;
    if (ds_tsv_open(path.c_str(), K, S, nthreads, &t) != DS_OK) { printf("ds_tsv_open failed on %s\n", path.c_str()); exit(2); }
    *located = ds_tsv_locate(t, 16);
    return t;
}

static int64_t parse_case(const std::string& path, int nthreads, int64_t short_by, Bytes* out, std::string* err)
{
    int64_t n = 0;
    ds_tsv* t = located_reader(path, nthreads, &n);
    std::vector<int32_t> kmer((size_t)n * K), labels((size_t)n);
    std::vector<float> means((size_t)n * K), stds((size_t)n * K), lens((size_t)n * K), signals((size_t)n * S);
    arm();
    const int64_t rc = ds_tsv_parse_into(t, n - short_by, kmer.data(), means.data(), stds.data(), lens.data(), signals.data(), labels.data());
    disarm();
    *err = ds_tsv_error(t);
    if (rc > 0) {
        put(*out, kmer); put(*out, means); put(*out, stds); put(*out, lens); put(*out, signals); put(*out, labels);
        put(*out, ds_tsv_info_offsets(t), (size_t)rc + 1);
        put(*out, ds_tsv_info(t), (size_t)ds_tsv_info_offsets(t)[rc]);
    }
    ds_tsv_close(t);
    return rc;
}

static const char CALLS[] =        // call_mods result rows: two chromosomes, a repeated site, a row below the threshold
    "chr1\t10\t+\t10\tr0\tt\t0.1\t0.9\t1\tACG\n"
    "chr1\t10\t+\t10\tr1\tt\t0.8\t0.2\t0\tACG\n"
    "chr2\t7\t-\t3\tr2\tt\t0.5\t0.5\t1\tCCG\n"
    "chr2\t8\t-\t2\tr3\tc\t0.25\t0.75\t1\tTCG";
static const char GENOME[] = "ACGTCGAA";      // CG at 1 and 4
static const char TABLE[] =        // frequency-table rows on GENOME: a '+' C, its '-' partner one base down, a position that is no CG
    "chr1\t1\t+\t1\t0.5\t1.5\t2\t0\t2\t1.0\tACG\n"
    "chr1\t2\t-\t5\t0.25\t0.75\t1\t0\t1\t1.0\tACG\n"
    "chr1\t6\t+\t6\t1.0\t0.0\t0\t1\t1\t0.0\tGAA";

static void add_io_cases(std::vector<Case>& cases, const std::string& dir)
{
    const std::string small = feature_file(dir, "four_rows.tsv", 4);        // parsed on the calling thread (one grain of 16 rows)
    const std::string team = feature_file(dir, "team_rows.tsv", 33);        // three grains: the team of 2 helpers starts and runs
    cases.push_back({"ds_tsv_open", NONE, [=](Bytes* out, std::string*) {
        ds_tsv* t = nullptr;
        arm();
        const int rc = ds_tsv_open(small.c_str(), K, S, 2, &t);
        disarm();
        if (rc == DS_OK) { const int64_t size = ds_tsv_size(t); put(*out, &size, 1); }
        else if (t) { printf("ds_tsv_open: a reader came back with an error\n"); exit(1); }
        ds_tsv_close(t);
        return (int64_t)rc;
    }});
    cases.push_back({"ds_tsv_locate", READER, [=](Bytes* out, std::string* err) {
        ds_tsv* t = nullptr;
        if (ds_tsv_open(small.c_str(), K, S, 2, &t) != DS_OK) exit(2);
        arm();
        const int64_t rc = ds_tsv_locate(t, 16);
        disarm();
        *err = ds_tsv_error(t);
        put(*out, &rc, 1);
        ds_tsv_close(t);
        return rc;
    }});
    cases.push_back({"ds_tsv_locate (a row of four columns)", READER, [=](Bytes*, std::string* err) {
        const std::string bad = dir + "/short_row.tsv";
        FILE* f = fopen(bad.c_str(), "wb");
        fputs("chr1\t1\t+\t1\n", f);
        fclose(f);
        ds_tsv* t = nullptr;
        if (ds_tsv_open(bad.c_str(), K, S, 2, &t) != DS_OK) exit(2);
        arm();
        const int64_t rc = ds_tsv_locate(t, 16);
        disarm();
        *err = ds_tsv_error(t);
        ds_tsv_close(t);
        return rc;
    }});
    cases.push_back({"ds_tsv_parse_into", READER, [=](Bytes* out, std::string* err) { return parse_case(small, 2, 0, out, err); }});
    cases.push_back({"ds_tsv_parse_into (33 rows, the team runs)", READER, [=](Bytes* out, std::string* err) { return parse_case(team, 3, 0, out, err); }});
    cases.push_back({"ds_tsv_parse_into (arrays one row short)", READER, [=](Bytes* out, std::string* err) { return parse_case(small, 2, 1, out, err); }});
    cases.push_back({"ds_tsv_next", READER, [=](Bytes* out, std::string* err) {
        ds_tsv* t = nullptr;
        if (ds_tsv_open(team.c_str(), K, S, 3, &t) != DS_OK) exit(2);
        arm();
        const int64_t rc = ds_tsv_next(t, 16);
        disarm();
        *err = ds_tsv_error(t);
        if (rc > 0) { put(*out, ds_tsv_kmer(t), (size_t)rc * K); put(*out, ds_tsv_signals(t), (size_t)rc * S); put(*out, ds_tsv_labels(t), (size_t)rc); }
        ds_tsv_close(t);
        return rc;
    }});
    for (int short_by = 0; short_by < 2; ++short_by)
        cases.push_back({short_by ? "ds_tsv_take_lines (arrays one row short)" : "ds_tsv_take_lines", READER, [=](Bytes* out, std::string* err) {
            int64_t n = 0;
            ds_tsv* t = located_reader(small, 2, &n);
            std::vector<int64_t> b((size_t)n), e((size_t)n);
            arm();
            const int64_t rc = ds_tsv_take_lines(t, n - short_by, b.data(), e.data());
            disarm();
            *err = ds_tsv_error(t);
            if (rc > 0) { put(*out, b); put(*out, e); }
            ds_tsv_close(t);
            return rc;
        }});
    cases.push_back({"ds_tsv_set_range", READER, [=](Bytes* out, std::string* err) {
        int64_t n = 0;
        ds_tsv* t = located_reader(small, 2, &n);
        arm();
        const int rc = ds_tsv_set_range(t, 0, ds_tsv_align(t, 1));
        disarm();
        *err = ds_tsv_error(t);
        const int64_t again = ds_tsv_locate(t, 16);
        put(*out, &again, 1);
        ds_tsv_close(t);
        return (int64_t)rc;
    }});
    cases.push_back({"ds_format_rows", NONE, [](Bytes* out, std::string*) {
        const char info[] = "chr1\t1\t+\t1\tr0\ttchr2\t5\t-\t9\tr1\tc";
        const int64_t off[3] = {0, 15, 30};
        const float act[4] = {0.25f, 0.75f, 1e-9f, 3.f};
        const int32_t pred[2] = {1, 1}, kmer[6] = {0, 1, 2, 3, 4, 9};
        std::vector<char> text(256);
        arm();
        const int64_t rc = ds_format_rows(2, info, off, act, 2, pred, kmer, 3, text.data(), (int64_t)text.size());
        disarm();
        if (rc > 0) put(*out, text.data(), (size_t)rc);
        return rc;
    }});
    cases.push_back({"ds_freq_locate", NONE, [](Bytes* out, std::string*) {
        std::vector<int64_t> b(8), e(8);
        std::vector<int32_t> chrom(8);
        std::vector<uint8_t> flags(8);
        std::vector<char> names(64);
        int64_t nb = 0;
        int32_t nn = 0;
        arm();
        const int64_t rc = ds_freq_locate(CALLS, (int64_t)strlen(CALLS), 8, b.data(), e.data(), chrom.data(), flags.data(), names.data(), 64, &nb, &nn);
        disarm();
        if (rc > 0) { put(*out, b.data(), (size_t)rc); put(*out, e.data(), (size_t)rc); put(*out, chrom.data(), (size_t)rc); put(*out, flags.data(), (size_t)rc);
                      put(*out, names.data(), (size_t)nb); put(*out, &nn, 1); }
        return rc;
    }});
    cases.push_back({"ds_freq_keys", NONE, [](Bytes* out, std::string*) {
        const char info[] = "chr1\t1\t+\t1\tr0\ttchr2\t5\t-\t9\tr1\tcchr1\t1\t+\t1\tr2\tt \t1";
        const int64_t off[5] = {0, 15, 30, 45, 48};      // the last row: column 0 is a blank
        std::vector<int32_t> chrom(4);
        std::vector<int64_t> pos(4);
        std::vector<uint8_t> flags(4);
        std::vector<char> names(64);
        int64_t nb = 0;
        int32_t nn = 0;
        arm();
        const int64_t rc = ds_freq_keys(4, info, off, chrom.data(), pos.data(), flags.data(), names.data(), 64, &nb, &nn);
        disarm();
        if (rc > 0) { put(*out, chrom); put(*out, pos); put(*out, flags); put(*out, names.data(), (size_t)nb); put(*out, &nn, 1); }
        return rc;
    }});
    cases.push_back({"ds_fasta_locate", NONE, [](Bytes* out, std::string*) {
        const char fa[] = "lead\n>one first record\nACGT\r\nCG\n\n>two\nAA";
        std::vector<int64_t> lb(8), le(8), lo(8), nb(4), ne(4), rl(4);
        std::vector<int32_t> lr(8);
        int64_t nrec = 0;
        int32_t flags = 0;
        arm();
        const int64_t rc = ds_fasta_locate(fa, (int64_t)strlen(fa), 8, lb.data(), le.data(), lr.data(), lo.data(), 4, nb.data(), ne.data(), rl.data(), &nrec, &flags);
        disarm();
        if (rc > 0) { put(*out, lb); put(*out, le); put(*out, lr); put(*out, lo); put(*out, nb); put(*out, ne); put(*out, rl); put(*out, &nrec, 1); put(*out, &flags, 1); }
        return rc;
    }});
    cases.push_back({"ds_eval_locate", NONE, [](Bytes* out, std::string*) {
        std::vector<int64_t> b(8), e(8);
        std::vector<uint8_t> flags(8);
        int32_t ff = 0;
        arm();
        const int64_t rc = ds_eval_locate(CALLS, (int64_t)strlen(CALLS), 8, b.data(), e.data(), flags.data(), &ff);
        disarm();
        if (rc > 0) { put(*out, b); put(*out, e); put(*out, flags); put(*out, &ff, 1); }
        return rc;
    }});
}

#ifndef ABI_FIREWALL_IO_ONLY
static void add_engine_cases(std::vector<Case>& cases)
{
    cases.push_back({"ds_parse_text_reference (one bad span)", THREAD, [](Bytes* out, std::string* err) {
        const char text[] = "chr1\t1\t+\t1\tr0\tt\tACG\t0.1,0.2,0.3\t0.01,0.02,0.03\t3,4,5\t0.5,-0.5,0.25,1.5\t1";
        const int64_t b[2] = {0, 5}, e[2] = {(int64_t)strlen(text), 4};
        std::vector<int32_t> kmer(2 * K), labels(2), ilen(2), status(2);
        std::vector<float> means(2 * K), stds(2 * K), lens(2 * K), signals(2 * S);
        arm();
        const int rc = ds_parse_text_reference(K, S, text, 2, b, e, kmer.data(), means.data(), stds.data(), lens.data(), signals.data(), labels.data(),
                                               ilen.data(), status.data());
        disarm();
        *err = ds_last_error(nullptr);
        (void)out;
        return (int64_t)rc;
    }});
    cases.push_back({"ds_parse_text_reference", THREAD, [](Bytes* out, std::string* err) {
        const char text[] = "chr1\t1\t+\t1\tr0\tt\tACG\t0.1,0.2,0.3\t0.01,0.02,0.03\t3,4,5\t0.5,-0.5,0.25,1.5\t1\nchr1\t2\t+\t2\tr0\tt\tACG\t+1,nan,3\t1,2,3\t3,4,5\t1,2,3,4\t0";
        const int64_t len = (int64_t)strlen(text), nl = (int64_t)(strchr(text, '\n') - text);
        const int64_t b[2] = {0, nl + 1}, e[2] = {nl, len};
        std::vector<int32_t> kmer(2 * K), labels(2), ilen(2), status(2);
        std::vector<float> means(2 * K), stds(2 * K), lens(2 * K), signals(2 * S);
        arm();
        const int rc = ds_parse_text_reference(K, S, text, 2, b, e, kmer.data(), means.data(), stds.data(), lens.data(), signals.data(), labels.data(),
                                               ilen.data(), status.data());
        disarm();
        *err = ds_last_error(nullptr);
        if (rc == DS_OK) { put(*out, status); put(*out, kmer.data(), K); put(*out, means.data(), K); put(*out, signals.data(), S); put(*out, labels.data(), 1); }
        return (int64_t)rc;
    }});
    // one read of five bases, two samples each; the site is its middle base
    static const int16_t raw[10] = {100, 104, 90, 96, 120, 118, 80, 85, 101, 99};
    static const int64_t raw_off[2] = {0, 10}, start[5] = {0, 2, 4, 6, 8}, base_off[2] = {0, 5};
    static const int32_t length[5] = {2, 2, 2, 2, 2}, site_read[1] = {0}, site_loc[1] = {2};
    static const int8_t base[5] = {0, 1, 2, 3, 0};
    static const double scaling[1] = {0.5}, offset[1] = {3.0};
    static ds_reads reads;
    reads.nreads = 1; reads.raw = raw; reads.raw_off = raw_off; reads.start = start; reads.length = length; reads.base = base;
    reads.base_off = base_off; reads.scaling = scaling; reads.offset = offset; reads.key = nullptr; reads.nsites = 1;
    reads.site_read = site_read; reads.site_loc = site_loc; reads.norm = DS_NORM_MAD; reads.seed = 7;
    cases.push_back({"ds_extract_reference", THREAD, [](Bytes* out, std::string* err) {
        std::vector<int32_t> kmer(K);
        std::vector<float> means(K), stds(K), sanums(K), signals(S);
        arm();
        const int rc = ds_extract_reference(&reads, K, S, kmer.data(), means.data(), stds.data(), sanums.data(), signals.data());
        disarm();
        *err = ds_last_error(nullptr);
        if (rc == DS_OK) { put(*out, kmer); put(*out, means); put(*out, stds); put(*out, sanums); put(*out, signals); }
        return (int64_t)rc;
    }});
    cases.push_back({"ds_extract_reference (a site at the read's edge)", THREAD, [](Bytes*, std::string* err) {
        static const int32_t edge[1] = {0};
        ds_reads r = reads;
        r.site_loc = edge;
        std::vector<int32_t> kmer(K);
        std::vector<float> means(K), stds(K), sanums(K), signals(S);
        arm();
        const int rc = ds_extract_reference(&r, K, S, kmer.data(), means.data(), stds.data(), sanums.data(), signals.data());
        disarm();
        *err = ds_last_error(nullptr);
        return (int64_t)rc;
    }});
    cases.push_back({"ds_extract_rows_reference", THREAD, [](Bytes* out, std::string* err) {
        const char info[] = "chr1\t2\t+\t2\tr0\tt";
        const int64_t info_off[2] = {0, (int64_t)strlen(info)};
        std::vector<char> text(4096);
        int64_t row_off[2] = {0, 0};
        arm();
        const int64_t rc = ds_extract_rows_reference(&reads, K, S, info, info_off, 1, text.data(), (int64_t)text.size(), row_off);
        disarm();
        *err = ds_last_error(nullptr);
        if (rc > 0) { put(*out, text.data(), (size_t)rc); put(*out, row_off, 2); }
        return rc;
    }});
    cases.push_back({"ds_freq_reference", THREAD, [](Bytes* out, std::string* err) {
        std::vector<int64_t> b(4), e(4), pos(4), first(4), spos(4);
        std::vector<int32_t> chrom(4), status(4, 0), met(4), schrom(4), smet(4), sunmet(4);
        std::vector<uint8_t> flags(4);
        std::vector<double> p0(4), p1(4), s0(4), s1(4);
        std::vector<char> names(64);
        int64_t nb = 0, used = 0;
        int32_t nn = 0;
        if (ds_freq_locate(CALLS, (int64_t)strlen(CALLS), 4, b.data(), e.data(), chrom.data(), flags.data(), names.data(), 64, &nb, &nn) != 4) exit(2);
        arm();
        const int64_t rc = ds_freq_reference(CALLS, 4, b.data(), e.data(), chrom.data(), flags.data(), 0.1, status.data(), pos.data(), p0.data(), p1.data(),
                                             met.data(), 4, first.data(), schrom.data(), spos.data(), s0.data(), s1.data(), smet.data(), sunmet.data(), &used);
        disarm();
        *err = ds_last_error(nullptr);
        if (rc > 0) { put(*out, status); put(*out, first.data(), (size_t)rc); put(*out, spos.data(), (size_t)rc); put(*out, s0.data(), (size_t)rc);
                      put(*out, s1.data(), (size_t)rc); put(*out, smet.data(), (size_t)rc); put(*out, sunmet.data(), (size_t)rc); put(*out, &used, 1); }
        return rc;
    }});
    cases.push_back({"ds_freq_reference (no room for the sites)", THREAD, [](Bytes*, std::string* err) {
        std::vector<int64_t> b(4), e(4), pos(4), first(4), spos(4);
        std::vector<int32_t> chrom(4), status(4, 0), met(4), schrom(4), smet(4), sunmet(4);
        std::vector<uint8_t> flags(4);
        std::vector<double> p0(4), p1(4), s0(4), s1(4);
        std::vector<char> names(64);
        int64_t nb = 0, used = 0;
        int32_t nn = 0;
        if (ds_freq_locate(CALLS, (int64_t)strlen(CALLS), 4, b.data(), e.data(), chrom.data(), flags.data(), names.data(), 64, &nb, &nn) != 4) exit(2);
        arm();
        const int64_t rc = ds_freq_reference(CALLS, 4, b.data(), e.data(), chrom.data(), flags.data(), 0.1, status.data(), pos.data(), p0.data(), p1.data(),
                                             met.data(), 1, first.data(), schrom.data(), spos.data(), s0.data(), s1.data(), smet.data(), sunmet.data(), &used);
        disarm();
        *err = ds_last_error(nullptr);
        return rc;
    }});
    static const int64_t seg_b[1] = {0}, seg_e[1] = {8}, seg_bit[1] = {0}, rec_len[1] = {8};
    static const uint8_t seg_carry[1] = {0};
    cases.push_back({"ds_motif_reference", THREAD, [](Bytes* out, std::string* err) {
        uint32_t bitmap[1] = {0};
        arm();
        const int rc = ds_motif_reference(GENOME, 1, seg_b, seg_e, seg_bit, seg_carry, 8, bitmap);
        disarm();
        *err = ds_last_error(nullptr);
        if (rc == DS_OK) put(*out, bitmap, 1);
        return (int64_t)rc;
    }});
    cases.push_back({"ds_motif_reference (a segment past the bitmap)", THREAD, [](Bytes*, std::string* err) {
        uint32_t bitmap[1] = {0};
        arm();
        const int rc = ds_motif_reference(GENOME, 1, seg_b, seg_e, seg_bit, seg_carry, 4, bitmap);
        disarm();
        *err = ds_last_error(nullptr);
        return (int64_t)rc;
    }});
    for (int cap = 3; cap >= 0; cap -= 3)
        cases.push_back({cap ? "ds_combine_reference" : "ds_combine_reference (the rows alone)", THREAD, [=](Bytes* out, std::string* err) {
            uint32_t bitmap[1] = {0};
            if (ds_motif_reference(GENOME, 1, seg_b, seg_e, seg_bit, seg_carry, 8, bitmap) != DS_OK) exit(2);
            std::vector<int64_t> b(3), e(3), pos(3), met(3), unmet(3), cov(3), spos(3), smet(3), sunmet(3), scov(3), last(3);
            std::vector<int32_t> chrom(3, 0), status(3, 0), plus(3), schrom(3);
            std::vector<uint8_t> flags(3);
            std::vector<double> a(3), bb(3), s0(3), s1(3);
            std::vector<char> names(64);
            int64_t nb = 0;
            int32_t nn = 0;
            if (ds_freq_locate(TABLE, (int64_t)strlen(TABLE), 3, b.data(), e.data(), chrom.data(), flags.data(), names.data(), 64, &nb, &nn) != 3) exit(2);
            arm();
            const int64_t rc = ds_combine_reference(DS_COMBINE_TABLE, TABLE, 3, b.data(), e.data(), chrom.data(), flags.data(), 1, rec_len, bitmap, status.data(),
                                                    pos.data(), plus.data(), a.data(), bb.data(), met.data(), unmet.data(), cov.data(), cap, schrom.data(),
                                                    spos.data(), s0.data(), s1.data(), smet.data(), sunmet.data(), scov.data(), last.data());
            disarm();
            *err = ds_last_error(nullptr);
            if (rc > 0 && !cap) put(*out, status);
            if (rc > 0 && cap) { put(*out, status); put(*out, spos.data(), (size_t)rc); put(*out, s0.data(), (size_t)rc); put(*out, s1.data(), (size_t)rc);
                          put(*out, scov.data(), (size_t)rc); put(*out, last.data(), (size_t)rc); }
            return rc;
        }});
    for (int ncf = 1; ncf <= 33; ncf += 32)
        cases.push_back({ncf == 1 ? "ds_eval_reference" : "ds_eval_reference (33 cut-offs)", THREAD, [=](Bytes* out, std::string* err) {
            std::vector<int64_t> b(4), e(4), counts(2 * (4 + 2 * (size_t)ncf)), pn(2), nn(2);
            std::vector<uint8_t> flags(4), mask = {3, 7, 2, 7};
            std::vector<int32_t> status(4, 0), called(4);
            std::vector<double> p0(4), p1(4), cf((size_t)ncf, 0.2);
            std::vector<uint64_t> u2(2);
            int32_t ff = 0;
            if (ds_eval_locate(CALLS, (int64_t)strlen(CALLS), 4, b.data(), e.data(), flags.data(), &ff) != 4) exit(2);
            arm();
            const int rc = ds_eval_reference(CALLS, 4, b.data(), e.data(), flags.data(), mask.data(), ncf, cf.data(), status.data(), p0.data(), p1.data(),
                                             called.data(), counts.data(), u2.data(), pn.data(), nn.data());
            disarm();
            *err = ds_last_error(nullptr);
            if (rc == DS_OK) { put(*out, status); put(*out, counts); put(*out, u2); put(*out, pn); put(*out, nn); }
            return (int64_t)rc;
        }});
}
#endif

// ---- the sweep ----------------------------------------------------------------------------------------------------------------
static int sweep(const Case& c)
{
    int bad = 0;
    Bytes out0;
    std::string err0;
    g_fail_at = -1;
    const int64_t rc0 = c.call(&out0, &err0);
    const long count = g_count.load();
    printf("%-48s rc %4lld  %3ld allocations  %4zu result bytes", c.name, (long long)rc0, count, out0.size());
#ifndef ABI_FIREWALL_NO_INJECT
    if (count == 0 && !no_alloc_listed(c.name)) { printf("\n  FAIL: no allocation was counted and the entry is not on NO_ALLOC: the sweep would test nothing\n"); return 1; }
    long fired = 0;
    for (int kind = BAD_ALLOC; kind <= RUNTIME_ERROR; ++kind)
        for (long n = 0; n < count; ++n) {
            g_kind = kind;
            g_fail_at = n;
            Bytes out;
            std::string err;
            const int64_t rc = c.call(&out, &err);
            g_fail_at = -1;
            if (!g_fired.load()) {      // fewer allocations than the first call (an error text that has room by now, helper threads in another order): nothing happened
                if (rc != rc0 || out != out0) { printf("\n  FAIL: allocation %ld was not reached and the call gave rc %lld, other bytes or both", n, (long long)rc); ++bad; }
                continue;
            }
            ++fired;
            const int want = kind == BAD_ALLOC ? DS_ERR_NOMEM : DS_ERR_INVALID;
            const char* text = kind == BAD_ALLOC ? "out of host memory" : "internal error: injected";
            if (rc != want) { printf("\n  FAIL: %s at allocation %ld: rc %lld, expected %d", kind == BAD_ALLOC ? "bad_alloc" : "runtime_error", n, (long long)rc, want); ++bad; }
            else if (c.sink != NONE && err != text) { printf("\n  FAIL: %s at allocation %ld: error text '%s', expected '%s'", kind == BAD_ALLOC ? "bad_alloc" : "runtime_error", n, err.c_str(), text); ++bad; }
        }
    printf("  %3ld injected", fired);
    if (count > 0 && fired == 0) { printf("\n  FAIL: no injection fired"); ++bad; }
#endif
    Bytes out1;
    std::string err1;
    const int64_t rc1 = c.call(&out1, &err1);
    if (rc1 != rc0 || out1 != out0 || (rc0 < 0 && err1 != err0)) { printf("\n  FAIL: the call after the sweep differs from the first (rc %lld, '%s')", (long long)rc1, err1.c_str()); ++bad; }
    printf("\n");
    return bad;
}

int main(int argc, char** argv)
{
    if (argc < 2) { printf("usage: abi_firewall <scratch directory>\n"); return 2; }
    setvbuf(stdout, nullptr, _IOLBF, 0);
    std::vector<Case> cases;
    add_io_cases(cases, argv[1]);
#ifndef ABI_FIREWALL_IO_ONLY
    add_engine_cases(cases);
#endif
    int bad = 0;
    for (const Case& c : cases) bad += sweep(c);
    if (bad) { printf("abi_firewall: %d FAILED\n", bad); return 1; }
    printf("abi_firewall: ok (%zu cases)\n", cases.size());
    return 0;
}
