// freq_hostile.cpp — the host half of call_freq --on gpu (ds_freq_locate, and dsf::reference behind ds_freq_reference) and of
// call_mods --freq_file (ds_freq_keys, and dsf::call_value through dsf::values_reference) over hostile
// buffers, as a stand-alone program for a host sanitizer build. Every buffer is copied into a heap block of exactly its size, so a
// read past either end is a report. Build and run (host code only; nothing here touches a GPU):
//   hipcc --offload-arch=gfx950 -std=c++17 -O1 -g -Xarch_host -fsanitize=address,undefined \
//         -x hip tools/freq_hostile.cpp deepsignal_amd/csrc/ds_freq.hip deepsignal_amd/csrc/ds_site_table.hip deepsignal_amd/csrc/ds_io.cpp \
//         -o freq_hostile && ./freq_hostile
#include "../include/deepsignal_hip.h"
#include "../deepsignal_amd/csrc/ds_freq.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

static int run(const std::string& data, const char* what)
{
    char* buf = static_cast<char*>(malloc(data.size() ? data.size() : 1));
    memcpy(buf, data.data(), data.size());
    const char* text = data.size() ? buf : nullptr;
    int64_t nb = 0;
    int32_t nn = 0;
    const int64_t n = ds_freq_locate(text, (int64_t)data.size(), 0, nullptr, nullptr, nullptr, nullptr, nullptr, 0, &nb, &nn);
    if (n < 0) { printf("%s: locate failed\n", what); return 1; }
    std::vector<int64_t> b((size_t)n + 1), e((size_t)n + 1), pos((size_t)n + 1), first((size_t)n + 1), spos((size_t)n + 1);
    std::vector<int32_t> chrom((size_t)n + 1), status((size_t)n + 1, 0), met((size_t)n + 1), schrom((size_t)n + 1), smet((size_t)n + 1), sunmet((size_t)n + 1);
    std::vector<uint8_t> flags((size_t)n + 1);
    std::vector<double> p0((size_t)n + 1), p1((size_t)n + 1), s0((size_t)n + 1), s1((size_t)n + 1);
    char* names = static_cast<char*>(malloc(nb ? (size_t)nb : 1));
    const int64_t n2 = ds_freq_locate(text, (int64_t)data.size(), n, b.data(), e.data(), chrom.data(), flags.data(), names, nb, &nb, &nn);
    int64_t used = 0;
    std::string err;
    const int64_t sites = dsf::reference(text ? text : "", n, b.data(), e.data(), chrom.data(), flags.data(), 0.1, status.data(), pos.data(), p0.data(),
                                         p1.data(), met.data(), n, first.data(), schrom.data(), spos.data(), s0.data(), s1.data(), smet.data(),
                                         sunmet.data(), &used, &err);
    int64_t host = 0;
    for (int64_t i = 0; i < n; ++i) host += status[(size_t)i] != 0;
    printf("%-28s %6lld bytes %4lld rows %3d names %4lld host rows %4lld sites %4lld used\n", what, (long long)data.size(), (long long)n, nn,
           (long long)host, (long long)sites, (long long)used);
    free(names);
    free(buf);
    return n2 == n && sites >= 0 ? 0 : 1;
}

// ds_freq_keys (call_mods --freq_file): the pieces of `data` between '\n' as sampleinfo strings, packed without separators into a heap
// block of exactly their size; then every piece once more as the only string of a block of its own
static int run_keys(const std::string& data, const char* what)
{
    std::vector<std::string> pieces;
    size_t at = 0;
    while (at <= data.size()) {
        const size_t nl = data.find('\n', at);
        pieces.push_back(data.substr(at, nl == std::string::npos ? std::string::npos : nl - at));
        if (nl == std::string::npos) break;
        at = nl + 1;
    }
    int bad = 0;
    long long flagged = 0;
    for (size_t round = 0; round <= pieces.size(); ++round) {      // round 0: all pieces in one call
        std::string packed;
        std::vector<int64_t> off = {0};
        for (size_t i = 0; i < pieces.size(); ++i) {
            if (round && i + 1 != round) continue;
            packed += pieces[i];
            off.push_back((int64_t)packed.size());
        }
        const int64_t n = (int64_t)off.size() - 1;
        char* buf = static_cast<char*>(malloc(packed.size() ? packed.size() : 1));
        memcpy(buf, packed.data(), packed.size());
        std::vector<int32_t> chrom((size_t)n + 1);
        std::vector<int64_t> pos((size_t)n + 1);
        std::vector<uint8_t> flags((size_t)n + 1);
        int64_t nb = 0;
        int32_t nn = 0;
        if (ds_freq_keys(n, buf, off.data(), chrom.data(), pos.data(), flags.data(), nullptr, 0, &nb, &nn) != n) bad = 1;
        char* names = static_cast<char*>(malloc(nb ? (size_t)nb : 1));
        if (ds_freq_keys(n, buf, off.data(), chrom.data(), pos.data(), flags.data(), names, nb, &nb, &nn) != n) bad = 1;
        for (int64_t i = 0; i < n; ++i) {
            if (flags[(size_t)i] ? chrom[(size_t)i] != -1 : !dss::key_ok(chrom[(size_t)i], pos[(size_t)i]) || chrom[(size_t)i] >= nn) bad = 1;
            if (!round) flagged += flags[(size_t)i];
        }
        free(names);
        free(buf);
    }
    printf("%-28s keys: %4zu strings %4lld flagged%s\n", what, pieces.size(), flagged, bad ? "  BAD" : "");
    return bad;
}

// dss::row_spans, the span check of ds_freq_parse / ds_combine_parse: heap blocks of exactly n entries; the first bad row, or none
static int run_spans()
{
    struct Case { std::vector<int64_t> b, e; int bad; };
    const int64_t big = (int64_t)1 << 31;
    const Case cases[] = {{{0}, {0}, -1}, {{5, 9, 9}, {9, 9, 20}, -1}, {{0, 4}, {5, 8}, 1}, {{3, 2}, {3, 2}, 1}, {{7}, {6}, 0}, {{0, 10}, {10, 10 + big}, 1},
                          {{0, 10}, {10, 9 + big}, -1}, {{INT64_MAX - 1, INT64_MAX}, {INT64_MAX, INT64_MAX}, -1}, {{0, 1, 2, 3}, {1, 2, 3, 2}, 3}};
    int wrong = 0;
    for (const Case& c : cases) {
        const int32_t n = (int32_t)c.b.size();
        int64_t* b = static_cast<int64_t*>(malloc((size_t)n * 8));
        int64_t* e = static_cast<int64_t*>(malloc((size_t)n * 8));
        memcpy(b, c.b.data(), (size_t)n * 8);
        memcpy(e, c.e.data(), (size_t)n * 8);
        std::vector<int64_t> off;
        std::vector<int32_t> len;
        int bad = -1;
        const bool ok = dss::row_spans(n, b, e, &off, &len, &bad);
        if (ok != (c.bad < 0) || (!ok && bad != c.bad)) wrong = 1;
        for (int32_t i = 0; ok && i < n; ++i)
            if (off[(size_t)i] != c.b[(size_t)i] - c.b[0] || len[(size_t)i] != c.e[(size_t)i] - c.b[(size_t)i]) wrong = 1;
        free(b);
        free(e);
    }
    printf("%-28s %4zu cases%s\n", "row spans", sizeof(cases) / sizeof(cases[0]), wrong ? "  BAD" : "");
    return wrong;
}

// dsf::call_value over the float32 patterns where its exponent arithmetic and table indices sit at their ends
static int run_values()
{
    const uint32_t patterns[] = {0x00000000u, 0x80000000u, 0x00000001u, 0x007fffffu, 0x00800000u, 0x0d800000u, 0x0dffffffu, 0x19000000u, 0x19800000u,
                                 0x1a000000u, 0x283424dcu, 0x28342000u, 0x33800000u, 0x3effffffu, 0x3f000000u, 0x3f7fffffu, 0x3f800000u, 0x3f800001u,
                                 0x40000000u, 0x7f7fffffu, 0x7f800000u, 0x7fc00000u, 0xff800000u, 0xbf800000u, 0xbf000000u};
    std::vector<float> act;
    for (uint32_t a : patterns)
        for (uint32_t b : patterns) {
            float x, y;
            memcpy(&x, &a, 4);
            memcpy(&y, &b, 4);
            act.push_back(x);
            act.push_back(y);
        }
    const int64_t n = (int64_t)act.size() / 2;
    std::vector<double> p0((size_t)n), p1((size_t)n);
    std::vector<int32_t> status((size_t)n);
    int bad = 0;
    dsf::values_reference(n, act.data(), 2, p0.data(), p1.data(), status.data());
    long long host = 0;
    for (int64_t i = 0; i < n; ++i) {
        host += status[(size_t)i] != 0;
        if (!status[(size_t)i] && !(p0[(size_t)i] >= -1.0 && p0[(size_t)i] <= 1.0 && p1[(size_t)i] >= -1.0 && p1[(size_t)i] <= 1.0)) bad = 1;
    }
    printf("%-28s %4lld act rows %4lld host rows%s\n", "value patterns", (long long)n, host, bad ? "  BAD" : "");
    return bad;
}

int main()
{
    const std::string good = "chr1\t10\t+\t990\tread0\tt\t0.25\t0.75\t1\tACGTACGTCGACGTACG";
    auto row = [](const std::string& pos, const std::string& p0, const std::string& p1, const std::string& label) {
        return "chr2\t" + pos + "\t-\t7\tread1\tt\t" + p0 + "\t" + p1 + "\t" + label + "\tACGTACGTCGACGTACG";
    };
    std::vector<std::string> rows = {good, good, row("5", "nan", "0.5", "1"), row("5", "inf", "0.5", "1"), row("5", "1e-30", "0.5", "0"),
                                     row("5", "+0.5", "0.5", "1"), " " + good, good + "\r", "a\rb", "", "\t", "\t\t\t\t\t\t\t\t\t", good + "\t", row("1099511627776", "0.1", "0.9", "1"),
                                     row("-1", "0.1", "0.9", "1"), row("1099511627775", "0.1", "0.9", "1"), row("999999999999999999999", "0.1", "0.9", "1"),
                                     row("5", "1234567890123456", "0.9", "1"), row("5", "1e22", "1e-22", "1"), row("5", "1e23", "1e-23", "1"),
                                     row("5", "1e", ".", "-"), row("5", "0.1", "0.9", "1234567890"), row("5", "0.1", "0.9", ""), "chr\xc3\xa9\t1\t+\t2", good.substr(0, 40),
                                     row("5", "1e99999999999999999999", "0.9", "1"), row("5", "-", "-", "-"), std::string(5000, '7'), std::string(300, '\t'), good};
    std::string all;
    for (const std::string& r : rows) all += r + "\n";
    int bad = 0;
    bad += run(all, "hostile rows");
    bad += run(all.substr(0, all.size() - 1), "no trailing newline");
    bad += run("", "empty");
    bad += run("\n", "one blank row");
    bad += run(good, "one row, no newline");
    for (size_t cut = 0; cut <= good.size() + 1; ++cut) bad += run((good + "\n" + good).substr(0, good.size() + 1 + cut), "truncated");
    for (size_t cut = 1; cut < all.size(); cut += 37) bad += run(all.substr(0, cut), "truncated hostile");
    bad += run_keys(all, "hostile rows");
    bad += run_keys("", "empty");
    bad += run_keys(good, "one row");
    for (size_t cut = 1; cut < all.size(); cut += 37) bad += run_keys(all.substr(0, cut), "truncated hostile");
    bad += run_values();
    bad += run_spans();
    printf(bad ? "FAILED\n" : "all buffers done\n");
    return bad ? 1 : 0;
}
