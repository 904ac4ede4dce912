// evaluate_hostile.cpp — the host half of evaluate --on gpu (ds_eval_locate, and dse::reference behind ds_eval_reference) over
// hostile, truncated and empty buffers, as a stand-alone program for a host sanitizer build. Every buffer is copied into a heap block
// of exactly its size, so a read past either end is a report. Build and run (host code only; nothing here touches a GPU):
//   hipcc --offload-arch=gfx950 -std=c++17 -O1 -g -Xarch_host -fsanitize=address,undefined \
//         -x hip tools/evaluate_hostile.cpp deepsignal_amd/csrc/ds_eval.hip deepsignal_amd/csrc/ds_site_table.hip deepsignal_amd/csrc/ds_io.cpp \
//         -o evaluate_hostile && ./evaluate_hostile
#include "../include/deepsignal_hip.h"
#include "../deepsignal_amd/csrc/ds_eval.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

static int run(const std::string& data, const char* what, bool print = true)
{
    char* buf = static_cast<char*>(malloc(data.size() ? data.size() : 1));
    memcpy(buf, data.data(), data.size());
    const char* text = data.size() ? buf : nullptr;
    int32_t ff = 0;
    const int64_t n = ds_eval_locate(text, (int64_t)data.size(), 0, nullptr, nullptr, nullptr, &ff);
    if (n < 0) { printf("%s: locate failed\n", what); free(buf); return 1; }
    const size_t N = (size_t)n;
    // heap blocks of exactly n entries
    int64_t* b = static_cast<int64_t*>(malloc(N ? N * 8 : 1));
    int64_t* e = static_cast<int64_t*>(malloc(N ? N * 8 : 1));
    uint8_t* flags = static_cast<uint8_t*>(malloc(N ? N : 1));
    uint8_t* mask = static_cast<uint8_t*>(malloc(N ? N : 1));
    int32_t* status = static_cast<int32_t*>(calloc(N ? N : 1, 4));
    int32_t* called = static_cast<int32_t*>(calloc(N ? N : 1, 4));
    double* p0 = static_cast<double*>(calloc(N ? N : 1, 8));
    double* p1 = static_cast<double*>(calloc(N ? N : 1, 8));
    const int64_t n2 = ds_eval_locate(text, (int64_t)data.size(), n, b, e, flags, &ff);
    int bad = n2 != n;
    for (size_t i = 0; i < N && !bad; ++i) {
        mask[i] = (uint8_t)(2 | (i % 4 ? 1 : 0) | (i % 3 ? 4 : 0));
        if (b[i] < 0 || e[i] < b[i] || e[i] > (int64_t)data.size() || (i > 0 && b[i] != e[i - 1] + 1)) bad = 1;
    }
    const double cf[dse::MAX_CF] = {0.0, 0.025, 0.05, 0.5, 1.0, 2.0};
    int64_t host = 0;
    for (int ncf : {1, 6, dse::MAX_CF}) {
        std::vector<int64_t> counts((size_t)dse::NSETS * (4 + 2 * (size_t)ncf));
        uint64_t u2[dse::NSETS];
        int64_t pn[dse::NSETS], nn[dse::NSETS];
        for (size_t i = 0; i < N; ++i) status[i] = 0;
        if (N > 2) { status[1] = dse::ROW_GIVEN; p0[1] = 0.5; p1[1] = -0.0; called[1] = 7; }      // a row the caller gave
        std::string err;
        if (!dse::reference(text ? text : "", n, b, e, flags, mask, ncf, cf, status, p0, p1, called, counts.data(), u2, pn, nn, &err)) bad = 1;
        host = 0;
        int64_t ok = 0;
        for (size_t i = 0; i < N; ++i) {
            host += status[i] != 0;
            ok += status[i] == 0;
            if (status[i] != 0 && status[i] != 1) bad = 1;
        }
        if (counts[(size_t)(4 + 2 * ncf)] + counts[(size_t)(4 + 2 * ncf) + 1] + counts[(size_t)(4 + 2 * ncf) + 2] + counts[(size_t)(4 + 2 * ncf) + 3] != ok) bad = 1;
        if (pn[1] + nn[1] > ok || u2[1] > 2 * (uint64_t)pn[1] * (uint64_t)nn[1]) bad = 1;
    }
    // the checker refuses what it cannot take
    std::string err;
    uint64_t u2[dse::NSETS];
    int64_t pn[dse::NSETS], nn[dse::NSETS], counts[dse::NSETS * (4 + 2 * dse::MAX_CF)];
    if (dse::reference(text ? text : "", n, b, e, flags, mask, 0, cf, status, p0, p1, called, counts, u2, pn, nn, &err)) bad = 1;
    if (dse::reference(text ? text : "", n, b, e, flags, mask, dse::MAX_CF + 1, cf, status, p0, p1, called, counts, u2, pn, nn, &err)) bad = 1;
    if (N > 0) {
        mask[0] = 8;
        if (dse::reference(text, n, b, e, flags, mask, 1, cf, status, p0, p1, called, counts, u2, pn, nn, &err)) bad = 1;
    }
    if (print)
        printf("%-28s %6lld bytes %4lld rows %4lld host rows  file flags %d%s\n", what, (long long)data.size(), (long long)n, (long long)host, ff,
               bad ? "  BAD" : "");
    free(p1); free(p0); free(called); free(status); free(mask); free(flags); free(e); free(b); free(buf);
    return bad;
}

int main()
{
    const std::string good = "chr1\t10\t+\t990\tread0\tt\t0.25\t0.75\t1\tACGTACGTCGACGTACG";
    auto row = [](const std::string& pos, const std::string& p0, const std::string& p1, const std::string& label) {
        return "chr2 \t" + pos + "  -\t7\tread1\tt\t" + p0 + " " + p1 + "\t" + label + "\tACGTACGTCGACGTACG";
    };
    std::vector<std::string> rows = {good, good, row("5", "nan", "0.5", "1"), row("5", "0.5", "inf", "1"), row("5", "1e-30", "0.5", "0"),
                                     row("5", "+0.5", "0.5", "1"), " " + good, "\t \t" + good + " \t ", good + "\r", "a\rb", "", "\t", " ", "\t\t\t\t\t\t\t\t\t",
                                     "a b c d e f g h i j", "a b c d e f g h i", "a 1 c 2 e f 0.5 0.5 1", "a 1 c 2 e f 0.5 0.5 1 j", good + "\x0b", "\x1c" + good,
                                     row("-1", "0.1", "0.9", "2"), row("999999999999999999", "0.1", "0.9", "-1"), row("9999999999999999999", "0.1", "0.9", "1"),
                                     row("5", "1234567890123456", "0.9", "1"), row("5", "1e22", "1e-22", "1"), row("5", "1e23", "1e-23", "1"), row("5", "-0.0", "-0", "00"),
                                     row("5", "1e", ".", "-"), row("5", "0.1", "0.9", "1234567890"), row("5", "0.1", "0.9", "1_0"), "chr\xc3\xa9\t1\t+\t2", good.substr(0, 40),
                                     row("5", "1e99999999999999999999", "0.9", "1"), row("5", "-", "-", "-"), std::string(5000, '7'), std::string(300, '\t'),
                                     std::string(300, ' ') + "x", good};
    std::string all;
    for (const std::string& r : rows) all += r + "\n";
    int bad = 0;
    bad += run(all, "hostile rows");
    bad += run(all.substr(0, all.size() - 1), "no trailing newline");
    bad += run("", "empty");
    bad += run("\n", "one blank row");
    bad += run("\r", "one carriage return");
    bad += run("\r\n\r\n", "blank CRLF rows");
    bad += run("a\r\rb", "bare carriage returns");
    bad += run(good, "one row, no newline");
    for (size_t cut = 0; cut <= good.size() + 1; ++cut) bad += run((good + "\n" + good).substr(0, good.size() + 1 + cut), "truncated", cut % 16 == 0);
    for (size_t cut = 1; cut < all.size(); cut += 37) bad += run(all.substr(0, cut), "truncated hostile", cut % 370 == 1);
    printf(bad ? "FAILED\n" : "all buffers done\n");
    return bad ? 1 : 0;
}
