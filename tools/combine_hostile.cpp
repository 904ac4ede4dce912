// combine_hostile.cpp — the host half of combine_strands --on gpu (ds_fasta_locate, and dsc::motif_reference / dsc::reference behind
// ds_motif_reference / ds_combine_reference) over hostile buffers, as a stand-alone program for a host sanitizer build. Every
// buffer is copied into a heap block of exactly its size, so a read past either end is a report. Build and run (host code only;
// nothing here touches a GPU):
//   hipcc --offload-arch=gfx950 -std=c++17 -O1 -g -ffp-contract=off -Xarch_host -fsanitize=address,undefined -x hip tools/combine_hostile.cpp \
//         deepsignal_amd/csrc/ds_combine.hip deepsignal_amd/csrc/ds_site_table.hip deepsignal_amd/csrc/ds_io.cpp -o combine_hostile && ./combine_hostile
#include "../include/deepsignal_hip.h"
#include "../deepsignal_amd/csrc/ds_combine.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

// a FASTA buffer: locate, keep every record (numbered as located), scan in chunks of `chunk` bytes; then `table` against it
static int run(const std::string& fasta, const std::string& table, int form, int64_t chunk, const char* what)
{
    char* buf = static_cast<char*>(malloc(fasta.size() ? fasta.size() : 1));
    memcpy(buf, fasta.data(), fasta.size());
    const char* text = fasta.size() ? buf : nullptr;
    int64_t nrec = 0;
    int32_t fl = 0;
    const int64_t nl = ds_fasta_locate(text, (int64_t)fasta.size(), 0, nullptr, nullptr, nullptr, nullptr, 0, nullptr, nullptr, nullptr, &nrec, &fl);
    if (nl < 0 || nrec < 1) { printf("%s: locate failed\n", what); free(buf); return 1; }
    std::vector<int64_t> lb((size_t)nl + 1), le((size_t)nl + 1), lo((size_t)nl + 1), nb((size_t)nrec), ne((size_t)nrec), len((size_t)nrec);
    std::vector<int32_t> lr((size_t)nl + 1);
    const int64_t nl2 = ds_fasta_locate(text, (int64_t)fasta.size(), nl, lb.data(), le.data(), lr.data(), lo.data(), nrec, nb.data(), ne.data(), len.data(), &nrec, &fl);
    int bad = nl2 != nl;
    std::vector<int64_t> base((size_t)nrec);
    int64_t nbits = 0;
    for (int64_t r = 0; r < nrec; ++r) {
        if (nb[(size_t)r] < 0 || ne[(size_t)r] < nb[(size_t)r] || ne[(size_t)r] > (int64_t)fasta.size()) bad = 1;
        base[(size_t)r] = nbits;
        nbits += len[(size_t)r];
    }
    // the segments: every line cut into pieces of at most `chunk` bytes, the base in front carried in
    std::vector<int64_t> sb, se, sbit;
    std::vector<uint8_t> carry;
    for (int64_t i = 0; i < nl; ++i) {
        if (lb[(size_t)i] < 0 || le[(size_t)i] <= lb[(size_t)i] || le[(size_t)i] > (int64_t)fasta.size() || lr[(size_t)i] < 0 || lr[(size_t)i] >= nrec) { bad = 1; continue; }
        for (int64_t b = lb[(size_t)i]; b < le[(size_t)i]; b += chunk) {
            sb.push_back(b);
            se.push_back(b + chunk < le[(size_t)i] ? b + chunk : le[(size_t)i]);
            sbit.push_back(base[(size_t)lr[(size_t)i]] + lo[(size_t)i] + (b - lb[(size_t)i]));
            const bool first = b == lb[(size_t)i] && lo[(size_t)i] == 0;
            carry.push_back(first ? 0 : (uint8_t)(b > lb[(size_t)i] ? text[b - 1] : text[le[(size_t)i - 1] - 1]));
        }
    }
    std::vector<uint32_t> bitmap((size_t)((nbits + 31) >> 5) + 1, 0u);
    std::string err;
    if (!bad && !dsc::motif_reference(text ? text : "", (int64_t)sb.size(), sb.data(), se.data(), sbit.data(), carry.data(), nbits, bitmap.data(), &err)) {
        printf("%s: scan failed: %s\n", what, err.c_str());
        bad = 1;
    }
    int64_t hits = 0;
    for (uint32_t w : bitmap) hits += __builtin_popcount(w);
    // the rows
    char* tbuf = static_cast<char*>(malloc(table.size() ? table.size() : 1));
    memcpy(tbuf, table.data(), table.size());
    const char* ttext = table.size() ? tbuf : nullptr;
    int64_t nbn = 0;
    int32_t nn = 0;
    const int64_t n = ds_freq_locate(ttext, (int64_t)table.size(), 0, nullptr, nullptr, nullptr, nullptr, nullptr, 0, &nbn, &nn);
    std::vector<int64_t> b((size_t)n + 1), e((size_t)n + 1), pos((size_t)n + 1), c0((size_t)n + 1), c1((size_t)n + 1), c2((size_t)n + 1), spos((size_t)n + 1),
        smet((size_t)n + 1), sunmet((size_t)n + 1), scov((size_t)n + 1), slast((size_t)n + 1);
    std::vector<int32_t> chrom((size_t)n + 1), status((size_t)n + 1, 0), plus((size_t)n + 1), schrom((size_t)n + 1);
    std::vector<uint8_t> flags((size_t)n + 1);
    std::vector<double> a((size_t)n + 1), bb((size_t)n + 1), s0((size_t)n + 1), s1((size_t)n + 1);
    char* names = static_cast<char*>(malloc(nbn ? (size_t)nbn : 1));
    if (ds_freq_locate(ttext, (int64_t)table.size(), n, b.data(), e.data(), chrom.data(), flags.data(), names, nbn, &nbn, &nn) != n) bad = 1;
    for (int64_t i = 0; i < n; ++i)
        if (chrom[(size_t)i] >= 0) chrom[(size_t)i] = chrom[(size_t)i] % (int32_t)(nrec < 1000 ? nrec : 1000) - (i % 7 == 0);      // now and then -1: no record
    int64_t sites = 0;
    if (!bad && nrec <= dss::CHROM_LIMIT)
        sites = dsc::reference(form, ttext ? ttext : "", n, b.data(), e.data(), chrom.data(), flags.data(), (int32_t)nrec, len.data(), bitmap.data(), status.data(),
                               pos.data(), plus.data(), a.data(), bb.data(), c0.data(), c1.data(), c2.data(), n, schrom.data(), spos.data(), s0.data(),
                               s1.data(), smet.data(), sunmet.data(), scov.data(), slast.data(), &err);
    int64_t host = 0, skip = 0;
    for (int64_t i = 0; i < n; ++i) { host += status[(size_t)i] == dsc::ROW_HOST; skip += status[(size_t)i] == dsc::ROW_SKIP; }
    printf("%-26s %7lld bytes %5lld lines %4lld records flags %d %5lld CG | %4lld rows %4lld host %4lld skipped %4lld sites%s\n", what, (long long)fasta.size(),
           (long long)nl, (long long)nrec, fl, (long long)hits, (long long)n, (long long)host, (long long)skip, (long long)sites, bad || sites < 0 ? "  BAD" : "");
    free(names);
    free(tbuf);
    free(buf);
    return bad || sites < 0 ? 1 : 0;
}

int main()
{
    const std::string kmer = "ACGTACGTCGACGTACG";
    auto trow = [&](const std::string& name, const std::string& pos, const std::string& strand, const std::string& p0, const std::string& cov) {
        return name + "\t" + pos + "\t" + strand + "\t7\t" + p0 + "\t0.5\t1\t2\t" + cov + "\t0.3333\t" + kmer;
    };
    auto brow = [&](const std::string& name, const std::string& pos, const std::string& strand, const std::string& cov, const std::string& pct) {
        return name + "\t" + pos + "\t0\t.\t" + cov + "\t" + strand + "\t" + pos + "\t0\t0,0,0\t" + cov + "\t" + pct;
    };
    const std::string fasta = "acg\n>chr1 desc\r\nACGc\r\ng\n\n>e\n>chr2\nCGC\n>chr1\nccg\nC\n> \n\t>x\n>\x01\x00y\nCG\0CG\n";
    const std::string fa(fasta.data(), fasta.size());
    std::vector<std::string> rows = {trow("chr1", "1", "+", "0.5", "3"), trow("chr1", "2", "-", "0.25", "3"), trow("chr2", "0", "+", "nan", "3"),
                                     trow("chr2", "-1", "-", "1e-30", "1234567890"), trow("chr1", "1099511627776", "+", "0.5", "3"),
                                     trow("chr1", "999999999999999999999", "-", "0.5", "3"), trow("", "", "", "", ""), "", "\t", "\t\t\t\t\t\t\t\t\t\t\t\t", "chr1\t1",
                                     " " + trow("chr1", "1", "+", "0.5", "3"), trow("chr1", "1", "+", "0.5", "3") + "\r", trow("chr1", "1", "+", "0.5", "3").substr(0, 30),
                                     brow("chr1", "1", "+", "7", "33"), brow("chr1", "2", "-", "9007199254740993", "1e22"), brow("chr2", "0", "+", "-", "."),
                                     std::string(5000, '7'), std::string(300, '\t'), "chr\xc3\xa9\t1\t+\t2", trow("chr1", "1", "+", "0.5", "3")};
    std::string table;
    for (const std::string& r : rows) table += r + "\n";
    int bad = 0;
    for (int form = 0; form < 2; ++form) {
        bad += run(fa, table, form, 64, "hostile genome and rows");
        bad += run(fa, table.substr(0, table.size() - 1), form, 1, "chunks of one byte");
        bad += run("", table, form, 64, "empty genome");
        bad += run(fa, "", form, 64, "empty table");
        bad += run(">only a header", table, form, 64, "header only");
        bad += run(">a\n>b\n>c", table, form, 64, "headers only");
        bad += run(std::string("\0\0\0>\0\n\0CG\0\n", 11), table, form, 3, "NUL-ridden");
        bad += run(">big\n" + std::string(300000, 'C') + "G" + std::string(300000, 'g') + "\nCG", table, form, 4096, "huge line");
        bad += run(std::string(100000, '\n') + "CG", table, form, 64, "blank lines");
        bad += run(std::string(70000, '>'), table, form, 64, "one huge header");
        for (size_t cut = 0; cut <= fa.size(); ++cut) bad += run(fa.substr(0, cut), table.substr(0, 40 + 13 * cut), form, 5, "truncated");
    }
    printf(bad ? "FAILED\n" : "all buffers done\n");
    return bad ? 1 : 0;
}
