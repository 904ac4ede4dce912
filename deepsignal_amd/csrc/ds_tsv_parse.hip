// ds_tsv_parse.hip — feature-TSV rows parsed on the GPU (call_mods --parse_on gpu): the text of a batch of rows becomes the
// forward's inputs, written straight into a pipeline slot. One wave per row. Pass 1 walks the row 1 KiB at a time, every lane
// with 16 bytes: tabs and commas by compare, their column and token index by a prefix count over the wave, and every numeric
// token's start goes to a table in LDS (the text itself too, when the row fits). Pass 2: lane l parses tokens l, l + 64, ... with
// the routines of ds_tsv_device.h, the code the host checker runs. A row in any form outside that grammar is left to the host
// parser (status ROW_HOST); nothing here fails. Built with -ffp-contract=off and no fast-math (csrc/Makefile).
#include "ds_tsv_device.h"

#include <string.h>

namespace dst {

namespace {

constexpr int N_SCALARS = 8;        // LDS scalars behind the token table: [0] the tab that closes column 5, [1] the one that closes column 6
constexpr int LDS_TEXT = 8192;      // bytes of a row kept in LDS for pass 2 (longer rows are read from global memory again)
constexpr size_t LDS_MAX = 60 * 1024;

// exclusive prefix sum of v over the 64 lanes of the wave (= the workgroup); *total = the wave's sum
__device__ inline int wave_excl_scan(int v, int lane, int* total)
{
    int x = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int y = __shfl_up(x, d, 64);
        if (lane >= d) x += y;
    }
    *total = __shfl(x, 63, 64);
    return x - v;
}

__global__ __launch_bounds__(64) void tsv_parse_kernel(ParseArgs a, int lds_text)
{
    extern __shared__ uint4 lds4[];
    const int row = blockIdx.x, lane = threadIdx.x;
    if (row >= a.n) return;
    const int K = a.K, S = a.S, NT = ntokens(K, S);
    const int len = a.len[row];
    if (len < 0) {                      // not staged (uniform over the wave)
        if (lane == 0) a.status[row] = ROW_HOST;
        return;
    }
    // LDS: [text (lds_text bytes) | token starts tok[0 .. NT] | scalars]: tok[t] = first byte of numeric token t, tok[t + 1] - 1 =
    // the separator that closes it (the separators between the tab closing column 6 and the one closing column 11 are consecutive)
    char* ltext = reinterpret_cast<char*>(lds4);
    uint32_t* tok = reinterpret_cast<uint32_t*>(ltext + lds_text);
    uint32_t* sc = tok + NT + 1;
    for (int i = lane; i <= NT; i += 64) tok[i] = 0;
    if (lane < N_SCALARS) sc[lane] = 0;
    __syncthreads();
    const char* g = a.text + a.off[row];          // 16-byte aligned (the rows are staged at aligned offsets)
    bool bad = false;
    int tabs = 0, zone = 0;                       // tabs / zone separators in front of this step
    // the row end counts as a tab at position len (it closes the last column), so the walk covers len + 1 positions; the bytes
    // behind the row that a step loads lie in the next rows or in the block's one-step pad and are masked out
    const int nsteps = (len + 1 + STEP - 1) / STEP;
    for (int s = 0; s < nsteps; ++s) {
        const int pos0 = s * STEP + lane * LANE_BYTES;
        const uint4 v = *reinterpret_cast<const uint4*>(g + pos0);
        if (pos0 + LANE_BYTES <= lds_text) *reinterpret_cast<uint4*>(ltext + pos0) = v;
        const uint32_t w[4] = {v.x, v.y, v.z, v.w};
        unsigned tabm = 0, comm = 0;
#pragma unroll
        for (int b = 0; b < LANE_BYTES; ++b) {
            const unsigned c = (w[b >> 2] >> (8 * (b & 3))) & 255u;
            const int p = pos0 + b;
            if (p < len) {
                tabm |= (unsigned)(c == '\t') << b;
                comm |= (unsigned)(c == ',') << b;
            } else if (p == len) {
                tabm |= 1u << b;
            }
        }
        int step_tabs;
        const int tb0 = tabs + wave_excl_scan(__popc(tabm), lane, &step_tabs);
        // zone separators: the tabs that close columns 6 .. 11 and the commas of columns 7 .. 10; the token behind the j-th one
        // (j from 0) is numeric token j
        unsigned zm = 0;
        {
            int tb = tb0;
            unsigned m = tabm | comm;
            while (m) {
                const int b = __ffs(m) - 1;
                m &= m - 1;
                const bool is_tab = (tabm >> b) & 1u;
                if (is_tab ? (tb >= 6 && tb <= 11) : (tb >= 7 && tb <= 10)) zm |= 1u << b;
                tb += is_tab;
            }
        }
        int step_zone;
        int j = zone + wave_excl_scan(__popc(zm), lane, &step_zone);
        {
            int tb = tb0;
            unsigned m = tabm | zm;
            while (m) {
                const int b = __ffs(m) - 1;
                m &= m - 1;
                const uint32_t p = (uint32_t)(pos0 + b);
                const bool is_tab = (tabm >> b) & 1u;
                if (is_tab) {
                    if (tb == 5) sc[0] = p;
                    if (tb == 6) sc[1] = p;
                    // the tab that closes column c has exactly the tokens of columns 7 .. c in front of it
                    if ((tb == 7 && j != K) || (tb == 8 && j != 2 * K) || (tb == 9 && j != 3 * K) || (tb == 10 && j != 3 * K + S) ||
                        (tb == 11 && j != NT))
                        bad = true;
                }
                if ((zm >> b) & 1u) {
                    if (j <= NT) tok[j] = p + 1;
                    ++j;
                }
                tb += is_tab;
            }
        }
        tabs += step_tabs;
        zone += step_zone;
    }
    __syncthreads();
    if (tabs < 12) bad = true;                    // fewer than 12 columns (11 tabs and the row end)
    const uint32_t c5 = sc[0], c6 = sc[1];
    if (tabs >= 12 && (int)(c6 - c5) - 1 != K) bad = true;      // k-mer length
    if (__ballot(bad) != 0ull) {                  // the table may be incomplete: nothing more to read from it
        if (lane == 0) a.status[row] = ROW_HOST;
        return;
    }
    const char* t = len <= lds_text ? ltext : g;
    for (int k = lane; k < K; k += 64) {
        const int code = base_code(t[c5 + 1 + k]);
        if (code < 0) bad = true;
        a.kmer[(size_t)row * K + k] = code < 0 ? 0 : code;      // never an index the embedding lookup cannot take
    }
    int32_t label = 0;
    for (int i = lane; i < NT; i += 64) {
        if (!store_token(i, K, S, t + tok[i], t + tok[i + 1] - 1, a.means + (size_t)row * K, a.stds + (size_t)row * K,
                         a.lens + (size_t)row * K, a.signals + (size_t)row * S, &label))
            bad = true;
        else if (i == NT - 1)
            a.label[row] = label;
    }
    const bool host = __ballot(bad) != 0ull;
    if (lane == 0) {
        a.info_len[row] = (int32_t)c5;
        a.status[row] = host ? ROW_HOST : ROW_OK;
    }
}

}  // namespace

size_t parse_lds_bytes(int K, int S, int* text_bytes)
{
    const size_t table = ((size_t)ntokens(K, S) + 1 + N_SCALARS) * 4;
    if (table > LDS_MAX) { if (text_bytes) *text_bytes = 0; return 0; }
    const int text = table + LDS_TEXT <= LDS_MAX ? LDS_TEXT : 0;
    if (text_bytes) *text_bytes = text;
    return table + (size_t)text;
}

hipError_t launch_parse(const ParseArgs& a, hipStream_t stream)
{
    int text = 0;
    const size_t lds = parse_lds_bytes(a.K, a.S, &text);
    if (!lds || a.n < 1) return hipErrorInvalidValue;
    hipLaunchKernelGGL(tsv_parse_kernel, dim3(a.n), dim3(64), lds, stream, a, text);
    return hipGetLastError();
}

void parse_reference(int K, int S, const char* text, int64_t nrows, const int64_t* begin, const int64_t* end, int32_t* kmer,
                     float* means, float* stds, float* lens, float* signals, int32_t* label, int32_t* info_len, int32_t* status)
{
    const int NT = ntokens(K, S);
    for (int64_t r = 0; r < nrows; ++r) {
        status[r] = ROW_HOST;
        const char* b = text + begin[r];
        const char* e = text + end[r];
        if (e < b) continue;
        // col[c] = start of column c; col[12] = one past the separator that closes column 11 (a tab, or the row end)
        const char* col[13];
        col[0] = b;
        int nc = 1;
        for (const char* p = b; p < e && nc < 13; ++p)
            if (*p == '\t') col[nc++] = p + 1;
        if (nc < 12) continue;
        if (nc == 12) col[12] = e + 1;
        if (col[7] - 1 - col[6] != K) continue;
        bool ok = true;
        for (int k = 0; k < K && ok; ++k) {
            const int code = base_code(col[6][k]);
            if (code < 0) ok = false; else kmer[r * K + k] = code;
        }
        int t = 0;
        for (int c = 7; c <= 11 && ok; ++c) {
            const int want = c == 7 ? K : c == 8 ? 2 * K : c == 9 ? 3 * K : c == 10 ? 3 * K + S : NT;
            const char* ce = col[c + 1] - 1;
            const char* p = col[c];
            for (;;) {
                const char* q = p;
                while (q < ce && *q != ',') ++q;
                if (c == 11) q = ce;                  // the label is one token whatever it holds
                if (t >= want || !store_token(t, K, S, p, q, means + r * K, stds + r * K, lens + r * K, signals + r * S, &label[r])) { ok = false; break; }
                ++t;
                if (q == ce) break;
                p = q + 1;
            }
            if (t != want) ok = false;
        }
        if (!ok) continue;
        info_len[r] = (int32_t)(col[6] - 1 - b);
        status[r] = ROW_OK;
    }
}

}  // namespace dst
