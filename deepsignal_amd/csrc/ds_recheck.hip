// ds_recheck.hip — cascaded precision (ds_set_recheck): which sites of a finished coarse forward go to the fine handle, and their
// inputs compacted for it. Built with -ffp-contract=off: the selection rule is two float32 subtractions / additions, one
// multiplication and one comparison, each rounded on its own, so numpy float32 reproduces it bit for bit.
#include "ds_internal.h"

namespace ds {

namespace {

constexpr int RC_THREADS = 256;              // sites per workgroup (one lane each), four waves
constexpr int RC_WAVES = RC_THREADS / 64;

// site i is selected iff d < margin * s, or d or s is not finite (include/deepsignal_hip.h ds_set_recheck)
__device__ __forceinline__ bool recheck_rule(const float* __restrict__ act, int C, int i, float margin)
{
    const float a0 = act[(size_t)i * C], a1 = act[(size_t)i * C + 1];
    const float d = fabsf(a1 - a0);
    const float s = a0 + a1;
    const float m = margin * s;
    // finite <=> the exponent field is not all ones (a bit test: no compiler flag can fold it away)
    const bool fin = ((__float_as_uint(d) & 0x7f800000u) != 0x7f800000u) && ((__float_as_uint(s) & 0x7f800000u) != 0x7f800000u);
    return d < m || !fin;
}

}  // namespace

// One lane per site. Slots come out in ascending site order without any atomic: a workgroup first COUNTS the selected sites in
// front of its own 256 (every workgroup re-evaluates the rule on them: 8 bytes per site out of L2, n is a few thousand), then
// places its own by a wave ballot + the count of selected lower lanes and a scan over its four waves' totals. The workgroup then
// copies the input rows of its selected sites, a site at a time, consecutive lanes writing consecutive 4-byte words of the
// site's five rows (T and S are arbitrary, so a row's 16-byte alignment is not given). The last workgroup writes the count.
__global__ __launch_bounds__(RC_THREADS) void recheck_select_kernel(const RecheckArgs a)
{
    __shared__ int wave_cnt[RC_WAVES];
    __shared__ int wave_pre[RC_WAVES];
    __shared__ int sel_site[RC_THREADS];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int base = blockIdx.x * RC_THREADS;
    const unsigned long long lower = (1ull << lane) - 1ull;

    // (1) selected sites in [0, base)
    int before = 0;
    for (int i0 = 0; i0 < base; i0 += RC_THREADS) {      // base is a multiple of RC_THREADS: every lane has a site
        const unsigned long long b = __ballot(recheck_rule(a.act, a.C, i0 + tid, a.margin));
        before += __popcll(b);
    }
    if (lane == 0) wave_pre[wave] = before;
    // (2) this workgroup's own sites
    const int site = base + tid;
    const bool sel = site < a.n && recheck_rule(a.act, a.C, site, a.margin);
    const unsigned long long ball = __ballot(sel);
    if (lane == 0) wave_cnt[wave] = __popcll(ball);
    __syncthreads();
    int before_wg = 0, earlier_waves = 0, own = 0;       // each wave counted its own lanes' share of [0, base)
    for (int w = 0; w < RC_WAVES; ++w) {
        before_wg += wave_pre[w];
        if (w < wave) earlier_waves += wave_cnt[w];
        own += wave_cnt[w];
    }
    const int slot = before_wg + earlier_waves + __popcll(ball & lower);
    if (sel) {
        a.index[slot] = site;
        sel_site[slot - before_wg] = site;
    }
    if (blockIdx.x == gridDim.x - 1 && tid == 0) a.count[0] = before_wg + own;
    __syncthreads();
    // (3) the rows of this workgroup's selected sites
    const int T = a.T, S = a.S, words = 4 * T + S;
    for (int k = 0; k < own; ++k) {
        const int src = sel_site[k];
        const size_t dst = (size_t)(before_wg + k);
        for (int w = tid; w < words; w += RC_THREADS) {
            if (w < 4 * T) {
                const int r = w / T, c = w - r * T;       // 0 kmer (int32 bits travel as a 4-byte word), 1 means, 2 stds, 3 sanums
                a.out[(size_t)r * a.B * T + dst * T + c] = a.in[(size_t)r * a.B * T + (size_t)src * T + c];
            } else {
                const int c = w - 4 * T;
                a.out[(size_t)4 * a.B * T + dst * S + c] = a.in[(size_t)4 * a.B * T + (size_t)src * S + c];
            }
        }
    }
}

hipError_t launch_recheck_select(const RecheckArgs& a, hipStream_t s)
{
    if (a.n <= 0) return hipSuccess;
    const int grid = (a.n + RC_THREADS - 1) / RC_THREADS;
    hipLaunchKernelGGL(recheck_select_kernel, dim3(grid), dim3(RC_THREADS), 0, s, a);
    return hipGetLastError();
}

}  // namespace ds
