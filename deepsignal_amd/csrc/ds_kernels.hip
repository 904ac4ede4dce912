// ds_kernels.hip — gfx950 (CDNA4 / MI355X) kernels of the call_mods forward pass.
//
// Kernels, by role (DESIGN.md section 4 has the table): a whole-module fused inception kernel (fp32 and bf16 operand
// forms), a conv_layer2 + conv_layer3 kernel, dedicated BiLSTM cell kernels of one anti-diagonal per launch (operands
// direct to registers, or shared through an LDS-DMA ring), an implicit-GEMM template (the 6032 x 6032 dense layer of
// the three-step joint model, the bf16-mode stem convolutions, the layer-granular diagnostic path), and small kernels
// for the Cin = 1 stem conv, the pools, the folded / two-class head and the input gather.
//
// Design notes (MI355X_MICROARCH.md / cdna_hip_programming.md):
//  * v_mfma_f32_32x32x2_f32 is exact fp32 (an fmaf chain) at 64 FLOP/clk/SIMD and needs only ONE
//    VGPR per operand per lane, so the weight (B) operand is pre-packed on the host in fragment
//    order and streamed global->VGPR with 1 KiB coalesced wave loads (no LDS round trip), while the
//    activation (A) tile is staged through LDS once per K-chunk and shared by all waves.
//  * K is consumed in groups of 8 with a lane-local permutation (lane half h owns k = 4h..4h+3 of
//    the group) so one ds_read_b128 / one global_load_dwordx4 feeds four consecutive MFMAs.
//  * LDS rows are padded to KC+4 floats: the 16-lane ds_read_b128 groups hit 16 distinct 16-B slots.
//  * wave64 everywhere; no CUDA-isms, no compatibility shims.
#include "ds_device.h"

namespace ds {


// ---- K loop of the fp32 dense instantiation (CFG_FC_DENSE: the 6032 x 6032 layer of the three-step joint model, 128 x 96 tile,
// four waves that own 32 rows each and share the three weight n-tiles).
// The template's generic loop streams the weights global -> VGPR in every wave: per 16-wide K chunk a workgroup asks for 24 KB of
// which 6 KB are distinct, and the two-chunk look-ahead is a register ring of 96 VGPRs (212 in all). Here the six 1 KiB weight
// fragments of a chunk go global -> LDS ONCE per workgroup by LDS-DMA into a ring of DR_SLOTS stages (lstm_cell_lds_kernel's
// request form: plain requests, counted vmcnt, the chunk's one barrier), and a wave reads them LDS -> VGPR one read step ahead
// of its MFMAs: two read steps' worth (24 VGPRs) are live. The activations keep their path (global -> VGPR -> ds_write_b128
// into rows padded to KC + 4 floats, double-buffered; LDS-DMA cannot write padded rows).
//   * One vmcnt counter serves the requests AND the activation loads, and hipcc does not see the requests: a load it knows of
//     would get a wait that counts only the loads it knows, i.e. one that also drains every request issued before the youngest
//     of them. So the activation loads are inline asm too and every vector-memory wait of the loop is counted by hand. Per chunk
//     a wave issues, in this order, 2 activation loads (chunk c + 2) and 2 requests (chunk c + DR_DIST); memory operations
//     retire in issue order, so `vmcnt(6)` before the ds_writes of chunk c + 1 leaves exactly {requests of c + 2, loads of
//     c + 2, requests of c + 3} in flight and has retired the requests of chunk c + 1 as well, which the barrier behind it
//     publishes to the other waves.
//   * Six fragments over four waves: waves 0 / 1 request fragments (w, w + 4), waves 2 / 3 request fragment w and refetch it
//     into a pad (SplitRing's filler), so the count is the same literal in every wave.
//   * Past the last chunk the cursors stay on it (scalar selects): the loop body has no look-ahead conditionals, the surplus
//     requests and loads refetch the last chunk into slots nobody reads again, and `vmcnt(0)` behind the loop retires them
//     before their target registers are reused.
//   * Sources are wave-uniform scalar bases advanced by scalar adds plus loop-invariant lane offsets: no VALU in the loop.
//   * The order inside a step is pinned instruction by instruction (sched_barrier): one non-MFMA instruction behind one MFMA.
//   * Per accumulator the MFMAs run in the generic loop's order (chunk, read step, x y z w): bit-identical results.
// What it buys: 286 -> 262 us per launch alone (the matrix pipe 82 -> 90 % busy) and a quarter of the weight requests. At 129
// VGPRs and 46 KB a workgroup would also fit beside a fused inception module (2 x 184 VGPRs per SIMD, 111 KB of LDS); that
// placement was measured and loses, so the launch keeps one dense workgroup per CU (launch_gemm, DR_SOLO_PAD_BYTES).
// Ring slot of chunk c is c % 4, activation buffer c & 1; a slot is requested again one barrier after its last read retired
// (`lgkmcnt(0)` in front of every barrier).
constexpr int DR_SLOTS = 4;                      // ring stages of one chunk
constexpr int DR_DIST = 3;                       // chunks between a request and the step that multiplies it
constexpr int DR_STAGE = 6 * 256;                // floats: 3 n-tiles x 2 k-groups of 1 KiB
constexpr int DR_A_FLOATS = 2 * 128 * (KC + 4);
constexpr int DR_LDS_FLOATS = DR_A_FLOATS + DR_SLOTS * DR_STAGE + 2 * 256;      // + the pad of waves 2 and 3: 47,104 B
constexpr int DR_SOLO_PAD_BYTES = 56 * 1024;      // unused dynamic LDS of the launch (launch_gemm): one dense workgroup per CU

// The load is asynchronous: dst holds the data only behind the hand-counted `s_waitcnt vmcnt` asm that names it as "+v". hipcc
// takes dst for written here, so a copy or a spill of it between the two statements would carry stale registers. Nothing forces
// the two together; what holds it is that R[][] has no other use in between (today's code keeps each R in one register quadruple,
// no v_mov in the loop), tests/test_dense_cotenancy_budget.py (no spills, no scratch) and the bitwise checks of
// tests/test_gpu_dense_ring.py, which a stale row fails.
__device__ __forceinline__ void dr_gload4(v4f& dst, unsigned voff, const void* sbase)
{
    asm volatile("global_load_dwordx4 %0, %1, %2" : "=&v"(dst) : "v"(voff), "s"(sbase) : "memory");
}
template <int E> __device__ __forceinline__ float dr_elem(const v4f& v) { return E == 0 ? v.x : E == 1 ? v.y : E == 2 ? v.z : v.w; }

__device__ __forceinline__ void dense_ring_loop(const GemmProblem& P, float* smem, int m0, int tid, int lane, int wave,
                                                int t0, int t1, int t2, floatx16 (&acc)[1][3])
{
    constexpr int LDA = KC + 4;
    const int nchunks = P.K / KC;
    if (nchunks <= 0) return;
    float* const ring = smem + DR_A_FLOATS;
    const unsigned ring_lds = (unsigned)(size_t)(__attribute__((address_space(3))) float*)ring;
    const unsigned lane16 = (unsigned)lane * 16;

    // ---- weight requests: fragment q = 2 nt + kg of a chunk lies at ring slot + q KiB
    const char* bsrc[2];
    unsigned bdst[2], bdstep[2];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int q = wave + 4 * j;
        const bool own = q < 6;
        const int qq = own ? q : wave, nt = qq >> 1, kg = qq & 1;
        const int tile = nt == 0 ? t0 : nt == 1 ? t1 : t2;
        bsrc[j] = reinterpret_cast<const char*>(P.Bp) + ((size_t)tile * P.kgroups_stride + kg) * 1024;
        bdst[j] = own ? ring_lds + q * 1024 : ring_lds + DR_SLOTS * DR_STAGE * 4 + (wave - 2) * 1024;
        bdstep[j] = own ? DR_STAGE * 4 : 0;
    }
    int breq_left = nchunks - 1;
    auto request0 = [&](int slot) __attribute__((always_inline)) { glds16s(bsrc[0], lane16, bdst[0] + slot * bdstep[0]); };
    auto request1 = [&](int slot) __attribute__((always_inline)) {
        glds16s(bsrc[1], lane16, bdst[1] + slot * bdstep[1]);
        const long inc = breq_left > 0 ? 2 * 1024 : 0;
        --breq_left;
        bsrc[0] += inc;
        bsrc[1] += inc;
    };

    // ---- activation cursor: row tile and chunk in the scalar base, the lane's row and 16 bytes in a 32-bit offset
    unsigned avoff[2];
    const char* abase = nullptr;
    int seg_i = 0, seg_left = 0;
    const int nseg = P.nseg;
    auto seg_begin = [&](int si) __attribute__((always_inline)) {
        const int ld = P.seg[si].ld;
        seg_left = P.seg[si].klen / KC;
        abase = reinterpret_cast<const char*>(P.seg[si].base + (size_t)(m0 + P.seg[si].row_shift) * ld);
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int idx = tid + i * 256;
            avoff[i] = ((unsigned)(idx >> 2) * (unsigned)ld + (idx & 3) * 4) * 4;
        }
    };
    auto advance_a = [&]() __attribute__((always_inline)) {
        if (--seg_left == 0) {
            if (seg_i + 1 < nseg) seg_begin(++seg_i);
            else seg_left = 1;                      // past the end: stay on the last chunk
        } else {
            abase += KC * 4;
        }
    };

    v4f R[2][2];                 // activation rows in flight: chunk k in R[k & 1]
    v4f af[2][2], b[2][3];       // fragments: af[chunk & 1][read step], b[read step][n-tile]
    const float* const fa = smem + ((wave * 32 + (lane & 31)) * LDA + (lane >> 5) * 4);
    float* const wa = smem + ((tid >> 2) * LDA + (tid & 3) * 4);
    const float* const fb = ring + lane * 4;

    // ---- prologue: the queue is left as every step expects it: ..., loads of chunk 1, requests of chunk 2
    seg_begin(0);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    dr_gload4(R[0][0], avoff[0], abase);
    dr_gload4(R[0][1], avoff[1], abase);
    advance_a();
    request0(0); request1(0);
    request0(1); request1(1);
    dr_gload4(R[1][0], avoff[0], abase);
    dr_gload4(R[1][1], avoff[1], abase);
    advance_a();
    request0(2); request1(2);
    asm volatile("s_waitcnt vmcnt(4)" : "+v"(R[0][0]), "+v"(R[0][1]) : : "memory");
    *reinterpret_cast<v4f*>(wa) = R[0][0];
    *reinterpret_cast<v4f*>(wa + 64 * LDA) = R[0][1];
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
    af[0][0] = *reinterpret_cast<const v4f*>(fa);
    af[0][1] = *reinterpret_cast<const v4f*>(fa + 8);
#pragma unroll
    for (int nt = 0; nt < 3; ++nt) b[0][nt] = *reinterpret_cast<const v4f*>(fb + nt * 512);

    // one chunk: X = its activation buffer, Q = its ring slot. MFMA m of a read step (n-tile m / 4, element m % 4), then one
    // other instruction, then a scheduling barrier.
#define DR_MFMA(RS, M_)                                                                                                        \
    acc[0][(M_) / 4] = __builtin_amdgcn_mfma_f32_32x32x2f32(dr_elem<(M_) % 4>(af[X][RS]), dr_elem<(M_) % 4>(b[RS][(M_) / 4]),                 \
                                                             acc[0][(M_) / 4], 0, 0, 0)
#define DR_PIN __builtin_amdgcn_sched_barrier(0)
    auto step = [&](auto xc, auto qc) __attribute__((always_inline)) {
        constexpr int X = decltype(xc)::value, Q = decltype(qc)::value;
        constexpr int XN = X ^ 1, QN = (Q + 1) % DR_SLOTS, QR = (Q + DR_DIST) % DR_SLOTS;
        DR_PIN;
        DR_MFMA(0, 0); dr_gload4(R[X][0], avoff[0], abase); DR_PIN;
        DR_MFMA(0, 1); dr_gload4(R[X][1], avoff[1], abase); DR_PIN;
        DR_MFMA(0, 2); request0(QR); DR_PIN;
        DR_MFMA(0, 3); request1(QR); DR_PIN;
        DR_MFMA(0, 4); b[1][0] = *reinterpret_cast<const v4f*>(fb + Q * DR_STAGE + 256); DR_PIN;
        DR_MFMA(0, 5); b[1][1] = *reinterpret_cast<const v4f*>(fb + Q * DR_STAGE + 768); DR_PIN;
        DR_MFMA(0, 6); b[1][2] = *reinterpret_cast<const v4f*>(fb + Q * DR_STAGE + 1280); DR_PIN;
        DR_MFMA(0, 7);
        asm volatile("s_waitcnt vmcnt(6)" : "+v"(R[XN][0]), "+v"(R[XN][1]) : : "memory");
        *reinterpret_cast<v4f*>(wa + XN * 128 * LDA) = R[XN][0]; DR_PIN;
        DR_MFMA(0, 8); *reinterpret_cast<v4f*>(wa + XN * 128 * LDA + 64 * LDA) = R[XN][1]; DR_PIN;
        DR_MFMA(0, 9); DR_PIN;
        DR_MFMA(0, 10); advance_a(); DR_PIN;
        DR_MFMA(0, 11); DR_PIN;
        asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
        DR_PIN;
        DR_MFMA(1, 0); af[XN][0] = *reinterpret_cast<const v4f*>(fa + XN * 128 * LDA); DR_PIN;
        DR_MFMA(1, 1); af[XN][1] = *reinterpret_cast<const v4f*>(fa + XN * 128 * LDA + 8); DR_PIN;
        DR_MFMA(1, 2); b[0][0] = *reinterpret_cast<const v4f*>(fb + QN * DR_STAGE); DR_PIN;
        DR_MFMA(1, 3); b[0][1] = *reinterpret_cast<const v4f*>(fb + QN * DR_STAGE + 512); DR_PIN;
        DR_MFMA(1, 4); b[0][2] = *reinterpret_cast<const v4f*>(fb + QN * DR_STAGE + 1024); DR_PIN;
        DR_MFMA(1, 5); DR_PIN;
        DR_MFMA(1, 6); DR_PIN;
        DR_MFMA(1, 7); DR_PIN;
        DR_MFMA(1, 8); DR_PIN;
        DR_MFMA(1, 9); DR_PIN;
        DR_MFMA(1, 10); DR_PIN;
        DR_MFMA(1, 11); DR_PIN;
    };
    for (int c = 0;;) {
        step(LdsSlot<0>{}, LdsSlot<0>{}); if (++c >= nchunks) break;
        step(LdsSlot<1>{}, LdsSlot<1>{}); if (++c >= nchunks) break;
        step(LdsSlot<0>{}, LdsSlot<2>{}); if (++c >= nchunks) break;
        step(LdsSlot<1>{}, LdsSlot<3>{}); if (++c >= nchunks) break;
    }
#undef DR_MFMA
#undef DR_PIN
    // the surplus loads and requests of the last steps: retired before their registers and the ring are given up
    asm volatile("s_waitcnt vmcnt(0)" : "+v"(R[0][0]), "+v"(R[0][1]), "+v"(R[1][0]), "+v"(R[1][1]) : : "memory");
}

// BF = bf16 operands. The byte geometry is the same as fp32: a "unit" is 4 bytes (one float or two bf16), a
// K chunk is 16 units = 64 B per row (16 floats / 32 bf16), one 16-B fragment per lane feeds four
// v_mfma_f32_32x32x2_f32 (fp32) or ONE v_mfma_f32_32x32x16_bf16 (lane half h owns k = 8h..8h+7 of the 16).
// The host passes ld / klen / K of bf16 operands in units, so the staging code is shared.
// KS is 1 in every instantiation (it was an in-workgroup K split that no plan selected, retired to
// profiles/experiments/); the parameter stays because the kernel names in the kernel table and the committed profiles carry it.
template <int MT, int NT, int WM, int WN, int EPI, int AMODE, int BD, int KS, bool BF = false>
__global__ __launch_bounds__(64 * WM * WN, (AMODE == 2 && !BF) ? 3 : 1) void gemm_kernel(const GemmLaunch* __restrict__ L)
{
    static_assert(KS == 1, "the in-workgroup K split is retired (profiles/EXPERIMENTS.md)");
    constexpr int BM = WM * MT * 32;
    constexpr int LDA = KC + 4;
    constexpr int NTHR = 64 * WM * WN;
    constexpr int SLOTS = (BM * 4 + NTHR - 1) / NTHR;
    // the fp32 dense instantiation has a K loop of its own (dense_ring_loop): its weights come through an LDS ring behind the A buffers.
    // AMODE 2 without BF is FC1 of the three-step joint model and nothing else (plan_joint_model: n % 128 == 0, row_shift 0, W = M,
    // every segment a positive multiple of KC wide); dense_ring_loop relies on all of that -- it has no row masks, no W bounds and
    // no empty segments. Its __launch_bounds__ second argument (3 waves per SIMD) is a REGISTER budget, not an occupancy: with
    // 46 KB of static LDS hipcc derives the budget from the LDS-limited occupancy anyway (three workgroups per CU: 168 VGPRs), and 3
    // states the same; the kernel takes 129. How many workgroups share a CU is decided at the launch (launch_gemm: one).
    constexpr bool RING = AMODE == 2 && !BF;
    static_assert(!RING || (MT == 1 && NT == 3 && WM == 4 && WN == 1 && 2 * BM * LDA == DR_A_FLOATS), "dense_ring_loop is written for the 128 x 96 tile");
    __shared__ __attribute__((aligned(16))) float smem_[RING ? DR_LDS_FLOATS : 2 * BM * LDA];

    // the wave index is wave-uniform, but hipcc cannot prove it from threadIdx: readfirstlane keeps the
    // segment-cursor logic on the scalar unit (otherwise it becomes exec-masked vector code)
    const int lane = threadIdx.x & 63, wave_all = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    // kl is 0 (a workgroup is NTHR threads) and hipcc folds it, but late: with the literal in its place the same instructions come
    // out on other scalar registers in every instantiation. It stays in these five lines so that the device code is the measured one.
    const int kl = wave_all / (WM * WN);
    const int wave = wave_all % (WM * WN);
    const int tid = threadIdx.x - kl * NTHR;
    float* const As0 = smem_ + kl * BM * LDA;
    float* const As1 = smem_ + (1 + kl) * BM * LDA;
    const int wm = wave % WM, wn = wave / WM;
    // XCD-aware tile order: hardware deals workgroup b to XCD b % 8, each with a private L2. Give every XCD a
    // contiguous run of logical tiles (m-tiles of one weight panel are neighbours), so a weight panel is pulled
    // into ONE L2 instead of up to eight (PMC: FC1 fetched its 146 MB of weights 4x before this remap).
    int bid;
    {
        const int total = L->total_tiles, q = total >> 3, r = total & 7;
        const int xcd = blockIdx.x & 7, idx = blockIdx.x >> 3;
        bid = xcd * q + (xcd < r ? xcd : r) + idx;
    }
    int pi = 0;
    for (int i = 1; i < L->nprob; ++i)
        if (bid >= L->prob[i].tile_start) pi = i;
    const GemmProblem& P = L->prob[pi];
    const int local = bid - P.tile_start;
    // neighbours in the logical order share the bigger operand: the weight panel (m fastest) for FC / LSTM
    // shapes, the activation rows (n fastest) for the convolutions
    const int tm = P.n_fast ? local / P.tiles_n : local % P.tiles_m;
    const int tn = P.n_fast ? local % P.tiles_n : local / P.tiles_m;
    const int m0 = tm * BM;
    const int M = P.M, W = P.W;
    const int nchunks = P.K / KC;               // (the planner pads K to a multiple of KC)
    const int nseg = P.nseg;

    // per-slot row bookkeeping (a slot = one float4 of the staged A chunk)
    int sm[SLOTS], sw[SLOTS];
    bool sin_[SLOTS];
#pragma unroll
    for (int i = 0; i < SLOTS; ++i) {
        const int idx = tid + i * NTHR;
        sm[i] = m0 + (idx >> 2);
        sin_[i] = (idx < BM * 4) && (sm[i] < M);
        sw[i] = sm[i] % W;
    }

    int ntile[NT];
    bool nvalid[NT];
    const float* bp[NT];
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
        ntile[nt] = (tn * WN + wn) * NT + nt;
        nvalid[nt] = ntile[nt] < P.ntiles32;
        const int tcl = nvalid[nt] ? ntile[nt] : P.ntiles32 - 1;   // clamp: loads stay in bounds, result unused
        bp[nt] = P.Bp + ((size_t)tcl * P.kgroups_stride + kl * 2) * 256 + lane * 4;
    }

    floatx16 acc[MT][NT];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
        for (int nt = 0; nt < NT; ++nt)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[mt][nt][r] = 0.0f;

    if constexpr (RING) {
        auto tile_of = [&](int nt) { return nvalid[nt] ? ntile[nt] : P.ntiles32 - 1; };      // clamp: requests stay in bounds, result unused
        dense_ring_loop(P, smem_, m0, tid, lane, wave, tile_of(0), tile_of(1), tile_of(2), acc);
    } else {
    // A cursor: branch-free loads. Every slot always loads from a legal address (its own row when
    // valid, the segment base otherwise) and invalid slots are zeroed by a select afterwards.
    const float* ap[SLOTS];
    const float* apm[SLOTS];   // AMODE 1: previous / next row (clamped to the own row at site edges)
    const float* app[SLOTS];
    bool aok[SLOTS];
    int seg_i = 0, seg_left = 0;
    auto seg_begin = [&](int si) {
        const float* base = P.seg[si].base;
        const int ld = P.seg[si].ld;
        const int shift = P.seg[si].row_shift;
        seg_left = P.seg[si].klen / KC;
#pragma unroll
        for (int i = 0; i < SLOTS; ++i) {
            const int idx = tid + i * NTHR;
            const int ws = sw[i] + shift;
            aok[i] = sin_[i] && (unsigned)ws < (unsigned)W;
            const float* q = base + (size_t)(sm[i] + shift) * ld + (idx & 3) * 4;
            ap[i] = aok[i] ? q : base;
            if (AMODE == 1) {
                apm[i] = (aok[i] && sw[i] > 0) ? q - ld : ap[i];
                app[i] = (aok[i] && sw[i] < W - 1) ? q + ld : ap[i];
            }
        }
    };
    auto advance = [&]() {
        if (--seg_left == 0 && ++seg_i < nseg) seg_begin(seg_i);
    };
    // Software pipeline (per chunk c, parity X = c&1; chunk k lives in R[k&1] / b[k&1] / As[k&1] / a[k&1]):
    //   (1) issue global loads: A rows of chunk c+2 -> R[X], weights of chunk c+BD -> b[(c+BD) % (BD+1)]
    //       (BD = weight prefetch distance in chunks: 1 for L2-resident weights, 2 when they stream from HBM)
    //   (2) write chunk c+1 (loaded one step ago) to LDS As[X^1] (SAME-padding select / 3-tap max applied here)
    //   (3) MFMAs of read-step 0 of chunk c
    //   (4) barrier                       -- everyone's (2) is done
    //   (5) ds_read chunk c+1 fragments -> a[X^1]   (latency hidden by (6))
    //   (6) MFMAs of read-step 1 of chunk c
    // One barrier per chunk, no load / LDS latency on the MFMA critical path.
    // BD == 3 ("deep"): activations AND weights are requested two full chunks ahead through rings of three register
    // buffers (chunk k in R[k % 3] / bq[k % 3]; four would not fit 256 VGPRs next to a 1x4 accumulator tile). For
    // bf16 operands a chunk is only ~256 matrix-pipe cycles, so one step of look-ahead cannot cover an L2 / HBM
    // round trip.
    constexpr int RA = BD == 3 ? 3 : 2;
    float4 R[RA][SLOTS], Rm[RA][SLOTS], Rp[RA][SLOTS];
    bool lok[RA][SLOTS];
    float4 bq[BD == 3 ? 3 : 2 * BD][NT][2];   // weight ring: 2 buffers (BD=1), 4 (BD=2) or 3 (BD=3), statically indexed
    float4 af[2][2][MT];
    auto load_a = [&](int X) {
#pragma unroll
        for (int i = 0; i < SLOTS; ++i) {
            R[X][i] = gload4(ap[i]);
            ap[i] += KC;
            if (AMODE == 1) {
                Rm[X][i] = gload4(apm[i]);
                Rp[X][i] = gload4(app[i]);
                apm[i] += KC;
                app[i] += KC;
            }
            if (AMODE != 2) lok[X][i] = aok[i];
        }
        advance();
    };
    auto store_a = [&](int X, int P = -1) {      // ring slot X -> LDS buffer P (default: the slot's own parity)
        float* dst = (P < 0 ? X : P) ? As1 : As0;
#pragma unroll
        for (int i = 0; i < SLOTS; ++i) {
            const int idx = tid + i * NTHR;
            float4 v = R[X][i];
            if (AMODE == 1) v = BF ? bf8max_relu(bf8max_relu(v, Rm[X][i]), Rp[X][i])
                                   : f4max_relu(f4max_relu(v, Rm[X][i]), Rp[X][i]);   // maxpool(3, s1, SAME): padded taps ignored
            if (AMODE != 2) {     // AMODE 2 = dense: every row of every tile is valid, no taps -> no select
                v.x = lok[X][i] ? v.x : 0.0f;
                v.y = lok[X][i] ? v.y : 0.0f;
                v.z = lok[X][i] ? v.z : 0.0f;
                v.w = lok[X][i] ? v.w : 0.0f;
            }
            if (SLOTS * NTHR == BM * 4 || idx < BM * 4)
                *reinterpret_cast<float4*>(dst + (idx >> 2) * LDA + (idx & 3) * 4) = v;
        }
    };
    auto load_b = [&](int X) {
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) {
            bq[X][nt][0] = gload4(bp[nt]);
            bq[X][nt][1] = gload4(bp[nt] + 256);
            bp[nt] += 512;
        }
    };
    auto read_frags = [&](int X) {
#pragma unroll
        for (int rs = 0; rs < 2; ++rs)
#pragma unroll
            for (int mt = 0; mt < MT; ++mt)
                af[X][rs][mt] = *reinterpret_cast<const float4*>(
                    (X ? As1 : As0) + ((wm * MT + mt) * 32 + (lane & 31)) * LDA + rs * 8 + (lane >> 5) * 4);
    };
    // X / JC / JN are literals at every call site, so all register arrays are statically indexed
    auto mfma_rs2 = [&](int X, int J, int rs) {
#pragma unroll
        for (int mt = 0; mt < MT; ++mt)
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) {
                if (BF) {
                    acc[mt][nt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, af[X][rs][mt]),
                                                                          __builtin_bit_cast(bf16x8, bq[J][nt][rs]), acc[mt][nt], 0, 0, 0);
                    continue;
                }
                acc[mt][nt] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[X][rs][mt].x, bq[J][nt][rs].x, acc[mt][nt], 0, 0, 0);
                acc[mt][nt] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[X][rs][mt].y, bq[J][nt][rs].y, acc[mt][nt], 0, 0, 0);
                acc[mt][nt] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[X][rs][mt].z, bq[J][nt][rs].z, acc[mt][nt], 0, 0, 0);
                acc[mt][nt] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[X][rs][mt].w, bq[J][nt][rs].w, acc[mt][nt], 0, 0, 0);
            }
    };
    // Instruction interleave inside a step (sched_group_barrier, cdna_hip_programming.md T19): with one
    // wave per SIMD a burst of loads / LDS ops in front of the MFMA block leaves the matrix pipe idle
    // while they issue, so each non-MFMA instruction is slotted behind one MFMA instead.
    //   masks: VALU 0x2, MFMA 0x8, VMEM read 0x20, DS read 0x100, DS write 0x200
    constexpr int N_MFMA_HALF = MT * NT * (BF ? 1 : 4);
    constexpr int N_ALOADS = SLOTS * (AMODE == 1 ? 3 : 1);
    constexpr int N_BLOADS = 2 * NT;
    constexpr int N_VALU_PER_STORE = (AMODE == 1 ? 12 : AMODE == 2 ? 0 : 4);
    // deep variant: chunk c sits in ring slot Q = c % 3 and LDS buffer X = c & 1
#define DS_STEPD(X, Q, HAS1, HAS3)                                                        \
    do {                                                                                  \
        if (HAS3) { load_a(((Q) + 2) % 3); load_b(((Q) + 2) % 3); }                       \
        if (HAS1) store_a(((Q) + 1) % 3, (X) ^ 1);                                        \
        mfma_rs2(X, Q, 0);                                                                \
        if (HAS1) {                                                                       \
            _Pragma("unroll") for (int i_ = 0; i_ < SLOTS; ++i_) {                        \
                __builtin_amdgcn_sched_group_barrier(0x8, 1, 0);                          \
                if (N_VALU_PER_STORE) __builtin_amdgcn_sched_group_barrier(0x2, N_VALU_PER_STORE, 0); \
                __builtin_amdgcn_sched_group_barrier(0x200, 1, 0);                        \
            }                                                                             \
        }                                                                                 \
        if (HAS3) {                                                                       \
            _Pragma("unroll") for (int i_ = 0; i_ < N_ALOADS + N_BLOADS; ++i_) {          \
                __builtin_amdgcn_sched_group_barrier(0x8, 1, 0);                          \
                __builtin_amdgcn_sched_group_barrier(0x20, 1, 0);                         \
            }                                                                             \
        }                                                                                 \
        __builtin_amdgcn_sched_group_barrier(0x8, N_MFMA_HALF, 0);                        \
        __builtin_amdgcn_sched_barrier(0);                                                \
        __syncthreads();                                                                  \
        if (HAS1) read_frags((X) ^ 1);                                                    \
        mfma_rs2(X, Q, 1);                                                                \
        __builtin_amdgcn_sched_group_barrier(0x8, 1, 0);                                  \
        if (HAS1) __builtin_amdgcn_sched_group_barrier(0x100, 2 * MT, 0);                 \
        __builtin_amdgcn_sched_group_barrier(0x8, N_MFMA_HALF, 0);                        \
        __builtin_amdgcn_sched_barrier(0);                                                \
    } while (0)
#define DS_STEP(X, JC, JN, HAS1, HAS2, HASB)                                              \
    do {                                                                                  \
        if (HAS2) load_a(X);                                                              \
        if (HASB) load_b(JN);                                                             \
        if (HAS1) store_a((X) ^ 1);                                                       \
        mfma_rs2(X, JC, 0);                                                               \
        if (HAS1) {                                                                       \
            _Pragma("unroll") for (int i_ = 0; i_ < SLOTS; ++i_) {                        \
                __builtin_amdgcn_sched_group_barrier(0x8, 1, 0);                          \
                if (N_VALU_PER_STORE) __builtin_amdgcn_sched_group_barrier(0x2, N_VALU_PER_STORE, 0); \
                __builtin_amdgcn_sched_group_barrier(0x200, 1, 0);                        \
            }                                                                             \
        }                                                                                 \
        if (HAS2) {                                                                       \
            _Pragma("unroll") for (int i_ = 0; i_ < N_ALOADS; ++i_) {                     \
                __builtin_amdgcn_sched_group_barrier(0x8, 1, 0);                          \
                __builtin_amdgcn_sched_group_barrier(0x20, 1, 0);                         \
            }                                                                             \
        }                                                                                 \
        if (HASB) {                                                                       \
            _Pragma("unroll") for (int i_ = 0; i_ < N_BLOADS; ++i_) {                     \
                __builtin_amdgcn_sched_group_barrier(0x8, 1, 0);                          \
                __builtin_amdgcn_sched_group_barrier(0x20, 1, 0);                         \
            }                                                                             \
        }                                                                                 \
        __builtin_amdgcn_sched_group_barrier(0x8, N_MFMA_HALF, 0);                        \
        __builtin_amdgcn_sched_barrier(0);                                                \
        __syncthreads();                                                                  \
        if (HAS1) read_frags((X) ^ 1);                                                    \
        mfma_rs2(X, JC, 1);                                                               \
        __builtin_amdgcn_sched_group_barrier(0x8, 1, 0);                                  \
        if (HAS1) __builtin_amdgcn_sched_group_barrier(0x100, 2 * MT, 0);                 \
        __builtin_amdgcn_sched_group_barrier(0x8, N_MFMA_HALF, 0);                        \
        __builtin_amdgcn_sched_barrier(0);                                                \
    } while (0)

    if (nchunks > 0) {
        seg_begin(0);
        load_a(0);
        load_b(0);
        store_a(0);
        if (nchunks > 1) load_a(1);
        if (BD >= 2 && nchunks > 1) load_b(1);
        __syncthreads();
        read_frags(0);
        int c = 0;
        if (BD == 3) {
            // six steps per trip: LDS parity has period 2, the register rings period 3
            while (c + 7 < nchunks) {      // chunks c .. c+5 with every look-ahead (up to c+7) in range
                DS_STEPD(0, 0, true, true);
                DS_STEPD(1, 1, true, true);
                DS_STEPD(0, 2, true, true);
                DS_STEPD(1, 0, true, true);
                DS_STEPD(0, 1, true, true);
                DS_STEPD(1, 2, true, true);
                c += 6;
            }
            // tail: 1..7 chunks left, runtime (wave-uniform) look-ahead flags
            DS_STEPD(0, 0, c + 1 < nchunks, c + 2 < nchunks);
            if (++c < nchunks) {
                DS_STEPD(1, 1, c + 1 < nchunks, c + 2 < nchunks);
                if (++c < nchunks) {
                    DS_STEPD(0, 2, c + 1 < nchunks, c + 2 < nchunks);
                    if (++c < nchunks) {
                        DS_STEPD(1, 0, c + 1 < nchunks, c + 2 < nchunks);
                        if (++c < nchunks) {
                            DS_STEPD(0, 1, c + 1 < nchunks, c + 2 < nchunks);
                            if (++c < nchunks) {
                                DS_STEPD(1, 2, c + 1 < nchunks, false);
                                if (++c < nchunks) DS_STEPD(0, 0, false, false);
                            }
                        }
                    }
                }
            }
        } else if (BD == 1) {
            while (c + 3 < nchunks) {      // steady state: every look-ahead exists, no conditionals
                DS_STEP(0, 0, 1, true, true, true);
                DS_STEP(1, 1, 0, true, true, true);
                c += 2;
            }
            const int left = nchunks - c;  // 1..3
            if (left == 3) {
                DS_STEP(0, 0, 1, true, true, true);
                DS_STEP(1, 1, 0, true, false, true);
                DS_STEP(0, 0, 1, false, false, false);
            } else if (left == 2) {
                DS_STEP(0, 0, 1, true, false, true);
                DS_STEP(1, 1, 0, false, false, false);
            } else {
                DS_STEP(0, 0, 1, false, false, false);
            }
        } else {
            while (c + 5 < nchunks) {
                DS_STEP(0, 0, 2, true, true, true);
                DS_STEP(1, 1, 3, true, true, true);
                DS_STEP(0, 2, 0, true, true, true);
                DS_STEP(1, 3, 1, true, true, true);
                c += 4;
            }
            // tail: 1..5 chunks, runtime (wave-uniform) look-ahead flags
            DS_STEP(0, 0, 2, c + 1 < nchunks, c + 2 < nchunks, c + 2 < nchunks);
            if (++c < nchunks) {
                DS_STEP(1, 1, 3, c + 1 < nchunks, c + 2 < nchunks, c + 2 < nchunks);
                if (++c < nchunks) {
                    DS_STEP(0, 2, 0, c + 1 < nchunks, c + 2 < nchunks, c + 2 < nchunks);
                    if (++c < nchunks) {
                        DS_STEP(1, 3, 1, c + 1 < nchunks, c + 2 < nchunks, c + 2 < nchunks);
                        if (++c < nchunks) DS_STEP(0, 0, 2, false, false, false);
                    }
                }
            }
        }
    }
#undef DS_STEP
#undef DS_STEPD
    }

    // ---------------- epilogue ----------------
    const int rbase = m0 + wm * MT * 32 + 4 * (lane >> 5);
    if (EPI == 0) {
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) {
            const int col = ntile[nt] * 32 + (lane & 31);
            if (!nvalid[nt] || col >= P.N) continue;
            int sel = 0;
            for (int o = 1; o < P.nout; ++o)
                if (col >= P.out[o].col0) sel = o;
            const OSeg os = P.out[sel];
            const int cc = col - os.col0;
            const float bias = P.bias ? gload(P.bias + col) : 0.0f;
#pragma unroll
            for (int mt = 0; mt < MT; ++mt)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int row = rbase + mt * 32 + (r & 3) + 8 * (r >> 2);
                    if (row < M) {
                        float v = acc[mt][nt][r] + bias;
                        if (os.add) v += gload(os.add + (size_t)row * os.add_ld + cc);
                        if (os.relu) v = relu_f(v);
                        if (BF && os.bf16)
                            *(__attribute__((address_space(1))) unsigned short*)((unsigned short*)os.base + (size_t)row * os.ld + cc) = f2bf(v);
                        else
                            gstore(os.base + (size_t)row * os.ld + cc, v);
                    }
                }
        }
    }
    static_assert(EPI == 0, "the BiLSTM epilogues left this template in round 3 (lstm_cell_*kernel)");
}

TileGeom gemm_geom(GemmCfg cfg)
{
    switch (cfg) {
    case CFG_CONV: return {128, 64, 256};        // MT1 NT2 WM4 WN1
    case CFG_FC: return {128, 96, 256};          // MT1 NT3 WM4 WN1, weights prefetched 2 chunks ahead
    case CFG_CONV_POOL: return {128, 64, 256};   // CFG_CONV with maxpool(3,s1) fused into the A load
    case CFG_FC_DENSE: return {128, 96, 256};    // CFG_FC for M % 128 == 0 (no row masks)
    case CFG_BCONV: return {128, 64, 256};       // bf16 operands, same staging as CFG_CONV
    case CFG_BCONV_POOL: return {128, 64, 256};
    case CFG_BFC: return {128, 256, 256};        // MT4 NT2 WM1 WN4: every wave owns all 128 rows x 64 columns, so a
    case CFG_BFC_DENSE: return {128, 256, 256};  // weight fragment is loaded by exactly one wave of the workgroup
    }
    return {0, 0, 0};
}

hipError_t launch_gemm(GemmCfg cfg, const GemmLaunch* d_launch, int total_tiles, hipStream_t s)
{
    if (total_tiles <= 0) return hipSuccess;
    // CFG_CONV_POOL / CFG_BCONV_POOL (AMODE 1) pool with f4max_relu / bf8max_relu: their A operand must come from a relu epilogue
    // (os.relu set in the producing launch, or stem1 / a fused module); on signed values the unsigned maximum is wrong.
    switch (cfg) {
    case CFG_CONV: hipLaunchKernelGGL((gemm_kernel<1, 2, 4, 1, 0, 0, 1, 1>), dim3(total_tiles), dim3(256), 0, s, d_launch); break;
    case CFG_FC: hipLaunchKernelGGL((gemm_kernel<1, 3, 4, 1, 0, 0, 2, 1>), dim3(total_tiles), dim3(256), 0, s, d_launch); break;
    case CFG_CONV_POOL: hipLaunchKernelGGL((gemm_kernel<1, 2, 4, 1, 0, 1, 1, 1>), dim3(total_tiles), dim3(256), 0, s, d_launch); break;
    case CFG_FC_DENSE:
        // ONE dense workgroup per CU, set by an unused dynamic LDS allocation (DR_SOLO_PAD_BYTES; the limit is raised once per device in
        // configure_fused_kernels). The ring loop's own footprint (129 VGPRs, 46 KB of static LDS) lets the dispatcher stack three dense
        // workgroups on a CU or put one beside a fused module, where no BiLSTM cell fits any more; launched that way the pipelined step
        // is SLOWER than the parent's (-1.7 %), with 46 + 56 KB -- room for four cell workgroups beside it and nothing else -- it is
        // faster (+2.2 %): profiles/dense_ring_ab.json, profiles/EXPERIMENTS.md. 46 + 52 KB would seat a FIFTH cell workgroup (158 KB,
        // 136 + 5 x 72 = 496 registers per SIMD): measured, -0.1 % alone and no better than 56 KB at any cell priority (profiles/cell_guest_ab.json).
        hipLaunchKernelGGL((gemm_kernel<1, 3, 4, 1, 0, 2, 2, 1>), dim3(total_tiles), dim3(256), DR_SOLO_PAD_BYTES, s, d_launch);
        break;
    case CFG_BCONV: hipLaunchKernelGGL((gemm_kernel<1, 2, 4, 1, 0, 0, 1, 1, true>), dim3(total_tiles), dim3(256), 0, s, d_launch); break;
    case CFG_BCONV_POOL: hipLaunchKernelGGL((gemm_kernel<1, 2, 4, 1, 0, 1, 1, 1, true>), dim3(total_tiles), dim3(256), 0, s, d_launch); break;
    case CFG_BFC: hipLaunchKernelGGL((gemm_kernel<4, 2, 1, 4, 0, 0, 2, 1, true>), dim3(total_tiles), dim3(256), 0, s, d_launch); break;
    case CFG_BFC_DENSE: hipLaunchKernelGGL((gemm_kernel<4, 2, 1, 4, 0, 2, 2, 1, true>), dim3(total_tiles), dim3(256), 0, s, d_launch); break;
    default: return hipErrorInvalidValue;      // the BiLSTM cells run in their own kernels (lstm_cell_*), not through this template
    }
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------
// fp32 BiLSTM cells of one wavefront diagonal (layers.py:45-72; TF LSTMCell: gate order i, j, f, o, forget_bias 1.0
// added at run time; c' = sigmoid(f + 1) c + sigmoid(i) tanh(j); h' = sigmoid(o) tanh(c')).
//
// A workgroup = 4 INDEPENDENT waves (no LDS, no barrier): wave w owns the 32 sites of m-tile 4*mb + w and NT n-tiles of
// 32 gate columns ([gate][8 units] order, so a lane ends up with the four gates of four neighbouring units of ONE
// site). Both operands stream global -> VGPR in MFMA-fragment order with 1 KiB coalesced wave loads, four k-groups
// ahead of the matrix pipe: the weights as packed by the host, the activations because the previous cell's epilogue
// wrote h in exactly that order (ds_internal.h, LstmCell). The product is issued transposed -- mfma(weights, h) --
// as in the fused inception kernel. Bias (+1 on the forget gate) and, for layer 0, the embedding-table row and the
// (mean, std, len) rank-1 terms are the accumulator's INITIAL value, computed while the first fragments are in
// flight; the previous cell state is requested up front as well, so the epilogue is pure gate arithmetic + two
// coalesced 1 KiB stores.
// Roofline: MFMA (fp32, 64 FLOP/clk/SIMD). Algorithmic FLOPs per launch = sum over cells of 2 * n * 1024 * K.
template <int NT>
__global__ __launch_bounds__(256, NT == 1 ? 4 : 2) void lstm_cell_kernel(const LstmLaunch L_)
{
    const LstmLaunch* const Lp = &L_;      // by-value kernel argument: the descriptor arrives with the dispatch packet (kernarg
                                           // segment) instead of behind a cold pointer chase at the start of every workgroup
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    // diagnostic stamps (wave 0, lane 0 of every workgroup; only when a debug buffer is attached):
    // [0] s_memrealtime at entry (100 MHz, comparable across CUs)  [1..4] s_memtime (shader clock) at entry / before the
    // K loop / after it / at exit  [5] s_memrealtime at exit  [6] HW_ID  [7] XCC_ID
    unsigned long long* const sdst = (Lp->dbg && blockIdx.x < DBG_MAX_WGS) ? Lp->dbg + (size_t)blockIdx.x * 8 : nullptr;
    const bool stamp = sdst != nullptr && threadIdx.x == 0;
#define DS_LSTAMP(i, v) do { if (stamp) sdst[i] = (v); } while (0)
    DS_LSTAMP(0, __builtin_amdgcn_s_memrealtime());
    DS_LSTAMP(1, __builtin_amdgcn_s_memtime());
    DS_LSTAMP(6, (unsigned long long)__builtin_amdgcn_s_getreg(63492));     // HW_REG_HW_ID, all 32 bits
    DS_LSTAMP(7, (unsigned long long)__builtin_amdgcn_s_getreg(63508));     // HW_REG_XCC_ID
    const int bid = lstm_logical_tile(blockIdx.x, gridDim.x, Lp->cls_tiles[0], Lp->cls_tiles[1]);   // work-balanced, XCD-aware order
    const int mtiles = Lp->mtiles;
    const int mblocks = (mtiles + 3) >> 2;
    constexpr int NGROUPS = 32 / NT;
    const int per_cell = mblocks * NGROUPS;
    const int ci = bid / per_cell, rem = bid - ci * per_cell;
    const int mb = rem % mblocks, ng = rem / mblocks;
    const int mt = mb * 4 + wave;
    if (mt >= mtiles) return;                       // waves are independent: a ragged last m-block just has fewer of them
    const LstmCell& C = Lp->cell[ci];
    const int half = lane >> 5, r31 = lane & 31;
    const int n = Lp->n, T = Lp->T;
    const int row = mt * 32 + r31;
    const int rowc = row < n ? row : n - 1;         // padding rows of the last m-tile compute on a copy of the last site

    // ---- requests that the accumulator's initial value needs
    floatx16 acc[NT];
    float4 cp[NT];
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) lstm_acc_init(C, (ng * NT + nt) * 8 + 4 * half, rowc, T, acc[nt]);
    const unsigned lane4 = (unsigned)lane * 4;
    const size_t mt_off = (size_t)mt * LSTM_MT_FLOATS;
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
        cp[nt] = make_float4(0.f, 0.f, 0.f, 0.f);
        if (!C.c_zero) cp[nt] = gload4(C.c + mt_off + (unsigned)(ng * NT + nt) * 256 + lane4);
    }

    // ---- K loop: k-groups of 8 (one 16-byte fragment per lane and operand = four MFMAs), a ring of four register
    // stages; x rows first, then h rows, as in the TF kernel (and in the packed weights)
    const bool has_x = C.ax != nullptr, has_h = C.ah != nullptr;
    const int KG = (has_x ? 32 : 0) + (has_h ? 32 : 0);
    // one linear k-group index for both segments: group kg lives at a0 + kg KiB (+ the distance between the two
    // buffers from group 32 on when both are present) -- scalar arithmetic only, no branch in the loop
    const char* const a0 = reinterpret_cast<const char*>(has_x ? C.ax : C.ah) + mt_off * 4;
    const long dseg = (has_x && has_h) ? (reinterpret_cast<const char*>(C.ah) - reinterpret_cast<const char*>(C.ax)) - 32 * 1024 : 0;
    const char* bpn[NT];
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) bpn[nt] = reinterpret_cast<const char*>(C.Bp + (size_t)(ng * NT + nt) * C.kg_stride * 256);
    const unsigned lane16 = (unsigned)lane * 16;
    DS_LSTAMP(2, __builtin_amdgcn_s_memtime());
    if (KG > 0) {
        float4 a[4], b[4][NT];
        auto request = [&](int slot, int kg) {           // slot is a literal at every call site
            const int kc = min(kg, KG - 1);              // past the end: re-request the last group (never consumed)
            const long aoff = (long)kc * 1024 + (kc >= 32 ? dseg : 0);                               // wave-uniform
            a[slot] = gload4(reinterpret_cast<const float*>(a0 + aoff + lane16));
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) b[slot][nt] = gload4(reinterpret_cast<const float*>(bpn[nt] + (long)kc * 1024 + lane16));
        };
        auto consume = [&](int slot) {
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) {
                acc[nt] = __builtin_amdgcn_mfma_f32_32x32x2f32(b[slot][nt].x, a[slot].x, acc[nt], 0, 0, 0);
                acc[nt] = __builtin_amdgcn_mfma_f32_32x32x2f32(b[slot][nt].y, a[slot].y, acc[nt], 0, 0, 0);
                acc[nt] = __builtin_amdgcn_mfma_f32_32x32x2f32(b[slot][nt].z, a[slot].z, acc[nt], 0, 0, 0);
                acc[nt] = __builtin_amdgcn_mfma_f32_32x32x2f32(b[slot][nt].w, a[slot].w, acc[nt], 0, 0, 0);
            }
        };
        request(0, 0); request(1, 1); request(2, 2); request(3, 3);
        for (int kg = 0; kg < KG; kg += 4) {             // KG is 32 or 64
            // sched_barrier pins the ring: without it hipcc sinks all eight requests to the bottom of the trip, and a
            // stage's operands are then only ~1 stage ahead of their MFMAs instead of 4
            consume(0); request(0, kg + 4); __builtin_amdgcn_sched_barrier(0);
            consume(1); request(1, kg + 5); __builtin_amdgcn_sched_barrier(0);
            consume(2); request(2, kg + 6); __builtin_amdgcn_sched_barrier(0);
            consume(3); request(3, kg + 7); __builtin_amdgcn_sched_barrier(0);
        }
    }
    DS_LSTAMP(3, __builtin_amdgcn_s_memtime());

    // ---- gates, new state, coalesced fragment-major stores
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
        const int ntile = ng * NT + nt;
        float4 cn, hn;
        lstm_gates(acc[nt], cp[nt], cn, hn);
        const size_t off = mt_off + (unsigned)ntile * 256 + lane4;
        const v4f co = {cn.x, cn.y, cn.z, cn.w}, ho = {hn.x, hn.y, hn.z, hn.w};
        *(__attribute__((address_space(1))) v4f*)(C.c + off) = co;
        *(__attribute__((address_space(1))) v4f*)(C.h_out + off) = ho;
        if (C.h_row && row < n)
            *(__attribute__((address_space(1))) v4f*)(C.h_row + (size_t)row * 256 + ntile * 8 + 4 * half) = ho;
    }
    DS_LSTAMP(4, __builtin_amdgcn_s_memtime());
    DS_LSTAMP(5, __builtin_amdgcn_s_memrealtime());
#undef DS_LSTAMP
}

// The same cells with the operands SHARED through LDS. A CU's vector-memory path moves ~64 B/clk at best; the
// direct-to-register kernel above asks it for 32 B/clk/CU (every wave fetches its own 1 KiB activation and weight
// fragment per four MFMAs), which is what bounds it. Here a workgroup owns a 64-site x (64 * NT)-column block: waves
// (mi, nj) = (wave & 1, wave >> 1) take m-tile mi and the NT n-tiles of column group nj, so every activation
// fragment feeds two waves and every weight fragment two waves -- half the global traffic per MFMA. Fragments are
// 1 KiB images in global memory already, so they go global -> LDS by LDS-DMA (no VGPR round trip): a ring of three
// stages of KGS k-groups (1 at NT = 1, 2 at NT = 2), requests two stages ahead, ONE barrier per stage, a counted vmcnt in
// front of it so the next stage's requests stay in flight across the barrier.
// (glds16 / glds16s, the LDS-DMA requests, live in ds_device.h)
//
// DS_CELL_PRIO: issue priority (s_setprio) of a cell wave from the K loop's entry on; it goes back to 0 behind the loop, or, with
// DS_CELL_PRIO_GATES = 1, behind the gate arithmetic and the stores. A cell workgroup is a guest on a CU whose fused-module or
// dense waves live 100 - 300 us, are the oldest, and win every oldest-first arbitration among equals; and the joint model of a
// forward waits for the 19 dependent cell launches, not for the signal branch (median 582 us, in every forward:
// profiles/branch_balance_parent.json). Measured on the pipelined 512-site step against the parent (0), libraries alternating,
// four runs a side, k sites/s (profiles/cell_guest_ab.json): K loop only, level 1 / 2 / 3: 450.1 / 450.1 / 449.7 against 447.8
// (+0.5 / +0.5 / +0.4 %); held through the gates, level 1: 453.0 (+1.16 %); a session of its own, held through the gates, level
// 1 / 2 / 3: 455.1 / 454.8 / 455.5 against 450.1 (+1.1 / +1.1 / +1.2 %, the three within the parent's own 0.24 % spread). The
// epilogue's 40 transcendental instructions are where a guest waits longest for issue, so more than half of the gain is there;
// the level does not matter, so it is the lowest. The code is the parent's but for the two s_setprio (and one s_nop count behind
// the loop); results are bit-identical.
#ifndef DS_CELL_PRIO
#define DS_CELL_PRIO 1
#endif
#ifndef DS_CELL_PRIO_GATES
#define DS_CELL_PRIO_GATES 1
#endif
__device__ __forceinline__ floatx16 mfma_bf_early(float4 a, float4 b, floatx16 c)
{
    return __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), c, 0, 0, 0);
}

template <int NT>
__global__ __launch_bounds__(256, NT == 1 ? 7 : 2) void lstm_cell_lds_kernel(const LstmLaunch L_)
{
    const LstmLaunch* const Lp = &L_;      // by-value kernel argument (see lstm_cell_kernel)
    constexpr int FR = 2 + 2 * NT;            // fragments per k-group: 2 m-tiles of h, 2 * NT n-tiles of weights
    constexpr int KGS = NT == 1 ? 1 : 2;      // k-groups per stage (KGS * FR fragments, a multiple of the four waves)
    constexpr int LPS = KGS * FR / 4;         // DMA requests per wave and stage
    constexpr int STAGE = KGS * FR * 256;     // floats
    // Dynamic on purpose: with a static array hipcc derives the register budget from the LDS-limited occupancy and ignores
    // __launch_bounds__. Footprint per workgroup (NT = 1): 12 KB of LDS and 70 VGPRs per wave (72 granted) -- up to seven
    // workgroups per CU, and TWO of them fit next to a fused-module workgroup (2 x 184 + 2 x 72 = 512 VGPRs per SIMD, 111 +
    // 2 x 12 KB; tests/test_cell_cotenancy_budget.py). The K loop needs ~30 registers; the budget is set by the prologue, which
    // is why lstm_acc_init loads the layer-0 terms in two groups and addresses everything as scalar base + 32-bit lane offset.
    // Measured at 512 sites per forward (ring = 3 stages of KGS k-groups): KGS 4 / 136 VGPRs 545 k sites/s, KGS 2 / 88 VGPRs
    // 554 k, KGS 1 / 88 VGPRs 561 k (one barrier per four MFMAs of a wave, but more waves per SIMD to hide it).
    extern __shared__ __attribute__((aligned(16))) float ring[];      // [3 * STAGE]

    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int mi = wave & 1, nj = wave >> 1;
    // diagnostic stamps (wave 0, lane 0 of every workgroup; only when a debug buffer is attached):
    // [0] s_memrealtime at entry (100 MHz, comparable across CUs)  [1..4] s_memtime (shader clock) at entry / before the
    // K loop / after it / at exit  [5] s_memrealtime at exit  [6] HW_ID  [7] XCC_ID
    unsigned long long* const sdst = (Lp->dbg && blockIdx.x < DBG_MAX_WGS) ? Lp->dbg + (size_t)blockIdx.x * 8 : nullptr;
    const bool stamp = sdst != nullptr && threadIdx.x == 0;
#define DS_LSTAMP(i, v) do { if (stamp) sdst[i] = (v); } while (0)
    DS_LSTAMP(0, __builtin_amdgcn_s_memrealtime());
    DS_LSTAMP(1, __builtin_amdgcn_s_memtime());
    DS_LSTAMP(6, (unsigned long long)__builtin_amdgcn_s_getreg(63492));     // HW_REG_HW_ID, all 32 bits
    DS_LSTAMP(7, (unsigned long long)__builtin_amdgcn_s_getreg(63508));     // HW_REG_XCC_ID
    const int bid = lstm_logical_tile(blockIdx.x, gridDim.x, Lp->cls_tiles[0], Lp->cls_tiles[1]);   // work-balanced, XCD-aware order
    const int mtiles = Lp->mtiles;
    const int mblocks = (mtiles + 1) >> 1;
    constexpr int NGROUPS = 16 / NT;
    const int per_cell = mblocks * NGROUPS;
    const int ci = bid / per_cell, rem = bid - ci * per_cell;
    const int mb = rem % mblocks, ng = rem / mblocks;
    const LstmCell& C = Lp->cell[ci];
    const int mt_raw = mb * 2 + mi;
    const bool valid = mt_raw < mtiles;                       // odd m-tile count: the last block's second half idles along
    const int mt = valid ? mt_raw : mtiles - 1;
    const int half = lane >> 5, r31 = lane & 31;
    const int n = Lp->n, T = Lp->T;
    const int row = mt * 32 + r31;
    const int rowc = row < n ? row : n - 1;
    const unsigned lane16 = (unsigned)lane * 16;

    const bool has_x = C.ax != nullptr, has_h = C.ah != nullptr;
    const int KG = (has_x ? 32 : 0) + (has_h ? 32 : 0);
    const int nstages = KG / KGS;
    const char* const a0 = reinterpret_cast<const char*>(has_x ? C.ax : C.ah);
    const long dseg = (has_x && has_h) ? (reinterpret_cast<const char*>(C.ah) - reinterpret_cast<const char*>(C.ax)) - 32 * 1024 : 0;
    // request j of this wave: linear fragment index q = wave + 4 j of the stage -> (k-group kgi, fragment f). The
    // source of a request is WAVE-UNIFORM up to the lane's 16 bytes, so it is kept as a scalar base (advanced with
    // scalar adds) plus one loop-invariant VGPR offset: on gfx950 a VALU instruction does not run in the shadow of an
    // fp32 MFMA (tools/attic/mfma_valu.hip) -- per-lane 64-bit pointer arithmetic in the K loop is matrix-pipe time lost.
    const char* src[LPS];
    int kgi_[LPS];
    bool is_a[LPS];
#pragma unroll
    for (int j = 0; j < LPS; ++j) {
        const int q = wave + 4 * j, kgi = q / FR, f = q - kgi * FR;
        kgi_[j] = kgi;
        is_a[j] = f < 2;
        if (f < 2) {
            const int m = min(mb * 2 + f, mtiles - 1);
            src[j] = a0 + (size_t)m * LSTM_MT_FLOATS * 4 + (size_t)kgi * 1024;
        } else {
            const int ntile = ng * 2 * NT + (f - 2);
            src[j] = reinterpret_cast<const char*>(C.Bp) + ((size_t)ntile * C.kg_stride + kgi) * 1024;
        }
    }
    const unsigned ring_lds = (unsigned)(size_t)(__attribute__((address_space(3))) float*)ring;    // LDS byte address
    auto request = [&](int st, int slot) __attribute__((always_inline)) {      // stage st -> ring slot st % 3
        const unsigned dst = __builtin_amdgcn_readfirstlane(ring_lds + (slot * STAGE + wave * 256) * 4);
#pragma unroll
        for (int j = 0; j < LPS; ++j) {
            const int kg = st * KGS + kgi_[j];
            const long off = (long)st * (KGS * 1024) + ((is_a[j] && kg >= 32) ? dseg : 0);
            glds16s(src[j] + off, lane16, dst + j * 4096);     // fragment q = wave + 4 j of the stage, 1 KiB each
        }
    };
    if (nstages > 0) request(0, 0);
    if (nstages > 1) request(1, 1);

    // ---- accumulator's initial value: bias (+1 on f), layer 0: table row + (mean, std, len) terms
    floatx16 acc[NT];
    float4 cp[NT];
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) lstm_acc_init(C, ((ng * 2 + nj) * NT + nt) * 8 + 4 * half, rowc, T, acc[nt]);
    const size_t mt_off = (size_t)mt * LSTM_MT_FLOATS;
    const unsigned lane4 = (unsigned)lane * 4;
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
        cp[nt] = make_float4(0.f, 0.f, 0.f, 0.f);
        if (!C.c_zero) cp[nt] = gload4(C.c + mt_off + (unsigned)(((ng * 2 + nj) * NT + nt)) * 256 + lane4);
    }

    // every compiler-visible load is retired here, so hipcc has no reason to put a vmcnt wait into the loop below (it
    // cannot see the LDS-DMA requests, which are counted by hand)
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
        asm volatile("" : "+v"(cp[nt].x), "+v"(cp[nt].y), "+v"(cp[nt].z), "+v"(cp[nt].w));
        asm volatile("" : "+v"(acc[nt]));          // bias loads land directly in the accumulator registers
    }
    DS_LSTAMP(2, __builtin_amdgcn_s_memtime());
    if constexpr (DS_CELL_PRIO != 0) __builtin_amdgcn_s_setprio(DS_CELL_PRIO);      // the K loop's issue priority (see DS_CELL_PRIO)
    // stage st has landed in LDS once every wave's requests for it are done: counted wait (stage st + 1 stays in
    // flight), then the barrier; it also tells everybody that ring slot (st + 2) % 3 -- read during stage st - 1 -- is
    // free again. The ring index is a compile-time constant of each of the three unrolled bodies, so every LDS address
    // is a loop-invariant VGPR plus an immediate.
    const float* const fa0 = ring + mi * 256 + lane4;
    const float* const fb0 = ring + (2 + nj * NT) * 256 + lane4;
    auto stage = [&](int st, auto slot_c) __attribute__((always_inline)) {
        constexpr int SLOT = decltype(slot_c)::value;
        if (st + 1 < nstages) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(LPS) : "memory");
        else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        if (st + 2 < nstages) request(st + 2, (SLOT + 2) % 3);
#pragma unroll
        for (int kgi = 0; kgi < KGS; ++kgi) {
            const float4 a = *reinterpret_cast<const float4*>(fa0 + SLOT * STAGE + kgi * FR * 256);
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) {
                const float4 b = *reinterpret_cast<const float4*>(fb0 + SLOT * STAGE + (kgi * FR + nt) * 256);
                acc[nt] = __builtin_amdgcn_mfma_f32_32x32x2f32(b.x, a.x, acc[nt], 0, 0, 0);
                acc[nt] = __builtin_amdgcn_mfma_f32_32x32x2f32(b.y, a.y, acc[nt], 0, 0, 0);
                acc[nt] = __builtin_amdgcn_mfma_f32_32x32x2f32(b.z, a.z, acc[nt], 0, 0, 0);
                acc[nt] = __builtin_amdgcn_mfma_f32_32x32x2f32(b.w, a.w, acc[nt], 0, 0, 0);
            }
        }
    };
    for (int st = 0; st < nstages;) {
        stage(st, LdsSlot<0>{}); if (++st >= nstages) break;
        stage(st, LdsSlot<1>{}); if (++st >= nstages) break;
        stage(st, LdsSlot<2>{}); ++st;
    }

    DS_LSTAMP(3, __builtin_amdgcn_s_memtime());
    if constexpr (DS_CELL_PRIO != 0 && !DS_CELL_PRIO_GATES) __builtin_amdgcn_s_setprio(0);
    if (!valid) return;
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
        const int ntile = (ng * 2 + nj) * NT + nt;
        float4 cn, hn;
        lstm_gates(acc[nt], cp[nt], cn, hn);
        const size_t off = mt_off + (unsigned)ntile * 256 + lane4;
        const v4f co = {cn.x, cn.y, cn.z, cn.w}, ho = {hn.x, hn.y, hn.z, hn.w};
        *(__attribute__((address_space(1))) v4f*)(C.c + off) = co;
        *(__attribute__((address_space(1))) v4f*)(C.h_out + off) = ho;
        if (C.h_row && row < n)
            *(__attribute__((address_space(1))) v4f*)(C.h_row + (size_t)row * 256 + ntile * 8 + 4 * half) = ho;
    }
    if constexpr (DS_CELL_PRIO != 0 && DS_CELL_PRIO_GATES) __builtin_amdgcn_s_setprio(0);
    DS_LSTAMP(4, __builtin_amdgcn_s_memtime());
    DS_LSTAMP(5, __builtin_amdgcn_s_memrealtime());
#undef DS_LSTAMP
}

// ---------------------------------------------------------------------------------------------
// The same cells with bf16 OPERANDS (DS_PRECISION_BF16_ALL): h and the weights are bf16, products accumulate in fp32
// (v_mfma_f32_32x32x16_bf16), the layer-0 table row / rank-1 terms, the gates and the cell state stay fp32.
//
// A bf16 MFMA does 16x the work of an fp32 one per cycle, so what bounds this kernel is operand delivery, not the matrix
// pipe: a diagonal at 4096 sites per forward moves ~75 MB (c: 8 MB per cell read + written in fp32, h: 4 + 2 MB, weights
// 1 MB) for 21 GFLOP -- ~20 us of memory against ~9 us of MFMA at peak. Design for bytes per MFMA:
//   * workgroup tile = 64 MTW sites x 64 NTW columns, 4 waves as 2 x 2, each wave MTW x NTW tiles of 32 x 32: at 2 x 2 a
//     k-step (16 k) needs 8 KB from L2 for 16 MFMAs -- 0.5 KB per MFMA (the round-1 template re-loaded every weight
//     fragment in each of its four waves: 1.25 KB per MFMA) -- and 1 KB of LDS reads per MFMA;
//   * operands are 1 KiB fragment images in global memory (weights packed so by the host; h because the previous cell's
//     epilogue wrote it so) and go global -> LDS by LDS-DMA, ring of three stages of two k-steps, one barrier per stage
//     behind a counted vmcnt -- the structure of lstm_cell_lds_kernel;
//   * h lives FRAGMENT-MAJOR in bf16: [m-tile of 32 sites][k-step of 16 units][64 lanes][8 bf16], lane (r, half) holding
//     units 16 s + 8 half .. + 7 of site 32 m + r. A lane of the epilogue owns four neighbouring units of one site
//     (8 bytes): lanes (r, 0) and (r, 1) of an n-tile fill the two halves of one 16-byte slot, a wave store covers 512
//     contiguous bytes. c keeps the fp32 kernels' fragment-major layout.
// Roofline: HBM / L2 (operand delivery). Algorithmic FLOPs per launch = sum over cells of 2 * n * 1024 * K.
constexpr int LSTM_MT_BYTES_BF16 = 32 * 256 * 2;      // one m-tile of a bf16 fragment-major h buffer
template <int MTW, int NTW>
__global__ __launch_bounds__(256, MTW * NTW >= 4 ? 2 : 3) void lstm_cell_bf16_kernel(const LstmLaunch L_)
{
    const LstmLaunch* const Lp = &L_;
    constexpr int FRA = 2 * MTW, FRB = 2 * NTW, FR = FRA + FRB;     // 1 KiB fragments per k-step: m-tiles of h, n-tiles of weights
    constexpr int KGS = 2;                                          // k-steps per ring stage
    constexpr int NF = KGS * FR;                                    // fragments per stage (a multiple of the four waves)
    static_assert(NF % 4 == 0, "fragments of a stage are dealt to four waves");
    constexpr int LPS = NF / 4;                                     // DMA requests per wave and stage
    constexpr int STAGE = NF * 256;                                 // floats
    extern __shared__ __attribute__((aligned(16))) float ring[];    // [3 * STAGE]

    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int mi = wave & 1, nj = wave >> 1;
    unsigned long long* const sdst = (Lp->dbg && blockIdx.x < DBG_MAX_WGS) ? Lp->dbg + (size_t)blockIdx.x * 8 : nullptr;
    const bool stamp = sdst != nullptr && threadIdx.x == 0;
#define DS_LSTAMP(i, v) do { if (stamp) sdst[i] = (v); } while (0)
    DS_LSTAMP(0, __builtin_amdgcn_s_memrealtime());
    DS_LSTAMP(1, __builtin_amdgcn_s_memtime());
    DS_LSTAMP(6, (unsigned long long)__builtin_amdgcn_s_getreg(63492));
    DS_LSTAMP(7, (unsigned long long)__builtin_amdgcn_s_getreg(63508));
    const int bid = lstm_logical_tile(blockIdx.x, gridDim.x, Lp->cls_tiles[0], Lp->cls_tiles[1]);
    const int mtiles = Lp->mtiles;
    const int mblocks = (mtiles + FRA - 1) / FRA;
    constexpr int NGROUPS = 32 / FRB;
    const int per_cell = mblocks * NGROUPS;
    const int ci = bid / per_cell, rem = bid - ci * per_cell;
    // n-groups of one m-block are neighbours (the fp32 kernels walk the m-blocks of one weight panel instead): the workgroups
    // an XCD has resident at one time then cover a few m-blocks x ALL n-groups -- every h fragment is fetched into that L2
    // once and used by eight workgroups, and the cell's whole weight matrix (1 MB in bf16) stays resident beside it
    const int ng = rem % NGROUPS, mb = rem / NGROUPS;
    const LstmCell& C = Lp->cell[ci];
    const int half = lane >> 5, r31 = lane & 31;
    const int n = Lp->n, T = Lp->T;
    const unsigned lane16 = (unsigned)lane * 16, lane4 = (unsigned)lane * 4;

    const bool has_x = C.ax != nullptr, has_h = C.ah != nullptr;
    const int KS = (has_x ? 16 : 0) + (has_h ? 16 : 0);             // k-steps of 16: x rows first, then h rows (TF kernel order)
    const int nstages = KS / KGS;
    const char* const a0 = reinterpret_cast<const char*>(has_x ? C.ax : C.ah);
    const long dseg = (has_x && has_h) ? (reinterpret_cast<const char*>(C.ah) - reinterpret_cast<const char*>(C.ax)) - 16 * 1024 : 0;
    // request j of this wave = fragment q = wave + 4 j of a stage -> (k-step kgi inside the stage, fragment f of the k-step);
    // sources are wave-uniform bases (scalar adds in the loop) + one loop-invariant lane offset
    const char* src[LPS];
    int kgi_[LPS];
    bool is_a[LPS];
#pragma unroll
    for (int j = 0; j < LPS; ++j) {
        const int q = wave + 4 * j, kgi = q / FR, f = q - kgi * FR;
        kgi_[j] = kgi;
        is_a[j] = f < FRA;
        if (f < FRA) {
            const int m = min(mb * FRA + f, mtiles - 1);
            src[j] = a0 + (size_t)m * LSTM_MT_BYTES_BF16 + (size_t)kgi * 1024;
        } else {
            const int ntile = ng * FRB + (f - FRA);
            src[j] = reinterpret_cast<const char*>(C.Bp) + ((size_t)ntile * C.kg_stride + kgi) * 1024;      // kg_stride: k-steps per n-tile panel
        }
    }
    const unsigned ring_lds = (unsigned)(size_t)(__attribute__((address_space(3))) float*)ring;
    auto request = [&](int st, int slot) __attribute__((always_inline)) {
        const unsigned dst = __builtin_amdgcn_readfirstlane(ring_lds + (slot * STAGE + wave * 256) * 4);
#pragma unroll
        for (int j = 0; j < LPS; ++j) {
            const int ks = st * KGS + kgi_[j];
            const long off = (long)st * (KGS * 1024) + ((is_a[j] && ks >= 16) ? dseg : 0);
            glds16s(src[j] + off, lane16, dst + j * 4096);
        }
    };
    if (nstages > 0) request(0, 0);
    if (nstages > 1) request(1, 1);

    // ---- this wave's tiles: m-tiles mb * FRA + mi * MTW + i, n-tiles ng * FRB + nj * NTW + j
    int mt[MTW];
    bool valid[MTW];
#pragma unroll
    for (int i = 0; i < MTW; ++i) {
        const int raw = mb * FRA + mi * MTW + i;
        valid[i] = raw < mtiles;
        mt[i] = valid[i] ? raw : mtiles - 1;
    }
    floatx16 acc[MTW][NTW];
    float4 cp[MTW][NTW];
#pragma unroll
    for (int i = 0; i < MTW; ++i) {
        const int row = mt[i] * 32 + r31;
        const int rowc = row < n ? row : n - 1;
#pragma unroll
        for (int j = 0; j < NTW; ++j) lstm_acc_init(C, (ng * FRB + nj * NTW + j) * 8 + 4 * half, rowc, T, acc[i][j]);
    }
    const bool c_zero = C.c_zero != 0;
#pragma unroll
    for (int i = 0; i < MTW; ++i)
#pragma unroll
        for (int j = 0; j < NTW; ++j) {
            cp[i][j] = make_float4(0.f, 0.f, 0.f, 0.f);
            if (!c_zero) cp[i][j] = gload4(C.c + (size_t)mt[i] * LSTM_MT_FLOATS + (unsigned)(ng * FRB + nj * NTW + j) * 256 + lane4);
        }
    // every compiler-visible load is retired here: the loop's vmcnt waits count the LDS-DMA requests only. (Leaving the
    // cell-state loads in flight across the first stages, with the waits widened by their number, was tried: on MI355X two
    // engines then disagreed in a few bits -- LDS-DMA requests and loads to registers do not retire strictly in issue order
    // with respect to each other, so a count cannot tell which of the two kinds is still outstanding. Requesting c late instead -- behind
    // the last ring request, the following stages waiting with vmcnt(0) -- is correct and was measured: 672 -> 662 us per step
    // at 4096 sites, 165 -> 168 us at 512: the prologue is not the c loads.)
#pragma unroll
    for (int i = 0; i < MTW; ++i)
#pragma unroll
        for (int j = 0; j < NTW; ++j) {
            asm volatile("" : "+v"(cp[i][j].x), "+v"(cp[i][j].y), "+v"(cp[i][j].z), "+v"(cp[i][j].w));
            asm volatile("" : "+v"(acc[i][j]));
        }
    DS_LSTAMP(2, __builtin_amdgcn_s_memtime());

    const float* const fa0 = ring + (mi * MTW) * 256 + lane4;
    const float* const fb0 = ring + (FRA + nj * NTW) * 256 + lane4;
    // (SplitRing::run's register-piped, pinned K loop -- ds_split.hip -- was built into this kernel in round 6, git 5dac46d: bit-identical,
    // 715 - 722 against 689 - 693 us per 4,096-site step, 159 against 163 us at 512; at 2 - 3 workgroups per CU the other waves already fill the
    // gaps that order closes for the one-wave-per-SIMD split kernels: profiles/r06_bf16_lstm_piped.json)
    auto stage = [&](int st, auto slot_c) __attribute__((always_inline)) {
        constexpr int SLOT = decltype(slot_c)::value;
        if (st + 1 < nstages) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(LPS) : "memory");
        else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        if (st + 2 < nstages) request(st + 2, (SLOT + 2) % 3);
#pragma unroll
        for (int kgi = 0; kgi < KGS; ++kgi) {
            float4 a[MTW], b[NTW];
#pragma unroll
            for (int i = 0; i < MTW; ++i) a[i] = *reinterpret_cast<const float4*>(fa0 + SLOT * STAGE + (kgi * FR + i) * 256);
#pragma unroll
            for (int j = 0; j < NTW; ++j) b[j] = *reinterpret_cast<const float4*>(fb0 + SLOT * STAGE + (kgi * FR + j) * 256);
#pragma unroll
            for (int i = 0; i < MTW; ++i)
#pragma unroll
                for (int j = 0; j < NTW; ++j) acc[i][j] = mfma_bf_early(b[j], a[i], acc[i][j]);     // transposed: (h W)^T
        }
    };
    for (int st = 0; st < nstages;) {
        stage(st, LdsSlot<0>{}); if (++st >= nstages) break;
        stage(st, LdsSlot<1>{}); if (++st >= nstages) break;
        stage(st, LdsSlot<2>{}); ++st;
    }
    DS_LSTAMP(3, __builtin_amdgcn_s_memtime());

    // ---- gates (fp32), new state; c fragment-major fp32, h fragment-major bf16 (8 bytes per lane), optional row-major fp32 h
    typedef unsigned int u2v __attribute__((ext_vector_type(2)));
#pragma unroll
    for (int i = 0; i < MTW; ++i) {
        if (!valid[i]) continue;
        const int row = mt[i] * 32 + r31;
#pragma unroll
        for (int j = 0; j < NTW; ++j) {
            const int ntile = ng * FRB + nj * NTW + j;
            float4 cn, hn;
            lstm_gates(acc[i][j], cp[i][j], cn, hn);
            const v4f co = {cn.x, cn.y, cn.z, cn.w};
            *(__attribute__((address_space(1))) v4f*)(C.c + (size_t)mt[i] * LSTM_MT_FLOATS + (unsigned)ntile * 256 + lane4) = co;
            const u2v ho = {pack_bf2(hn.x, hn.y), pack_bf2(hn.z, hn.w)};
            char* const hb = reinterpret_cast<char*>(C.h_out) + (size_t)mt[i] * LSTM_MT_BYTES_BF16 + (unsigned)(ntile >> 1) * 1024 +
                             (unsigned)(((ntile & 1) * 32 + r31) * 16 + half * 8);
            *(__attribute__((address_space(1))) u2v*)hb = ho;
            if (C.h_row && row < n) {
                const v4f hr = {hn.x, hn.y, hn.z, hn.w};
                *(__attribute__((address_space(1))) v4f*)(C.h_row + (size_t)row * 256 + ntile * 8 + 4 * half) = hr;
            }
        }
    }
    DS_LSTAMP(4, __builtin_amdgcn_s_memtime());
    DS_LSTAMP(5, __builtin_amdgcn_s_memrealtime());
#undef DS_LSTAMP
}

hipError_t launch_lstm_cells(LstmTile tile, const LstmLaunch& L, hipStream_t s)
{
    if (L.ncell <= 0 || L.mtiles <= 0) return hipSuccess;
    const dim3 grid(L.ncell * lstm_tiles_per_cell(tile, L.mtiles));
    switch (tile) {
    case LT_LDS1: hipLaunchKernelGGL(lstm_cell_lds_kernel<1>, grid, dim3(256), 3 * 1 * 4 * 1024, s, L); break;      // 3 stages x KGS x FR KiB
    case LT_LDS2: hipLaunchKernelGGL(lstm_cell_lds_kernel<2>, grid, dim3(256), 3 * 2 * 6 * 1024, s, L); break;
    // bf16-operand cells (DS_PRECISION_BF16_ALL): LT_Bmn = workgroup tile of 64 m sites x 64 n columns
    case LT_B11: hipLaunchKernelGGL((lstm_cell_bf16_kernel<1, 1>), grid, dim3(256), 3 * 2 * 4 * 1024, s, L); break;
    case LT_B12: hipLaunchKernelGGL((lstm_cell_bf16_kernel<1, 2>), grid, dim3(256), 3 * 2 * 6 * 1024, s, L); break;
    case LT_B22: hipLaunchKernelGGL((lstm_cell_bf16_kernel<2, 2>), grid, dim3(256), 3 * 2 * 8 * 1024, s, L); break;
    // (a 128 x 256 tile -- a wave owning 64 sites x 128 columns, 0.09 KiB of operand fragments per MFMA against 0.125 -- was measured in
    // round 5: 756 against 673 us per 4096-site step; 768 workgroups of 72 KB rings fill the GPU in 1.5 rounds)
    case LT_F1: hipLaunchKernelGGL(lstm_cell_kernel<1>, grid, dim3(256), 0, s, L); break;
    case LT_F4: hipLaunchKernelGGL(lstm_cell_kernel<4>, grid, dim3(256), 0, s, L); break;
    case LT_S11: case LT_S12: case LT_S22: case LT_S28: case LT_COUNT: return hipErrorInvalidValue;      // launch_lstm_cells_split's
    }
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------
// Fused inception module. One workgroup (8 waves) owns a tile of whole sites (<= 96 rows):
//   P1  [rows x cin] x [cin x 240]: the six 1x1 convs that read the module input in ONE pass over
//       it (branch 1 reads the 3-tap max-pooled rows, staged next to the plain rows). Wave w < 6 owns
//       32-wide n-tile w for all m-tiles; waves 6, 7 share branch 1's 48 channels by ROWS, on 16-wide
//       tiles. b2/b1 go straight to HBM, the three 32-channel intermediates go
//       to LDS (T1, with zero halo rows = SAME padding), the residual stem stays in accumulators.
//   P2a 1x3 64-ch conv of branch 5 (T1 -> T2 in LDS) + part of branch 3.
//   P2b branch 5's last 1x1 accumulates ON TOP of the stem accumulators (waves 0,1) while the other
//       waves finish the 1x3 / 1x5 convs of branches 3 and 4.
// The 48-channel outputs (b1, b3b, b4b) are 32 + 16: channels 32..47 run on v_mfma_f32_16x16x4_f32 (the same FLOP per
// clock as 32x32x2), so only the residual tail still pays for padded columns. Issued MFMA time per 96-row tile and module
// (cin = 240), in units of 64 cycles: 3756 (P1 2700 + P2 1056), of which 3708 are real channels; 32-wide tiles alone took 4128.
// HBM traffic per module = read input once + write output once (module-granular bytes).
#ifndef DS_FUSED_WPS
#define DS_FUSED_WPS 2
#endif
// Register stages of the fused module's P1 operand prefetch (weight fragments / input rows): 2 = one chunk ahead. Deeper
// rings were measured (3, 4 stages each): the same P1 time -- the operands are not late -- and more registers. The
// register count matters beyond spills: at 183 VGPRs two module waves leave room for one BiLSTM cell wave (136) on the
// same SIMD, and a cell workgroup's 48 KB of LDS fits next to the module's 105 - 111 KB, so cell workgroups run in the
// shadow of module workgroups (512-site bench 527 k -> 540 k sites/s; 532 k at 188, 529 k at 196 VGPRs).
#ifndef DS_FUSED_BD
#define DS_FUSED_BD 2
#endif
// (s_setprio 2 for the fp32 pooling waves, as in the bf16 kernel, was measured: 625 against 586 us per step; the BiLSTM cell
// waves' own priority is DS_CELL_PRIO, defined in front of lstm_cell_lds_kernel)
#ifndef DS_FUSED_POOLPRIO
#define DS_FUSED_POOLPRIO 0
#endif
#ifndef DS_FUSED_VD
#define DS_FUSED_VD 2
#endif
constexpr int F_LDA = KC + 4;   // staged chunk row stride (floats)
constexpr int F_LD1 = 100;      // T1 row stride: 96 channels + 4 pad (25 x 16 B: odd -> conflict-free b128)
constexpr int F_LD2 = 68;       // T2 row stride: 64 channels + 4 pad

size_t inception_fused_lds_bytes(int tm, int W, int spt)
{
    const int tr32 = tm * 32;
    // region A (chunk staging, later the b1|b2 output tile) | T1 | T2 | rowmap
    return (size_t)(tr32 * F_LD1 + (spt * (W + 4) + 5) * F_LD1 + tr32 * F_LD2 + tr32 + 192) * sizeof(float);
}

// All weights of a conv unit (ntaps x 4 k-groups, <= 20 float4): requested EARLY — before the barrier or
// the epilogue in front of the unit — so their L2 latency is off the unit's critical path.
// (NFRAG fragments: ntaps x 4 of a unit on 32-wide tiles, ntaps x 2 of a 16-channel remainder unit)
// (Bp is wave-uniform: fragment g is the scalar base + g KiB, and the lane adds lane16 = 16 lane as a 32-bit offset -- no 64-bit
// vector address. DS_LANE_OFFSET: see inception_fused_body)
#define DS_LANE_OFFSET(v) asm volatile("" : "+v"(v))
// a wave-uniform address the same way: the sum stays one SGPR pair (scalar adds), in reach of the load's immediate
template <typename P> __device__ __forceinline__ P sbase(P p)
{
    asm volatile("" : "+s"(p));
    return p;
}
template <int NFRAG>
__device__ __forceinline__ void fused_unit_prefetch(const float* __restrict__ Bp, unsigned& lane16, float4 (&ub)[20])
{
    DS_LANE_OFFSET(lane16);
    const float* b4 = Bp;                   // 4 KiB of fragments per scalar base
#pragma unroll
    for (int g = 0; g < NFRAG; ++g) {
        if (g % 4 == 0) b4 = sbase(Bp + g * 256);
        ub[g] = gload4_at(b4 + (g % 4) * 256, lane16);
    }
}

template <int NTAPS>
__device__ __forceinline__ void fused_conv_unit(const float* T1, int rm, int coloff, int lane, const float4 (&ub)[20], floatx16& acc)
{
    const float* base = T1 + rm + coloff + (lane >> 5) * 4;        // rm: the row's offset in T1, in floats (the row map holds it so)
#pragma unroll
    for (int t = 0; t < NTAPS; ++t) {
        const float* arow = base + (t - NTAPS / 2) * F_LD1;
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const float4 a = *reinterpret_cast<const float4*>(arow + g * 8);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(ub[t * 4 + g].x, a.x, acc, 0, 0, 0);     // transposed: see the kernel
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(ub[t * 4 + g].y, a.y, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(ub[t * 4 + g].z, a.z, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(ub[t * 4 + g].w, a.w, acc, 0, 0, 0);
        }
    }
}

// Output channels 32..47 of a 48-channel conv (b3b, b4b) for one 32-row m-tile: two 16-row x 16-channel tiles on
// v_mfma_f32_16x16x4_f32 -- the same FLOP per clock as the 32x32x2 form, and 48 = 32 + 16 leaves no padded columns. Transposed
// like every MFMA here: lane (r = lane & 15, q = lane >> 4) reads channels 16g + 4q .. + 3 of activation row r with one
// ds_read_b128 and feeds element e to the e-th of four MFMAs, whose weight fragment element e holds k = 16g + 4q + e
// (ds_engine.cpp pack_b_rem16); it ends up with output channels 32 + 4q .. + 3 of its row. rm0 / rm1: T1 rows of the lane's row
// (as offsets in floats, as the row map holds them) in the upper / lower tile. The two tiles' MFMAs alternate, so no MFMA waits for the one before it.
template <int NTAPS>
__device__ __forceinline__ void fused_conv_unit16(const float* T1, int rm0, int rm1, int coloff, int lane, const float4 (&ub)[20], v4f& acc0, v4f& acc1)
{
    const float* base0 = T1 + rm0 + coloff + (lane >> 4) * 4;
    const float* base1 = T1 + rm1 + coloff + (lane >> 4) * 4;
#pragma unroll
    for (int t = 0; t < NTAPS; ++t) {
#pragma unroll
        for (int g = 0; g < 2; ++g) {
            const float4 a0 = *reinterpret_cast<const float4*>(base0 + (t - NTAPS / 2) * F_LD1 + g * 16);
            const float4 a1 = *reinterpret_cast<const float4*>(base1 + (t - NTAPS / 2) * F_LD1 + g * 16);
            const float4 w = ub[t * 2 + g];
            acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(w.x, a0.x, acc0, 0, 0, 0);
            acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(w.x, a1.x, acc1, 0, 0, 0);
            acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(w.y, a0.y, acc0, 0, 0, 0);
            acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(w.y, a1.y, acc1, 0, 0, 0);
            acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(w.z, a0.z, acc0, 0, 0, 0);
            acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(w.z, a1.z, acc1, 0, 0, 0);
            acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(w.w, a0.w, acc0, 0, 0, 0);
            acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(w.w, a1.w, acc1, 0, 0, 0);
        }
    }
}

__device__ __forceinline__ float f4elem(const float4& v, int e) { return e == 0 ? v.x : e == 1 ? v.y : e == 2 ? v.z : v.w; }

struct FusedTagT { static constexpr bool value = true; };
struct FusedTagF { static constexpr bool value = false; };
struct FusedTaps3 { static constexpr int value = 3; };
struct FusedTaps5 { static constexpr int value = 5; };

template <int TM>
__device__ __forceinline__ void inception_fused_body(const FusedChain& c)
{
    constexpr int TR32 = TM * 32;
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* Ad = smem;                         // [2][TR32*F_LDA] staged input rows
    float* Ys = smem;                         // [TR32][F_LD1] b1|b2 output tile, aliases Ad once P1 is done
    float* T1 = smem + TR32 * F_LD1;          // [spt*(W+4)][F_LD1]   (TR32*F_LD1 >= 4*TR32*F_LDA)
    const int W = c.m[0].W, spt = c.m[0].spt;          // the same for every module of a chain (ds_internal.h FusedChain)
    float* T2 = T1 + (spt * (W + 4) + 5) * F_LD1;   // [TR32*F_LD2]  (T1 has 5 spare rows: a dump row for padding rows + its halo)
    int* rowmap = reinterpret_cast<int*>(T2 + TR32 * F_LD2);   // [TR32] tile row -> offset of its T1 row, in floats (no multiply per use)
    float* const Bs = reinterpret_cast<float*>(rowmap + TR32); // [3][64] biases of b5b | b3b | b4b
    const int site0 = blockIdx.x * spt;
    const int nhere = min(spt, c.m[0].n_sites - site0);
    const int TRv = nhere * W;                // valid rows of this tile
    const size_t grow0 = (size_t)site0 * W;
    // once per workgroup: zero halo rows of T1 (every module rewrites the interior rows completely and never touches the
    // halos) and the tile's row map
    for (int i = threadIdx.x; i < (spt * (W + 4) + 5) * (F_LD1 / 4); i += 512)
        reinterpret_cast<float4*>(T1)[i] = make_float4(0.f, 0.f, 0.f, 0.f);
    if (threadIdx.x < TR32)   // rows past the tile's last site map to the dump row, so LDS writes need no predicate
        rowmap[threadIdx.x] = ((int)threadIdx.x < TRv ? ((int)threadIdx.x / W) * (W + 4) + 2 + (int)threadIdx.x % W : spt * (W + 4) + 2) * F_LD1;

    // ---- the modules of the chain, one after the other on THIS tile (one module per launch in the diagnostic modes): module
    // k + 1 reads the rows module k has just written -- same workgroup, so they come back from this XCD's L2 and no launch
    // boundary (with its drain and its cold start) sits between the modules
    for (int mi = 0; mi < c.nmod; ++mi) {
    const FusedArgs& a = c.m[mi];
    // every per-lane quantity derives from this opaque copy of the thread index: hipcc otherwise hoists loop-invariant
    // per-lane addresses out of the module loop, and the kernel must stay within 184 VGPRs (co-tenancy)
    int tid_opaque = threadIdx.x, wave_opaque = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    asm volatile("" : "+v"(tid_opaque), "+s"(wave_opaque));
    const int tid = tid_opaque, lane = tid & 63, wave = wave_opaque;
    const int cin = a.cin;
    const gptr1w Yg = (gptr1w)(a.Y + grow0 * 240);     // wave-uniform base; per-lane offsets stay 32-bit

    // diagnostic phase stamps (wave 0 and wave 7, lane 0): only when a debug buffer is attached
    const bool stamp = a.dbg != nullptr && lane == 0 && (wave == 0 || wave == 7) && blockIdx.x < DBG_MAX_WGS;
    // (the destination is recomputed at every stamp: a pointer held in VGPRs for the whole kernel costs two registers)
#define DS_STAMP(i) do { if (stamp) (a.dbg + ((size_t)blockIdx.x * 2 + (wave == 7)) * 8)[i] = __builtin_amdgcn_s_memtime(); } while (0)
    DS_STAMP(0);
    if (tid >= 256 && tid < 448) {
        const int q = tid - 256;
        Bs[q] = gload_at(q < 64 ? a.bias5b : q < 128 ? a.bias3b : a.bias4b, (unsigned)(q & 63) * 4u);
    }

    // ---- P1 staging cursor: thread -> (row, 16-byte slot); rows past the tile end re-read row TRv-1
    const bool stager = tid < TR32 * 4;
    const int sr = tid >> 2, sq = tid & 3;
    const int rr = sr < TRv ? sr : TRv - 1;
    // plain input: one row per staged row. Pooled input (modules right after maxpool_layer2/3): the staged
    // row (site s, w) is the max of input rows 2w - pad + {0,1,2} of site s that exist (padded taps ignored).
    // Every global address of P1 is (wave-uniform base: the tile's first input row / the wave's weight panel, in SGPRs) +
    // (32-bit byte offset of the lane, the same for all chunks) + (the chunk, a literal of the unrolled loop): a vector
    // instruction does not run in the shadow of an fp32 MFMA, so a per-lane 64-bit pointer bumped in every chunk is matrix time.
    // (a tile's rows span < 2 MB: 8 sites x pool_win rows x 1 KB)
    // DS_LANE_OFFSET(v) in front of a group of loads is an empty asm statement that "rewrites" the offset in place: no
    // instruction, but hipcc can then no longer widen the offset to a 64-bit pair once per module, add the base to it there and
    // carry that pair (two registers, and v_add_co / v_addc per chunk for whatever the 13-bit immediate does not reach).
    const bool pooled_in = a.pool_win > 0;
    const float* const xs = a.X + (pooled_in ? (size_t)site0 * a.pool_win : grow0) * cin;
    unsigned oc, oq = 0, orr = 0;
    if (!pooled_in) {
        oc = (unsigned)(rr * cin + sq * 4) * 4u;
    } else {
        const int s_ = rr / W, w_ = rr % W;
        const int i0 = 2 * w_ - a.pool_pad;
        const int ia = i0 < 0 ? i0 + 1 : i0;                               // first existing tap
        const int ib = i0 + 1 < a.pool_win ? (i0 + 1 < 0 ? ia : i0 + 1) : ia;
        const int ic = i0 + 2 < a.pool_win ? i0 + 2 : ib;
        const int sb = s_ * a.pool_win;
        oc = (unsigned)((sb + ia) * cin + sq * 4) * 4u;
        oq = (unsigned)((sb + ib) * cin + sq * 4) * 4u;
        orr = (unsigned)((sb + ic) * cin + sq * 4) * 4u;
    }
    // waves 0..5: n-tile `wave` of the 32-wide panel (K padded to 32 in the pack); waves 6, 7: b1's three 16-wide column tiles
    const float* const bs = wave < 6 ? a.Bp1 + (size_t)wave * ((cin + 31) / 32 * 4) * 256 : a.Bp1r;
    unsigned lane16 = (unsigned)lane * 16u;

    // Every MFMA of this kernel is issued TRANSPOSED -- mfma(weight fragment, activation fragment) computes (X W)^T --
    // so a lane ends up holding, for ONE activation row (lane & 31), 4 x 4 consecutive output channels
    // (register 4g+e <-> channel 32*ntile + 8g + 4*(lane >> 5) + e). Results leave as float4 groups (LDS and HBM)
    // instead of scalars, and the bias is simply the accumulator's initial value.
    // Waves 6, 7 (branch 1, 48 channels) instead split the tile's ROWS between them and run 16x16x4 MFMAs, so that no matrix
    // cycle goes to the 16 padded columns of an eighth 32-wide n-tile: wave 6 + i owns rows i * TM * 16 .. + TM * 16 - 1 as TM row
    // tiles x 3 column tiles. Its lane (r = lane & 15, q = lane >> 4) holds, for row tile mt and column tile g, channels
    // 16g + 4q .. + 3 of row 16 mt + r in acc[mt][4g .. 4g + 3] -- again one float4 per (mt, g), so the epilogue is shared.
    const int h4 = 4 * (lane >> 5), rlane = lane & 31;
    const int q4 = 4 * (lane >> 4), r15 = lane & 15, rbase16 = (wave - 6) * (TM * 16);
    floatx16 acc[TM];
    {
        float4 bv[4];
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            bv[g] = gload4_at(a.bias1, (unsigned)(wave < 6 ? wave * 32 + 8 * g + h4 : 192 + 16 * g + q4) * 4u);   // bias1 is zero-padded to 256
            if (wave < 2) {                                                     // b5 stem columns also carry the tail's BN shift
                const float4 t = gload4_at(a.bias5c, (unsigned)(wave * 32 + 8 * g + h4) * 4u);     // (zero-padded to 64)
                bv[g].x += t.x; bv[g].y += t.y; bv[g].z += t.z; bv[g].w += t.w;
            }
        }
#pragma unroll
        for (int mt = 0; mt < TM; ++mt)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                acc[mt][4 * g + 0] = bv[g].x; acc[mt][4 * g + 1] = bv[g].y;
                acc[mt][4 * g + 2] = bv[g].z; acc[mt][4 * g + 3] = bv[g].w;
            }
    }

    // branch 1's maxpool(3, stride 1, SAME): waves 6,7 build their A fragments as the max of three staged
    // rows (previous / own / next; at a site edge the missing neighbour is the own row = "padded taps
    // ignored"), so the input is read from HBM once and staged once.
    int offm[TM], offp[TM];
#pragma unroll
    for (int mt = 0; mt < TM; ++mt) {
        const int row = rbase16 + mt * 16 + r15;      // (only waves 6, 7 use these)
        const int w = row % W;
        offm[mt] = (row < TRv && w > 0) ? -F_LDA : 0;
        offp[mt] = (row < TRv && w < W - 1) ? F_LDA : 0;
    }

    const int nchunks = cin / KC;      // >= 15

    // P1 main loop: one barrier per 16-channel chunk; fragments of chunk c+1 are read into registers behind the second
    // half of chunk c's MFMAs; input rows and weight fragments are requested DS_FUSED_VD - 1 / DS_FUSED_BD - 1 chunks
    // ahead. Fully unrolled over the 15 or 16 chunks, so every register-ring and LDS-buffer index is a literal (183
    // instead of 247 VGPRs: see DS_FUSED_BD above).
    __builtin_assume(nchunks >= 15 && nchunks <= 16);
    auto run_p1 = [&](auto pool_tag) {
        constexpr bool POOL = decltype(pool_tag)::value;
        constexpr int VD = DS_FUSED_VD;
        float4 vc[VD];
        constexpr int BD = DS_FUSED_BD;                  // register stages of the weight fragments (chunk c's are requested BD - 1 steps ahead)
        float4 bq[BD][POOL ? 3 : 2];                     // pooling waves: one fragment per 16-wide column tile
        float4 af[2][POOL ? 1 : 2][TM];                  // pooling waves: one 16-row x 16-k fragment per row tile
        // (the pooling waves 6, 7 hold threads 384 .. 511 and a tile has at most 96 x 4 = 384 staging slots: they never stage,
        // and their variant carries neither the staging registers nor the row pointers)
        auto load_a = [&](int V, int ch) __attribute__((always_inline)) {      // chunk ch into stage V
            if (!POOL && stager) {
                DS_LANE_OFFSET(oc);
                vc[V] = gload4_at(xs + ch * KC, oc);
                if (pooled_in) {       // wave-uniform per launch
                    DS_LANE_OFFSET(oq); DS_LANE_OFFSET(orr);
                    vc[V] = f4max_relu(f4max_relu(vc[V], gload4_at(xs + ch * KC, oq)), gload4_at(xs + ch * KC, orr));
                }
            }
        };
        auto store_a = [&](int X, int V) __attribute__((always_inline)) {
            if (!POOL && stager) *reinterpret_cast<float4*>(Ad + X * TR32 * F_LDA + sr * F_LDA + sq * 4) = vc[V];
        };
        auto load_b = [&](int Bi, int ch) __attribute__((always_inline)) {     // chunk ch's fragments into stage Bi
            DS_LANE_OFFSET(lane16);
            if (POOL) {
#pragma unroll
                for (int ct = 0; ct < 3; ++ct) bq[Bi][ct] = gload4_at(sbase(bs + ct * cin * 16 + ch * 256), lane16);      // a column tile's image is cin / 16 KiB
            } else {
                const float* const b = sbase(bs + ch * 512);
                bq[Bi][0] = gload4_at(b, lane16);
                bq[Bi][1] = gload4_at(b + 256, lane16);
            }
        };
        auto read_frags = [&](int X) __attribute__((always_inline)) {
            if (POOL) {
#pragma unroll
                for (int mt = 0; mt < TM; ++mt) {
                    const float* q = Ad + X * TR32 * F_LDA + (rbase16 + mt * 16 + r15) * F_LDA + q4;
                    af[X][0][mt] = f4max_relu(f4max_relu(*reinterpret_cast<const float4*>(q), *reinterpret_cast<const float4*>(q + offm[mt])),
                                              *reinterpret_cast<const float4*>(q + offp[mt]));
                }
                return;
            }
#pragma unroll
            for (int rs = 0; rs < 2; ++rs)
#pragma unroll
                for (int mt = 0; mt < TM; ++mt) {
                    const float* q = Ad + X * TR32 * F_LDA + (mt * 32 + (lane & 31)) * F_LDA + rs * 8 + (lane >> 5) * 4;
                    af[X][rs][mt] = *reinterpret_cast<const float4*>(q);
                }
        };
        auto mfma_rs = [&](int X, int Bi, int rs) __attribute__((always_inline)) {
            if (POOL) {
                // half rs of a chunk = elements 2 rs, 2 rs + 1 of every fragment (k = 4q + e); the 3 TM accumulators take turns,
                // so no MFMA waits for the one before it
#pragma unroll
                for (int e = 2 * rs; e < 2 * rs + 2; ++e)
#pragma unroll
                    for (int mt = 0; mt < TM; ++mt)
#pragma unroll
                        for (int ct = 0; ct < 3; ++ct) {
                            v4f t = {acc[mt][4 * ct], acc[mt][4 * ct + 1], acc[mt][4 * ct + 2], acc[mt][4 * ct + 3]};
                            t = __builtin_amdgcn_mfma_f32_16x16x4f32(f4elem(bq[Bi][ct], e), f4elem(af[X][0][mt], e), t, 0, 0, 0);
                            acc[mt][4 * ct] = t[0]; acc[mt][4 * ct + 1] = t[1]; acc[mt][4 * ct + 2] = t[2]; acc[mt][4 * ct + 3] = t[3];
                        }
                return;
            }
#pragma unroll
            for (int mt = 0; mt < TM; ++mt) {
                acc[mt] = __builtin_amdgcn_mfma_f32_32x32x2f32(bq[Bi][rs].x, af[X][rs][mt].x, acc[mt], 0, 0, 0);
                acc[mt] = __builtin_amdgcn_mfma_f32_32x32x2f32(bq[Bi][rs].y, af[X][rs][mt].y, acc[mt], 0, 0, 0);
                acc[mt] = __builtin_amdgcn_mfma_f32_32x32x2f32(bq[Bi][rs].z, af[X][rs][mt].z, acc[mt], 0, 0, 0);
                acc[mt] = __builtin_amdgcn_mfma_f32_32x32x2f32(bq[Bi][rs].w, af[X][rs][mt].w, acc[mt], 0, 0, 0);
            }
        };
#pragma unroll
        for (int i = 0; i < VD; ++i) load_a(i, i);               // chunks 0 .. VD - 1 (nchunks >= 15)
#pragma unroll
        for (int i = 0; i < BD - 1; ++i) load_b(i, i);           // weight fragments of chunks 0 .. BD - 2
        store_a(0, 0);
        __syncthreads();
        read_frags(0);
#pragma unroll
        for (int c = 0; c < 16; ++c) {
            if (c < nchunks) {                                    // wave-uniform; only c = 15 is really conditional
                const int X = c & 1;
                const bool has1 = c + 1 < nchunks;
                if (c + VD < nchunks) load_a(c % VD, c + VD);     // chunk c + VD into the stage chunk c left (written at step c - 1)
                if (c + BD - 1 < nchunks) load_b((c + BD - 1) % BD, c + BD - 1);
                if (has1) store_a(X ^ 1, (c + 1) % VD);
                mfma_rs(X, c % BD, 0);
                __builtin_amdgcn_sched_barrier(0);
                __syncthreads();
                if (has1) read_frags(X ^ 1);
                mfma_rs(X, c % BD, 1);
                __builtin_amdgcn_sched_group_barrier(0x8, 1, 0);
                if (has1) __builtin_amdgcn_sched_group_barrier(0x100, (POOL ? 3 : 2) * TM, 0);
                __builtin_amdgcn_sched_group_barrier(0x8, (POOL ? 6 : 4) * TM, 0);
                __builtin_amdgcn_sched_barrier(0);
            }
        }
    };
    // the two pooling waves carry three LDS reads + eight v_max per fragment where the others carry one read: every chunk's
    // barrier waits for them, so they get the SIMD's issue priority while P1 runs (DS_FUSED_POOLPRIO, measured)
    if (wave >= 6) { __builtin_amdgcn_s_setprio(DS_FUSED_POOLPRIO); run_p1(FusedTagT{}); __builtin_amdgcn_s_setprio(0); }
    else run_p1(FusedTagF{});     // wave-uniform
    DS_STAMP(1);
    __syncthreads();   // all fragment reads of the staging area are done before T2 aliases it
    DS_STAMP(2);

    // ---- static wave -> unit assignment of P2 (wave-uniform). Units, in 64-cycle MFMA units: b5b (1x3, 32 -> 64; 48 per
    // m-tile and n-tile), b3b / b4b channels 0..31 on 32x32x2 tiles (48 / 80 per m-tile), b3b / b4b channels 32..47 on 16x16x4
    // tiles (24 / 40), the tail (TM x 32 on waves 0, 1, in P2b). b5b must run in P2a; the others are free. Every wave walks
    // the same sequence of SITES, each with one tile shape and one tap count, and runs or skips each of them:
    //   P2a  A1 1x3 on 32-wide tiles (kind 1 = b5b, 2 = b3b) | A2 b3b remainder
    //   P2b  B1 1x5 (kind 3 = b4b on 32-wide tiles, 5 = its remainder) | B2 b3b on 32-wide tiles | B3 b3b remainder
    // (a site whose weights differ in number from wave to wave costs registers: see pf below). Waves w and w+4 share a SIMD.
    // Three m-tiles, per SIMD: P2a 96 96 120 96, P2b 160 160 160 168 -- 1056 in all, where 32-wide tiles alone took 1248.
    int a1k = 0, a1m = 0, a1n = 0, a2m = -1;                        // P2a
    int b1k = 0, b1m = 0, b2m = -1, b3m = -1;                       // P2b (waves 0, 1 run the residual tail)
    if (TM == 3) {
        if (wave < 6) { a1k = 1; a1m = wave % 3; a1n = wave / 3; }
        else { a1k = 2; a1m = wave - 6; }
        if (wave == 6) a2m = 0;
        if (wave == 2 || wave == 3) { b1k = 3; b1m = wave - 2; }
        else if (wave == 6) { b1k = 3; b1m = 2; }
        else if (wave == 4 || wave == 5) { b1k = 5; b1m = wave - 4; b3m = wave - 3; }
        else if (wave == 7) { b1k = 5; b1m = 2; b2m = 2; }
    } else if (TM == 2) {
        if (wave < 4) { a1k = 1; a1m = wave & 1; a1n = wave >> 1; }
        else if (wave < 6) { a1k = 2; a1m = wave & 1; }
        else a2m = wave & 1;
        if (wave >= 2 && wave < 6) { b1k = wave < 4 ? 3 : 5; b1m = wave & 1; }
    } else {
        if (wave < 2) { a1k = 1; a1n = wave; }
        else if (wave == 2) a1k = 2;
        else if (wave == 3) a2m = 0;
        else if (wave < 6) b1k = wave == 4 ? 3 : 5;
    }
    float4 pf[20];                                   // prefetched weights of the next unit
    // (defined on every path: a register array that is only loaded under a wave-uniform condition is "undefined on some
    // paths", and hipcc keeps such a value live around the whole module loop -- 80 + 32 VGPRs of phantom live range here)
#pragma unroll
    for (int g = 0; g < 20; ++g) pf[g] = make_float4(0.f, 0.f, 0.f, 0.f);
    if (a1k) fused_unit_prefetch<12>(a1k == 1 ? a.Bp5b + a1n * (12 * 256) : a.Bp3b, lane16, pf);

    // ---- P1 epilogue (bias already inside acc): route the 256 columns. b1|b2 go through an LDS tile and leave as
    // whole 384-B row segments.
    if (wave >= 3 && wave <= 5) {            // wave-uniform: n-tiles 3,4,5 = b3a | b4a | b5a -> T1, through the row map
#pragma unroll
        for (int mt = 0; mt < TM; ++mt) {
            const int rm = rowmap[mt * 32 + rlane];
#pragma unroll
            for (int g = 0; g < 4; ++g)
                *reinterpret_cast<float4*>(T1 + rm + (wave * 32 - 96) + 8 * g + h4) =
                    make_float4(relu_f(acc[mt][4 * g]), relu_f(acc[mt][4 * g + 1]), relu_f(acc[mt][4 * g + 2]),
                                relu_f(acc[mt][4 * g + 3]));
        }
    } else if (wave != 0) {                  // n-tiles 1,2 (b5s tail | b2) and b1 (waves 6, 7: rows split, 16-wide tiles) -> output tile
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            // waves 1, 2: columns 32 .. 95 of the panel, of which 48 .. 95 are b2 = Y[:, 48:96) (groups of 4 never straddle 48);
            // waves 6, 7: b1 = Y[:, 0:48), column tile g (there is no fourth)
            const int ycol = wave < 6 ? wave * 32 + 8 * g + h4 : 16 * g + q4;
            if (wave < 6 ? ycol >= 48 : g < 3) {
#pragma unroll
                for (int mt = 0; mt < TM; ++mt)
                    *reinterpret_cast<float4*>(Ys + (wave < 6 ? mt * 32 + rlane : rbase16 + mt * 16 + r15) * F_LD1 + ycol) =
                        make_float4(relu_f(acc[mt][4 * g]), relu_f(acc[mt][4 * g + 1]), relu_f(acc[mt][4 * g + 2]),
                                    relu_f(acc[mt][4 * g + 3]));
            }
        }
    }
    DS_STAMP(3);
    __syncthreads();   // T1 and the b1|b2 tile complete
    DS_STAMP(4);
    for (int idx = tid; idx < TR32 * 24; idx += 512) {
        const int row = idx / 24, q = idx - row * 24;
        if (row < TRv) {
            const float4 v = *reinterpret_cast<const float4*>(Ys + row * F_LD1 + q * 4);
            v4f o = {v.x, v.y, v.z, v.w};
            gstore4_at(Yg, (unsigned)(row * 240 + q * 4) * 4u, o);
        }
    }

    // 1x3 on a 32-row x 32-channel tile. kind 1: b5b, 32 -> 64, ReLU, to T2 (n-tile nt)     layers.py:127-131
    //                                    kind 2: b3b, 32 -> 48, ReLU, channels 0..31 to Y[96,128)   layers.py:106-110
    auto unit_full3 = [&](int kind, int mt, int nt) {
        floatx16 u;
        const float* bsrc = Bs + (kind == 1 ? nt * 32 : 64) + h4;
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const float4 t = *reinterpret_cast<const float4*>(bsrc + 8 * g);
            u[4 * g] = t.x; u[4 * g + 1] = t.y; u[4 * g + 2] = t.z; u[4 * g + 3] = t.w;
        }
        const int row = mt * 32 + rlane;
        fused_conv_unit<3>(T1, rowmap[row], kind == 1 ? 64 : 0, lane, pf, u);
        if (kind == 1) {
#pragma unroll
            for (int g = 0; g < 4; ++g)
                *reinterpret_cast<float4*>(T2 + (mt * 32 * F_LD2 + nt * 32) + (rlane * F_LD2 + h4) + 8 * g) =      // scalar part | lane part
                    make_float4(relu_f(u[4 * g]), relu_f(u[4 * g + 1]), relu_f(u[4 * g + 2]), relu_f(u[4 * g + 3]));
        } else if (row < TRv) {
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                v4f o = {relu_f(u[4 * g]), relu_f(u[4 * g + 1]), relu_f(u[4 * g + 2]), relu_f(u[4 * g + 3])};
                gstore4_at(Yg + 96 + 8 * g, (unsigned)(row * 240 + h4) * 4u, o);      // the literal rides in the store's immediate
            }
        }
    };
    // b4b: 1x5, 32 -> 48, ReLU, channels 0..31 to Y[144,176)                                  layers.py:115-119
    auto unit_full5 = [&](int mt) {
        floatx16 u;
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const float4 t = *reinterpret_cast<const float4*>(Bs + 128 + h4 + 8 * g);
            u[4 * g] = t.x; u[4 * g + 1] = t.y; u[4 * g + 2] = t.z; u[4 * g + 3] = t.w;
        }
        const int row = mt * 32 + rlane;
        fused_conv_unit<5>(T1, rowmap[row], 32, lane, pf, u);
        if (row < TRv) {
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                v4f o = {relu_f(u[4 * g]), relu_f(u[4 * g + 1]), relu_f(u[4 * g + 2]), relu_f(u[4 * g + 3])};
                gstore4_at(Yg + 144 + 8 * g, (unsigned)(row * 240 + h4) * 4u, o);
            }
        }
    };
    // channels 32..47 of b3b (NTAPS 3, to Y[128,144)) or b4b (NTAPS 5, to Y[176,192)) on 16-wide tiles
    auto unit_rem = [&](auto ntaps_tag, int mt) {
        constexpr int NTAPS = decltype(ntaps_tag)::value;
        const int q4 = 4 * (lane >> 4), row0 = mt * 32 + (lane & 15), row1 = row0 + 16;
        const float4 t = *reinterpret_cast<const float4*>(Bs + (NTAPS == 3 ? 64 : 128) + 32 + q4);
        v4f u0 = {t.x, t.y, t.z, t.w}, u1 = u0;
        fused_conv_unit16<NTAPS>(T1, rowmap[row0], rowmap[row1], NTAPS == 3 ? 0 : 32, lane, pf, u0, u1);
        constexpr int ycol = (NTAPS == 3 ? 96 : 144) + 32;
        if (row0 < TRv) {
            v4f o = {relu_f(u0[0]), relu_f(u0[1]), relu_f(u0[2]), relu_f(u0[3])};
            gstore4_at(Yg + ycol, (unsigned)(row0 * 240 + q4) * 4u, o);
        }
        if (row1 < TRv) {
            v4f o = {relu_f(u1[0]), relu_f(u1[1]), relu_f(u1[2]), relu_f(u1[3])};
            gstore4_at(Yg + ycol, (unsigned)(row1 * 240 + q4) * 4u, o);
        }
    };

    // Waves 0, 1 keep the stem accumulators through P2a for the tail; the other waves' accumulators are dead after the P1
    // epilogue. The two groups take separate (wave-uniform) paths, each with its own copy of the T2 barrier, so that the
    // registers of acc are free where the 1x5 units run (80 registers of weights).
    if (wave >= 2) {
        // ---- P2a
        if (a1k) unit_full3(a1k, a1m, a1n);
        if (a2m >= 0) {
            fused_unit_prefetch<6>(a.Bp3r, lane16, pf);
            unit_rem(FusedTaps3{}, a2m);
        }
        // ---- P2b behind the T2 barrier (the same barrier as waves 0, 1's). The weights of a wave's 1x5 unit are requested before
        // it. Request, barrier and unit sit in ONE branch per kind: were the request under one condition and the unit under
        // another, hipcc would keep the previous unit's weights alive across the barrier for the paths it cannot rule out.
        if (b1k == 3) {
            fused_unit_prefetch<20>(a.Bp4b, lane16, pf);
            DS_STAMP(5); __syncthreads(); DS_STAMP(6);
            unit_full5(b1m);
        } else if (b1k == 5) {
            fused_unit_prefetch<10>(a.Bp4r, lane16, pf);
            DS_STAMP(5); __syncthreads(); DS_STAMP(6);
            unit_rem(FusedTaps5{}, b1m);
        } else {
            DS_STAMP(5); __syncthreads(); DS_STAMP(6);
        }
        if (b2m >= 0) {
            fused_unit_prefetch<12>(a.Bp3b, lane16, pf);
            unit_full3(2, b2m, 0);
        }
        if (b3m >= 0) {
            fused_unit_prefetch<6>(a.Bp3r, lane16, pf);
            unit_rem(FusedTaps3{}, b3m);
        }
    } else {
        // ---- P2a: one b5b unit (every table above gives waves 0, 1 kind 1 and nothing else)
        unit_full3(1, a1m, a1n);
        // weights of the tail are requested before the barrier
        float4 b5c[8];
        DS_LANE_OFFSET(lane16);
#pragma unroll
        for (int g = 0; g < 8; ++g) b5c[g] = gload4_at(sbase(a.Bp5c + (size_t)(wave * 8 + g / 4 * 4) * 256) + (g % 4) * 256, lane16);
        DS_STAMP(5);
        __syncthreads();   // T2 complete
        DS_STAMP(6);
        // ---- P2b
        // branch 5 tail: 1x1 64 -> 48 (BN, no ReLU) accumulated on top of the stem conv held in acc,
        // then relu(stem + tail)                                                         layers.py:132-138
#pragma unroll
        for (int mt = 0; mt < TM; ++mt) {
            const float* base = T2 + (mt * 32 + rlane) * F_LD2 + h4;
#pragma unroll
            for (int g = 0; g < 8; ++g) {
                const float4 av = *reinterpret_cast<const float4*>(base + g * 8);
                acc[mt] = __builtin_amdgcn_mfma_f32_32x32x2f32(b5c[g].x, av.x, acc[mt], 0, 0, 0);
                acc[mt] = __builtin_amdgcn_mfma_f32_32x32x2f32(b5c[g].y, av.y, acc[mt], 0, 0, 0);
                acc[mt] = __builtin_amdgcn_mfma_f32_32x32x2f32(b5c[g].z, av.z, acc[mt], 0, 0, 0);
                acc[mt] = __builtin_amdgcn_mfma_f32_32x32x2f32(b5c[g].w, av.w, acc[mt], 0, 0, 0);
            }
        }
        const gptr1w Yt = sbase(Yg + 192 + wave * 32);
#pragma unroll
        for (int mt = 0; mt < TM; ++mt) {
            const int row = mt * 32 + rlane;
            if (row < TRv) {
                unsigned yo = (unsigned)(row * 240 + h4) * 4u;
#pragma unroll
                for (int g = 0; g < 4; ++g)
                    if (wave * 32 + 8 * g < 48) {
                        DS_LANE_OFFSET(yo);
                        v4f o = {relu_f(acc[mt][4 * g]), relu_f(acc[mt][4 * g + 1]), relu_f(acc[mt][4 * g + 2]),
                                 relu_f(acc[mt][4 * g + 3])};
                        gstore4_at(Yt + 8 * g, yo, o);
                    }
            }
        }
    }
    DS_STAMP(7);
#undef DS_STAMP
    // the next module reads the rows this one has stored (other waves' stores included) and re-uses every LDS region
    if (mi + 1 < c.nmod) __syncthreads();
    }   // modules of the chain
}

template <int TM>
__global__ __launch_bounds__(512, DS_FUSED_WPS) void inception_fused_kernel(const FusedChain c) { inception_fused_body<TM>(c); }
// one tiling for the whole chain; only its first module may pool its input (ds_internal.h FusedChain)
static bool fused_chain_ok(const FusedChain& c)
{
    if (c.nmod <= 0 || c.nmod > FUSED_CHAIN_MAX) return false;
    for (int i = 1; i < c.nmod; ++i)
        if (c.m[i].W != c.m[0].W || c.m[i].spt != c.m[0].spt || c.m[i].n_sites != c.m[0].n_sites || c.m[i].pool_win != 0 ||
            c.m[i].X != c.m[i - 1].Y) return false;
    return true;
}

hipError_t launch_inception_fused(int tm, const FusedChain& c, hipStream_t s)
{
    if (!fused_chain_ok(c)) return hipErrorInvalidValue;
    const FusedArgs& a = c.m[0];
    if (a.n_sites <= 0) return hipSuccess;
    for (int i = 0; i < c.nmod; ++i)
        if (c.m[i].cin != 240 && c.m[i].cin != 256) return hipErrorInvalidValue;      // P1 is unrolled over 15 or 16 chunks (every module of the model)
    const size_t lds = inception_fused_lds_bytes(tm, a.W, a.spt);
    const int grid = (a.n_sites + a.spt - 1) / a.spt;
    switch (tm) {
    case 1: hipLaunchKernelGGL(inception_fused_kernel<1>, dim3(grid), dim3(512), lds, s, c); break;
    case 2: hipLaunchKernelGGL(inception_fused_kernel<2>, dim3(grid), dim3(512), lds, s, c); break;
    case 3: hipLaunchKernelGGL(inception_fused_kernel<3>, dim3(grid), dim3(512), lds, s, c); break;
    default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------
// Fused inception modules, bf16 operands (DS_PRECISION_BF16*). Same phases and wave roles as
// inception_fused_kernel; what changes is the data: activations are bf16 rows of 256-channel pitch (channels
// 240..255 are zero in global memory), a K chunk is 16 four-byte units = 32 channels = two v_mfma_f32_32x32x16_bf16 steps,
// the 32-channel intermediates live in LDS as bf16 (T1 row = 104 elements: an odd number of 16-B slots, conflict-free
// ds_read_b128), accumulation / bias / ReLU / residual are fp32 and every value is rounded to bf16 (nearest even) exactly
// once, when it is stored.
//
// Roofline: HBM (module-granular bytes: 512 B in + 480 B out per module row). A 96-row tile is ~2 us of matrix-pipe time, so
// what matters is the memory traffic and how much of it a CU keeps in flight. Round 3 form:
//   * TWO workgroups per CU (<= 128 VGPRs, <= 76 KB of LDS each): one tile's load / store phases run under the other's MFMAs;
//   * the 3-tap max-pooled copy of the input tile (branch 1's operand, 50 KB) is gone: waves 6, 7 pool their fragments
//     on the fly (three ds_read_b128 + v_pk_max_u16 per fragment), as the fp32 kernel does;
//   * the P1 weights stream through a ring of two fragments per wave instead of sixteen resident ones;
//   * a launch carries the modules of one width class and the tile's rows STAY IN LDS from module to module: every result is
//     written in place over the (dead) input rows in the layout the next module's P1 reads. Only the chain's first module
//     loads rows and only its last one stores them (whole 480-byte rows): eight of the eleven module outputs never reach
//     HBM. Bisect builds had priced the parts of the 755 us the global-memory chain took at 4096 sites: re-loading the rows
//     55 us, issuing their stores 30 us, the write traffic itself 65 us; this form takes 620 us.
#ifndef DS_FUSEDB_WPS
#define DS_FUSEDB_WPS 4
#endif
#ifndef DS_FUSEDB_POOLPRIO
#define DS_FUSEDB_POOLPRIO 2
#endif
#ifndef DS_FUSEDB_RING
#define DS_FUSEDB_RING 2      // register stages of a wave's P1 weight fragments (2, 3: same time on MI355X; 3 and 4 spill at 128 VGPRs)
#endif
constexpr int B_LDA = 132;      // staged input row stride in units (256 channels + 8 pad: 33 x 16 B, odd)
constexpr int B_LD1 = 52;       // T1 row stride in units (96 channels + 8 pad)

size_t inception_fused_bf16_lds_bytes(int tm, int W, int spt)
{
    const int tr32 = tm * 32;
    return (size_t)(tr32 * B_LDA + (spt * (W + 4) + 5) * B_LD1 + tr32 + 192) * sizeof(float);    // the tile's rows (input, then output in place; T2 in their last 64 channels) | T1 | rowmap | 3x64 biases
}

// weights of one conv unit: ntaps x 2 k-steps (<= 10 fragments); the packed panel of an n-tile holds KS k-steps
__device__ __forceinline__ void fusedb_unit_prefetch(const float* __restrict__ Bp, int ntaps, int nt, int lane, float4 (&ub)[10])
{
    const int ks = (ntaps * 32 + 63) / 64 * 4;      // K padded to 64 elements by pack_b_bf16
    const float* bsrc = Bp + ((size_t)(nt * ks) * 64 + lane) * 4;
#pragma unroll
    for (int g = 0; g < 10; ++g)
        if (g < ntaps * 2) ub[g] = gload4(bsrc + g * 256);
}

template <int NTAPS>
__device__ __forceinline__ void fusedb_conv_unit(const float* T1, int rm, int coloff_units, int lane, const float4 (&ub)[10], floatx16& acc)
{
    const float* base = T1 + rm * B_LD1 + coloff_units + (lane >> 5) * 4;
#pragma unroll
    for (int t = 0; t < NTAPS; ++t) {
        const float* arow = base + (t - NTAPS / 2) * B_LD1;
#pragma unroll
        for (int j = 0; j < 2; ++j)
            acc = mfma_bf(ub[t * 2 + j], *reinterpret_cast<const float4*>(arow + j * 8), acc);     // transposed: see the kernel
    }
}

// the same unit on NM m-tiles at once (one set of weights, NM independent accumulator chains: a single unit is a chain of
// dependent MFMAs behind dependent LDS reads, i.e. latency)
template <int NTAPS, int NM>
__device__ __forceinline__ void fusedb_conv_units(const float* T1, const int (&rm)[NM], int coloff_units, int lane, const float4 (&ub)[10], floatx16 (&acc)[NM])
{
#pragma unroll
    for (int t = 0; t < NTAPS; ++t)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int m = 0; m < NM; ++m)
                acc[m] = mfma_bf(ub[t * 2 + j], *reinterpret_cast<const float4*>(T1 + (rm[m] + t - NTAPS / 2) * B_LD1 + coloff_units + (lane >> 5) * 4 + j * 8), acc[m]);
}

template <int TM>
__global__ __launch_bounds__(512, TM >= 2 ? DS_FUSEDB_WPS : 2) void inception_fused_bf16_kernel(const FusedChain c)
{
    constexpr int TR32 = TM * 32;
    extern __shared__ __attribute__((aligned(16))) float smem[];
    // [TR32][B_LDA] the tile's rows, 256 channels each. A module's INPUT during its P1; behind P1 the same rows receive the
    // module's OUTPUT in place (b1 | b2 | b3 | b4 | b5 = channels [0, 240)), which is the next module's input: inside a chain
    // the rows never leave the CU. Channels [192, 256) of a row hold branch 5's 64-channel intermediate (T2) between P2a and
    // the tail; what T2 leaves in the pad channels [240, 256) is finite and meets zero weight rows in the next module's P1.
    float* const As = smem;
    float* const T1 = smem + TR32 * B_LDA;          // [spt*(W+4)+5][B_LD1] b3a | b4a | b5a with zero halo rows
    const int tid = threadIdx.x, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int W = c.m[0].W, spt = c.m[0].spt, cinu = c.m[0].cin;          // cin in units (128); the same for every module of a chain
    int* const rowmap = reinterpret_cast<int*>(T1 + (spt * (W + 4) + 5) * B_LD1);
    float* const Bs = reinterpret_cast<float*>(rowmap + TR32);                    // [3][64] biases of b5b | b3b | b4b
    unsigned short* const T1h = reinterpret_cast<unsigned short*>(T1);
    unsigned short* const Ash = reinterpret_cast<unsigned short*>(As);
    // workgroup barrier for LDS traffic only: __syncthreads() also drains vmcnt, i.e. waits for prefetched weights and for the
    // row stores that are meant to leave in the background
    auto lds_barrier = []() __attribute__((always_inline)) { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); };
    constexpr int NSLOT = TR32 * 32 / 512;    // 16-B slots of the input tile per thread: 2 * TM

    const int site0 = blockIdx.x * spt;
    const int TRv = min(spt, c.m[0].n_sites - site0) * W;          // valid rows of this tile
    typedef __attribute__((address_space(1))) unsigned short* gbf16w;

    // relu + round four consecutive channels to bf16 -> one 8-byte group
    auto pack4 = [](float x0, float x1, float x2, float x3) -> uint2 {
        return make_uint2(pack_bf2(relu_f(x0), relu_f(x1)), pack_bf2(relu_f(x2), relu_f(x3)));
    };

    // static wave -> unit assignment of P2 (wave-uniform). kind: 0 none, 1 b5b, 2 b3b, 3 b4b; with three m-tiles waves 6, 7 run
    // branch 3's n-tile on all of them in phase a (one set of weights)
    int ak = 0, am = 0, an = 0;
    int bk = 0, bm = 0, bn = 0;
    if (TM == 3) {
        if (wave < 6) { ak = 1; am = wave % 3; an = wave / 3; }
        else { ak = 2; am = 0; an = wave - 6; }
        if (wave >= 2) { bk = 3; bm = (wave - 2) % 3; bn = (wave - 2) / 3; }
    } else if (TM == 2) {
        if (wave < 4) { ak = 1; am = wave & 1; an = wave >> 1; }
        else { ak = 2; am = wave & 1; an = (wave - 4) >> 1; }
        if (wave >= 2 && wave < 6) { bk = 3; bm = (wave - 2) & 1; bn = (wave - 2) >> 1; }
    } else {
        if (wave < 2) { ak = 1; an = wave; }
        else if (wave < 4) { ak = 2; an = wave - 2; }
        else if (wave < 6) { ak = 3; an = wave - 4; }
    }

    // once per workgroup: the tile's row map and the zero halo rows of T1 (every module of the chain rewrites T1's interior
    // rows completely and never touches the halos)
    for (int i = tid; i < (spt * (W + 4) + 5) * (B_LD1 / 4); i += 512)
        reinterpret_cast<float4*>(T1)[i] = make_float4(0.f, 0.f, 0.f, 0.f);
    if (tid < TR32)
        rowmap[tid] = tid < TRv ? (tid / W) * (W + 4) + 2 + tid % W : spt * (W + 4) + 2;

    // ---- the modules of the chain, one after the other on THIS tile. Only the first module reads rows from global memory
    // and only the last one writes rows back: in between a module's output rows are the next module's input, in LDS.
    for (int mi = 0; mi < c.nmod; ++mi) {
    const FusedArgs& a = c.m[mi];
    // Every per-lane quantity of the body derives from this opaque copy of the thread index: hipcc otherwise hoists ~100
    // loop-invariant per-lane addresses out of the module loop and spills them (the kernel lives on 128 VGPRs).
    int tid_opaque = threadIdx.x, wave_opaque = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    asm volatile("" : "+v"(tid_opaque), "+s"(wave_opaque));
    const int tid = tid_opaque, lane = tid & 63, h4 = 4 * (lane >> 5), rlane = lane & 31, wave = wave_opaque;
    const bool stamp = a.dbg != nullptr && lane == 0 && (wave == 0 || wave == 7) && blockIdx.x < DBG_MAX_WGS;
    // (the destination is recomputed at every stamp: a pointer held in VGPRs for the whole kernel costs two of the 128)
#define DS_STAMP(i) do { if (stamp) (a.dbg + ((size_t)blockIdx.x * 2 + (wave == 7)) * 8)[i] = __builtin_amdgcn_s_memtime(); } while (0)
    DS_STAMP(0);
    auto unit_Bp = [&](int k) { return k == 1 ? a.Bp5b : k == 2 ? a.Bp3b : a.Bp4b; };
    auto unit_taps = [&](int k) { return k == 3 ? 5 : 3; };

    // the small global requests of a module's prologue, all issued before anything waits: the unit biases, this wave's P1 bias
    // (+ the tail's BN shift on the b5 stem columns)
    float bsv;
    float4 bv[4], tv[4];
    auto request_biases = [&]() __attribute__((always_inline)) {
        bsv = tid < 192 ? gload((tid < 64 ? a.bias5b : tid < 128 ? a.bias3b : a.bias4b) + (tid & 63)) : 0.0f;
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            bv[g] = gload4(a.bias1 + wave * 32 + 8 * g + h4);                               // bias1 is zero-padded to 256
            tv[g] = gload4(a.bias5c + (wave < 2 ? wave : 0) * 32 + 8 * g + h4);             // zero-padded to 64; used by waves 0, 1 only
        }
    };
    if (mi == 0) {
        // ---- chain head: the WHOLE input tile is requested at once (a bf16 K chunk is ~200 matrix-pipe cycles: nothing
        // hides behind it; the other workgroup of the CU computes meanwhile)
        const bool pooled_in = a.pool_win > 0;
        float4 st[NSLOT];
        const size_t grow0 = (size_t)site0 * W;
        if (!pooled_in) {
#pragma unroll
            for (int i = 0; i < NSLOT; ++i) {
                const int id = tid + i * 512, row = id >> 5, q = id & 31;
                const int rr = row < TRv ? row : TRv - 1;
                // read exactly once: a non-temporal load does not keep the input rows in the XCD's L2, which then holds the rows the
                // workgroups have just WRITTEN (the next module of the chain reads those)
                st[i] = gload4_nt(a.X + (grow0 + rr) * cinu + q * 4);
            }
        } else {
            // module right after maxpool_layer2/3: staged row (site s, w) = max of the input rows 2w - pad + {0,1,2} that exist
#pragma unroll
            for (int i = 0; i < NSLOT; ++i) {
                const int id = tid + i * 512, row = id >> 5, q = id & 31;
                const int rr = row < TRv ? row : TRv - 1;
                const int s_ = rr / W, w_ = rr % W;
                const int i0 = 2 * w_ - a.pool_pad;
                const int ia = i0 < 0 ? i0 + 1 : i0;
                const int ib = i0 + 1 < a.pool_win ? (i0 + 1 < 0 ? ia : i0 + 1) : ia;
                const int ic = i0 + 2 < a.pool_win ? i0 + 2 : ib;
                const float* sb = a.X + ((size_t)(site0 + s_) * a.pool_win) * cinu + q * 4;
                st[i] = bf8max_relu(bf8max_relu(gload4(sb + (size_t)ia * cinu), gload4(sb + (size_t)ib * cinu)), gload4(sb + (size_t)ic * cinu));
            }
        }
        request_biases();
#pragma unroll
        for (int i = 0; i < NSLOT; ++i) {
            const int id = tid + i * 512, row = id >> 5, q = id & 31;
            *reinterpret_cast<float4*>(As + row * B_LDA + q * 4) = st[i];
        }
    } else {
        request_biases();
    }
    if (tid < 192) Bs[tid] = bsv;        // read behind the barriers of P1; the previous module's last use is behind its barriers
    // P1 weights of this wave's n-tile (16 fragments, L2-resident) through a ring of DS_FUSEDB_RING
    // (wave-uniform base + one 32-bit lane offset: scalar address arithmetic, no 64-bit per-lane pointers in the loop)
    const char* const bp_base = reinterpret_cast<const char*>(a.Bp1) + (size_t)wave * ((cinu + 31) / 32 * 4) * 1024;
    const unsigned lane16 = (unsigned)lane * 16;
    auto bfrag = [&](int g) __attribute__((always_inline)) { return gload4(reinterpret_cast<const float*>(bp_base + g * 1024 + lane16)); };
    float4 bw[DS_FUSEDB_RING];
#pragma unroll
    for (int g = 0; g < DS_FUSEDB_RING; ++g) bw[g] = bfrag(g);
    // Every MFMA of this kernel is issued TRANSPOSED: mfma(weight fragment, activation fragment) gives (X W)^T, so
    // a lane ends up holding, for ONE activation row (lane & 31), 4 x 4 consecutive output channels
    // (register 4g+e <-> channel 32*ntile + 8g + 4*(lane >> 5) + e). Results leave as packed 8-byte groups of four
    // bf16 instead of 2-byte scalars, and the bias is simply the accumulator's initial value.
    floatx16 acc[TM];
    {
        const float tsel = wave < 2 ? 1.0f : 0.0f;      // b5 stem columns also carry the tail's BN shift (exact: x + 1 * t)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const float4 b = make_float4(fmaf(tsel, tv[g].x, bv[g].x), fmaf(tsel, tv[g].y, bv[g].y), fmaf(tsel, tv[g].z, bv[g].z),
                                         fmaf(tsel, tv[g].w, bv[g].w));
#pragma unroll
            for (int mt = 0; mt < TM; ++mt) {
                acc[mt][4 * g + 0] = b.x; acc[mt][4 * g + 1] = b.y;
                acc[mt][4 * g + 2] = b.z; acc[mt][4 * g + 3] = b.w;
            }
        }
    }
    if (mi == 0) lds_barrier();   // input tile, zeroed T1, rowmap in place (later modules: behind the previous module's last barrier)
    DS_STAMP(1);

    // ---- P1: [rows x 256] x [256 x 256], 16 k-steps back to back out of LDS. Waves 6, 7
    // (branch 1) take the 3-tap max of their fragment and its two neighbour rows -- maxpool(3, stride 1, SAME), a missing
    // neighbour at a site edge = the own row ("padded taps ignored")        layers.py:90-91
    auto run_p1 = [&](auto pool_tag) __attribute__((always_inline)) {
        constexpr bool POOL = decltype(pool_tag)::value;
        const float* const src = As + rlane * B_LDA + h4;
        if (!POOL) {
            // ONE fragment buffer: the reads of k-step g + 1 are issued right behind the MFMAs of k-step g (which have
            // taken their operands by then) and land while those run -- the look-ahead of a double buffer without its registers
            float4 af[TM];
#pragma unroll
            for (int mt = 0; mt < TM; ++mt) af[mt] = *reinterpret_cast<const float4*>(src + mt * 32 * B_LDA);
#pragma unroll
            for (int g = 0; g < 16; ++g) {
#pragma unroll
                for (int mt = 0; mt < TM; ++mt) acc[mt] = mfma_bf(bw[g % DS_FUSEDB_RING], af[mt], acc[mt]);
                if (g + DS_FUSEDB_RING < 16) bw[g % DS_FUSEDB_RING] = bfrag(g + DS_FUSEDB_RING);
                if (g + 1 < 16) {
#pragma unroll
                    for (int mt = 0; mt < TM; ++mt) af[mt] = *reinterpret_cast<const float4*>(src + mt * 32 * B_LDA + (g + 1) * 8);
                }
                __builtin_amdgcn_sched_barrier(0);
            }
        } else {
            // pooled operand: raw[mt] = (own, previous, next) row fragments of k-step g, requested one k-step ahead; per
            // m-tile: 3-tap max (8 x v_pk_max_u16) -> MFMA -> request the next k-step's three fragments into the registers
            // just consumed. The max of m-tile mt + 1 issues under the MFMA of m-tile mt.
            int om[TM], op[TM];
#pragma unroll
            for (int mt = 0; mt < TM; ++mt) {
                const int row = mt * 32 + rlane, w = row % W;
                om[mt] = (row < TRv && w > 0) ? -B_LDA : 0;
                op[mt] = (row < TRv && w < W - 1) ? B_LDA : 0;
            }
            float4 raw[TM][3];
#pragma unroll
            for (int mt = 0; mt < TM; ++mt) {
                const float* q = src + mt * 32 * B_LDA;
                raw[mt][0] = *reinterpret_cast<const float4*>(q);
                raw[mt][1] = *reinterpret_cast<const float4*>(q + om[mt]);
                raw[mt][2] = *reinterpret_cast<const float4*>(q + op[mt]);
            }
#pragma unroll
            for (int g = 0; g < 16; ++g) {
#pragma unroll
                for (int mt = 0; mt < TM; ++mt) {
                    const float4 af = bf8max_relu(bf8max_relu(raw[mt][0], raw[mt][1]), raw[mt][2]);
                    if (g + 1 < 16) {
                        const float* q = src + mt * 32 * B_LDA + (g + 1) * 8;
                        raw[mt][0] = *reinterpret_cast<const float4*>(q);
                        raw[mt][1] = *reinterpret_cast<const float4*>(q + om[mt]);
                        raw[mt][2] = *reinterpret_cast<const float4*>(q + op[mt]);
                    }
                    acc[mt] = mfma_bf(bw[g % DS_FUSEDB_RING], af, acc[mt]);
                }
                if (g + DS_FUSEDB_RING < 16) bw[g % DS_FUSEDB_RING] = bfrag(g + DS_FUSEDB_RING);
                __builtin_amdgcn_sched_barrier(0);
            }
        }
    };
    // the two pooling waves carry ~2x the instructions of the others per k-step and everybody waits for them at the barrier
    // below: they get the SIMD's issue priority while they are in P1
    if (wave >= 6) { __builtin_amdgcn_s_setprio(DS_FUSEDB_POOLPRIO); run_p1(FusedTagT{}); __builtin_amdgcn_s_setprio(0); }
    else run_p1(FusedTagF{});     // wave-uniform
    DS_STAMP(2);
    lds_barrier();   // all fragment reads of the input rows are done: the output may overwrite them
    float4 pf[10];
    // (fragments 6..9 are only loaded for the five-tap unit; defined here so that their live range starts here and not, as an
    // "undefined on some paths" value, in front of the module loop -- sixteen registers held across P1 otherwise)
#pragma unroll
    for (int g = 6; g < 10; ++g) pf[g] = make_float4(0.f, 0.f, 0.f, 0.f);
    if (ak) fusedb_unit_prefetch(unit_Bp(ak), unit_taps(ak), an, lane, pf);

    // ---- P1 epilogue (bias already inside acc)
    if (wave >= 3 && wave <= 5) {            // b3a | b4a | b5a -> T1 (bf16), through the row map (SAME-padding halos)
#pragma unroll
        for (int mt = 0; mt < TM; ++mt) {
            const int rm = rowmap[mt * 32 + rlane];
#pragma unroll
            for (int g = 0; g < 4; ++g)
                *reinterpret_cast<uint2*>(T1h + rm * (2 * B_LD1) + (wave * 32 - 96) + 8 * g + h4) =
                    pack4(acc[mt][4 * g], acc[mt][4 * g + 1], acc[mt][4 * g + 2], acc[mt][4 * g + 3]);
        }
    } else if (wave != 0) {                  // b2 -> channels [48, 96), b1 -> channels [0, 48) of the tile's rows (b5 stem | padding stay behind)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const int col = wave * 32 + 8 * g + h4;          // groups of 4 never straddle 48 / 240
            if (col >= 48 && col < 240) {
                const int ycol = col < 96 ? col : col - 192;
#pragma unroll
                for (int mt = 0; mt < TM; ++mt)
                    *reinterpret_cast<uint2*>(Ash + (mt * 32 + rlane) * (2 * B_LDA) + ycol) =
                        pack4(acc[mt][4 * g], acc[mt][4 * g + 1], acc[mt][4 * g + 2], acc[mt][4 * g + 3]);
            }
        }
    }
    lds_barrier();   // T1 complete
    DS_STAMP(3);

    // unit (kind, m-tile, n-tile) of the second-stage convs: 1 = 1x3 32 -> 64 of branch 5 (-> T2 = channels [192, 256) of the
    // rows, layers.py:127-131), 2 = 1x3 32 -> 48 of branch 3 (channels [96, 144), layers.py:106-110), 3 = 1x5 32 -> 48 of
    // branch 4 (channels [144, 192), layers.py:115-119)
    auto run_unit = [&](int kind, int mt, int nt) __attribute__((always_inline)) {
        floatx16 u;
        const float* bsrc = Bs + (kind == 1 ? 0 : kind == 2 ? 64 : 128) + nt * 32 + h4;
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const float4 t = *reinterpret_cast<const float4*>(bsrc + 8 * g);
            u[4 * g] = t.x; u[4 * g + 1] = t.y; u[4 * g + 2] = t.z; u[4 * g + 3] = t.w;
        }
        const int row = mt * 32 + rlane;
        const int rm = rowmap[row];
        if (kind == 1) fusedb_conv_unit<3>(T1, rm, 32, lane, pf, u);          // b5a = channels 64..95 = units 32..47
        else if (kind == 2) fusedb_conv_unit<3>(T1, rm, 0, lane, pf, u);      // b3a = channels 0..31
        else fusedb_conv_unit<5>(T1, rm, 16, lane, pf, u);                    // b4a = channels 32..63
        const int cbase = kind == 1 ? 192 : kind == 2 ? 96 : 144;
        const int ncol = kind == 1 ? 64 : 48;                                 // wave-uniform: 48 output channels = n-tile 0 and half of n-tile 1
#pragma unroll
        for (int g = 0; g < 4; ++g)
            if (nt * 32 + 8 * g < ncol)
                *reinterpret_cast<uint2*>(Ash + row * (2 * B_LDA) + cbase + nt * 32 + 8 * g + h4) = pack4(u[4 * g], u[4 * g + 1], u[4 * g + 2], u[4 * g + 3]);
    };

    // ---- P2a: branch 5's 1x3 units -> T2, branch 3 (/ 4) units -> their output channels
    if (TM == 3 && wave >= 6) {
        // branch 3's n-tile on all three m-tiles (same weights): m-tiles 0, 1 interleaved, then m-tile 2 (one after the other
        // the three units took 4.4 k cycles against 2.4 k for the single unit of the other waves: a unit is a chain of
        // dependent LDS reads and MFMAs; three accumulators at once do not fit the 128 registers next to the stem's)
        {
            floatx16 u2[2];
            const float* bsrc = Bs + 64 + an * 32 + h4;
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const float4 t = *reinterpret_cast<const float4*>(bsrc + 8 * g);
#pragma unroll
                for (int mt = 0; mt < 2; ++mt) { u2[mt][4 * g] = t.x; u2[mt][4 * g + 1] = t.y; u2[mt][4 * g + 2] = t.z; u2[mt][4 * g + 3] = t.w; }
            }
            int rm[2];
#pragma unroll
            for (int mt = 0; mt < 2; ++mt) rm[mt] = rowmap[mt * 32 + rlane];
            fusedb_conv_units<3, 2>(T1, rm, 0, lane, pf, u2);
#pragma unroll
            for (int mt = 0; mt < 2; ++mt)
#pragma unroll
                for (int g = 0; g < 4; ++g)
                    if (an * 32 + 8 * g < 48)
                        *reinterpret_cast<uint2*>(Ash + (mt * 32 + rlane) * (2 * B_LDA) + 96 + an * 32 + 8 * g + h4) =
                            pack4(u2[mt][4 * g], u2[mt][4 * g + 1], u2[mt][4 * g + 2], u2[mt][4 * g + 3]);
        }
        run_unit(2, 2, an);
    } else if (ak) {
        run_unit(ak, am, an);
    }
    if (wave < 2) {       // the tail's four weight fragments travel in the (idle) unit-weight registers
#pragma unroll
        for (int g = 0; g < 4; ++g) pf[g] = gload4(a.Bp5c + ((size_t)(wave * 4 + g) * 64 + lane) * 4);
    } else if (bk) {
        fusedb_unit_prefetch(unit_Bp(bk), unit_taps(bk), bn, lane, pf);
    }
    DS_STAMP(4);
    lds_barrier();     // T2 complete
    DS_STAMP(5);

    // ---- P2b: branch 4's 1x5 units; waves 0, 1: branch 5's tail
    if (wave < 2) {
        // 1x1 64 -> 48 (BN, no ReLU) accumulated on top of the stem conv held in acc, then relu(stem + tail)   layers.py:132-138
#pragma unroll
        for (int mt = 0; mt < TM; ++mt) {
            const float* base = As + (mt * 32 + rlane) * B_LDA + 96 + h4;
#pragma unroll
            for (int g = 0; g < 4; ++g) acc[mt] = mfma_bf(pf[g], *reinterpret_cast<const float4*>(base + g * 8), acc[mt]);
        }
    } else if (bk) {
        run_unit(bk, bm, bn);
    }
    DS_STAMP(6);
    lds_barrier();     // every T2 fragment has been read: branch 5's output may take its place
    if (wave < 2) {
#pragma unroll
        for (int mt = 0; mt < TM; ++mt)
#pragma unroll
            for (int g = 0; g < 4; ++g)
                if (wave * 32 + 8 * g < 48)
                    *reinterpret_cast<uint2*>(Ash + (mt * 32 + rlane) * (2 * B_LDA) + 192 + wave * 32 + 8 * g + h4) =
                        pack4(acc[mt][4 * g], acc[mt][4 * g + 1], acc[mt][4 * g + 2], acc[mt][4 * g + 3]);
    }
    lds_barrier();     // the module's output rows are complete: the next module's input
    if (a.write_rows) {
        // ---- the chain's last module (every module when taps are on): rows out, 480 contiguous bytes each (30 x 16 B)
        const gbf16w Yg = (gbf16w)(reinterpret_cast<unsigned short*>(a.Y) + (size_t)__builtin_amdgcn_readfirstlane(site0) * W * 256);
        for (int idx = tid; idx < TR32 * 30; idx += 512) {
            const int row = idx / 30, q = idx - row * 30;
            if (row < TRv) {
                const float4 v = *reinterpret_cast<const float4*>(As + row * B_LDA + q * 4);
                v4f o = {v.x, v.y, v.z, v.w};
                *(__attribute__((address_space(1))) v4f*)(Yg + (unsigned)(row * 256 + q * 8)) = o;
            }
        }
    }
    DS_STAMP(7);
#undef DS_STAMP
    }   // modules of the chain
}

// ---------------------------------------------------------------------------------------------
// conv_layer2 (1x1, 64 -> 128) + conv_layer3 (1x3, 128 -> 256), BN folded, ReLU            layers.py:192-203
// One workgroup (8 waves) owns a tile of whole sites (<= 96 rows), two workgroups per CU (<= 128 VGPRs, ~76 KB of LDS),
// so one workgroup's staging / epilogue runs under the other's MFMAs.
//   stage  the 64-channel input rows (stem_pool) -> Xs
//   conv2  12 units of (32 rows x 32 channels, K = 64), three per SIMD -> T (ReLU) with one zero halo row on either
//          side of every site = conv3's SAME padding
//   conv3  wave w = output channels [32 w, 32 w + 32) of all three m-tiles. The WHOLE activation tile is in LDS, so the
//          48 k-groups (3 taps x 16) run without a barrier: weights global -> VGPR through a ring of four register
//          stages, activation fragments from T one k-group ahead. Every LDS / global offset is an immediate on a
//          loop-invariant base (fully unrolled): no vector ALU work between the MFMAs (tools/attic/mfma_valu.hip).
// MFMAs are issued transposed (weights, activations) as in the fused module: a lane holds 4 x 4 consecutive channels of
// one row, bias = accumulator init, float4 stores.
// Roofline: MFMA. Algorithmic FLOPs per site = 2 * W * (64 * 128 + 3 * 128 * 256); HBM bytes per row 256 in, 1024 out.
constexpr int S23_LDX = 68;     // Xs row stride (floats): 17 x 16 B, odd -> conflict-free b128 fragment reads
constexpr int S23_LDT = 132;    // T row stride: 33 x 16 B
size_t stem23_lds_bytes(int W, int spt)
{
    return (size_t)(96 * S23_LDX + (spt * (W + 2) + 3) * S23_LDT + 96) * sizeof(float);
}

__global__ __launch_bounds__(512, 2) void stem23_kernel(const Stem23Args a)
{
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* const Xs = smem;                                   // [96][S23_LDX]
    float* const T = smem + 96 * S23_LDX;                     // [spt * (W + 2) + 3][S23_LDT]
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int W = a.W, spt = a.spt;
    const int trows = spt * (W + 2) + 3;                      // last three rows: halo | dump row (padding rows of the tile) | halo
    int* const rowmap = reinterpret_cast<int*>(T + trows * S23_LDT);     // [96] tile row -> T row
    const int site0 = blockIdx.x * spt;
    const int nhere = min(spt, a.n_sites - site0);
    const int TRv = nhere * W;
    const size_t grow0 = (size_t)site0 * W;
    const int h4 = 4 * (lane >> 5), rlane = lane & 31;

    // ---- stage: zero T (halo rows must be zero; the rest is overwritten), row map, input rows
    for (int i = tid; i < trows * (S23_LDT / 4); i += 512) reinterpret_cast<float4*>(T)[i] = make_float4(0.f, 0.f, 0.f, 0.f);
    if (tid < 96) rowmap[tid] = tid < TRv ? (tid / W) * (W + 2) + 1 + tid % W : spt * (W + 2) + 1;
    {
        float4 v[3];
#pragma unroll
        for (int i = 0; i < 3; ++i) {                          // 96 rows x 16 float4
            const int idx = tid + 512 * i, row = idx >> 4, q = idx & 15;
            const int rr = row < TRv ? row : TRv - 1;
            v[i] = gload4(a.X + (grow0 + rr) * 64 + q * 4);
        }
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            const int idx = tid + 512 * i, row = idx >> 4, q = idx & 15;
            *reinterpret_cast<float4*>(Xs + row * S23_LDX + q * 4) = v[i];
        }
    }
    // conv3 weights of the first ring stages and both bias vectors are requested before the barrier
    const char* const b3 = reinterpret_cast<const char*>(a.Bp3) + (size_t)wave * 48 * 1024;
    const unsigned lane16 = (unsigned)lane * 16;
    float4 bq[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) bq[i] = gload4(reinterpret_cast<const float*>(b3 + i * 1024 + lane16));
    float4 bias3[4];
#pragma unroll
    for (int g = 0; g < 4; ++g) bias3[g] = gload4(a.bias3 + wave * 32 + 8 * g + h4);
    __syncthreads();

    // ---- conv2: unit u = (m, n); waves 0..3 take (0, w) and (2, w), waves 4..7 take (1, w - 4): three units per SIMD
    {
        const int n2 = wave & 3;
        float4 w2[8];
#pragma unroll
        for (int g = 0; g < 8; ++g) w2[g] = gload4(a.Bp2 + ((size_t)(n2 * 8 + g) * 64 + lane) * 4);
        float4 bias2[4];
#pragma unroll
        for (int g = 0; g < 4; ++g) bias2[g] = gload4(a.bias2 + n2 * 32 + 8 * g + h4);
        const int nunits = wave < 4 ? 2 : 1;
        for (int ui = 0; ui < nunits; ++ui) {
            const int m = wave < 4 ? 2 * ui : 1;
            floatx16 u;
#pragma unroll
            for (int g = 0; g < 4; ++g) { u[4 * g] = bias2[g].x; u[4 * g + 1] = bias2[g].y; u[4 * g + 2] = bias2[g].z; u[4 * g + 3] = bias2[g].w; }
            const float* xr = Xs + (m * 32 + rlane) * S23_LDX + h4;
#pragma unroll
            for (int g = 0; g < 8; ++g) {
                const float4 x = *reinterpret_cast<const float4*>(xr + g * 8);
                u = __builtin_amdgcn_mfma_f32_32x32x2f32(w2[g].x, x.x, u, 0, 0, 0);
                u = __builtin_amdgcn_mfma_f32_32x32x2f32(w2[g].y, x.y, u, 0, 0, 0);
                u = __builtin_amdgcn_mfma_f32_32x32x2f32(w2[g].z, x.z, u, 0, 0, 0);
                u = __builtin_amdgcn_mfma_f32_32x32x2f32(w2[g].w, x.w, u, 0, 0, 0);
            }
            const int row = m * 32 + rlane;
            float* const td = T + rowmap[row] * S23_LDT + n2 * 32 + h4;
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const float4 o = make_float4(relu_f(u[4 * g]), relu_f(u[4 * g + 1]), relu_f(u[4 * g + 2]), relu_f(u[4 * g + 3]));
                *reinterpret_cast<float4*>(td + 8 * g) = o;
                if (a.C2 && row < TRv) {                       // diagnostic tap (debug mode): conv_layer2's output rows
                    const v4f ov = {o.x, o.y, o.z, o.w};
                    *(__attribute__((address_space(1))) v4f*)(a.C2 + (grow0 + row) * 128 + n2 * 32 + 8 * g + h4) = ov;
                }
            }
        }
    }
    __syncthreads();

    // ---- conv3
    floatx16 acc[3];
#pragma unroll
    for (int m = 0; m < 3; ++m)
#pragma unroll
        for (int g = 0; g < 4; ++g) { acc[m][4 * g] = bias3[g].x; acc[m][4 * g + 1] = bias3[g].y; acc[m][4 * g + 2] = bias3[g].z; acc[m][4 * g + 3] = bias3[g].w; }
    const float* tb[3];
#pragma unroll
    for (int m = 0; m < 3; ++m) tb[m] = T + (rowmap[m * 32 + rlane] - 1) * S23_LDT + h4;     // tap t reads row + t - 1
    float4 af[2][3];
#pragma unroll
    for (int m = 0; m < 3; ++m) af[0][m] = *reinterpret_cast<const float4*>(tb[m]);
#pragma unroll
    for (int kgl = 0; kgl < 48; ++kgl) {
        const int cur = kgl & 1, slot = kgl & 3;
        if (kgl + 1 < 48) {
            const int t1 = (kgl + 1) >> 4, g1 = (kgl + 1) & 15;
#pragma unroll
            for (int m = 0; m < 3; ++m) af[cur ^ 1][m] = *reinterpret_cast<const float4*>(tb[m] + t1 * S23_LDT + g1 * 8);
        }
#pragma unroll
        for (int m = 0; m < 3; ++m) {
            acc[m] = __builtin_amdgcn_mfma_f32_32x32x2f32(bq[slot].x, af[cur][m].x, acc[m], 0, 0, 0);
            acc[m] = __builtin_amdgcn_mfma_f32_32x32x2f32(bq[slot].y, af[cur][m].y, acc[m], 0, 0, 0);
            acc[m] = __builtin_amdgcn_mfma_f32_32x32x2f32(bq[slot].z, af[cur][m].z, acc[m], 0, 0, 0);
            acc[m] = __builtin_amdgcn_mfma_f32_32x32x2f32(bq[slot].w, af[cur][m].w, acc[m], 0, 0, 0);
        }
        if (kgl + 4 < 48) bq[slot] = gload4(reinterpret_cast<const float*>(b3 + (kgl + 4) * 1024 + lane16));
        __builtin_amdgcn_sched_barrier(0);       // pins the ring: requests stay four k-groups ahead of their MFMAs
    }

    // ---- ReLU, rows out (each lane: 4 x 16 B of one row)
#pragma unroll
    for (int m = 0; m < 3; ++m) {
        const int row = m * 32 + rlane;
        if (row < TRv) {
            float* const yd = a.Y + (grow0 + row) * 256 + wave * 32 + h4;
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const v4f o = {relu_f(acc[m][4 * g]), relu_f(acc[m][4 * g + 1]), relu_f(acc[m][4 * g + 2]), relu_f(acc[m][4 * g + 3])};
                *(__attribute__((address_space(1))) v4f*)(yd + 8 * g) = o;
            }
        }
    }
}

hipError_t launch_stem23(const Stem23Args& a, hipStream_t s)
{
    if (a.n_sites <= 0) return hipSuccess;
    const int grid = (a.n_sites + a.spt - 1) / a.spt;
    hipLaunchKernelGGL(stem23_kernel, dim3(grid), dim3(512), stem23_lds_bytes(a.W, a.spt), s, a);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------
// conv_layer2 + conv_layer3 with bf16 operands (DS_PRECISION_BF16*): the bf16 form of stem23_kernel.   layers.py:192-203
// Rows are bf16 (64 channels in, 128 in LDS only, 256 out); v_mfma_f32_32x32x16_bf16, fp32 accumulate, bias = accumulator
// init, ReLU and one rounding to bf16 when a value is stored. Two workgroups per CU (<= 128 VGPRs, 52 KB of LDS); the
// 256-channel output rows leave through an LDS tile (over the dead input / conv2 tiles) as whole 512-byte rows.
// Roofline: HBM. Algorithmic bytes per row: 128 in + 512 out (the two-launch GEMM form also wrote and re-read 256 + 768).
constexpr int SB_LDX = 36;      // Xs row stride in 4-byte units: 64 channels + 8 pad (9 x 16 B, odd)
constexpr int SB_LDT = 68;      // T row stride: 128 channels + 8 pad (17 x 16 B)
constexpr int SB_LDO = 132;     // output tile row stride: 256 channels + 8 pad (33 x 16 B)
size_t stem23_bf16_lds_bytes(int W, int spt)
{
    const size_t work = (size_t)96 * SB_LDX + (size_t)(spt * (W + 2) + 3) * SB_LDT;
    const size_t outt = (size_t)96 * SB_LDO;
    return ((work > outt ? work : outt) + 96) * sizeof(float);
}

__global__ __launch_bounds__(512, 4) void stem23_bf16_kernel(const Stem23Args a)
{
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* const Xs = smem;                                   // [96][SB_LDX]
    float* const T = smem + 96 * SB_LDX;                      // [spt * (W + 2) + 3][SB_LDT]
    float* const Ot = smem;                                   // [96][SB_LDO] output tile, over Xs / T once conv3 has read them
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int W = a.W, spt = a.spt;
    const int trows = spt * (W + 2) + 3;
    const size_t work = (size_t)96 * SB_LDX + (size_t)trows * SB_LDT, outt = (size_t)96 * SB_LDO;
    int* const rowmap = reinterpret_cast<int*>(smem + (work > outt ? work : outt));     // [96] tile row -> T row
    const int site0 = blockIdx.x * spt;
    const int TRv = min(spt, a.n_sites - site0) * W;
    const size_t grow0 = (size_t)site0 * W;
    const int h4 = 4 * (lane >> 5), rlane = lane & 31;
    unsigned short* const Th = reinterpret_cast<unsigned short*>(T);
    unsigned short* const Oh = reinterpret_cast<unsigned short*>(Ot);
    auto pack4 = [](float x0, float x1, float x2, float x3) -> uint2 {
        return make_uint2(pack_bf2(relu_f(x0), relu_f(x1)), pack_bf2(relu_f(x2), relu_f(x3)));
    };

    // ---- stage: zero T (halo rows), row map, input rows (96 rows x 8 slots of 16 B: 768 slots)
    for (int i = tid; i < trows * (SB_LDT / 4); i += 512) reinterpret_cast<float4*>(T)[i] = make_float4(0.f, 0.f, 0.f, 0.f);
    if (tid < 96) rowmap[tid] = tid < TRv ? (tid / W) * (W + 2) + 1 + tid % W : spt * (W + 2) + 1;
    {
        float4 v[2];
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int idx = tid + 512 * i, row = idx >> 3, q = idx & 7;
            const int rr = row < TRv ? row : TRv - 1;
            if (idx < 768) v[i] = gload4(a.X + (grow0 + rr) * 32 + q * 4);      // 64 bf16 = 32 units per row
        }
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int idx = tid + 512 * i, row = idx >> 3, q = idx & 7;
            if (idx < 768) *reinterpret_cast<float4*>(Xs + row * SB_LDX + q * 4) = v[i];
        }
    }
    // conv3 weights of this wave's n-tile: 24 k-steps (3 taps x 8), ring of four; both bias vectors
    const char* const b3 = reinterpret_cast<const char*>(a.Bp3) + (size_t)wave * 24 * 1024;
    const unsigned lane16 = (unsigned)lane * 16;
    float4 bq[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) bq[i] = gload4(reinterpret_cast<const float*>(b3 + i * 1024 + lane16));
    float4 bias3[4];
#pragma unroll
    for (int g = 0; g < 4; ++g) bias3[g] = gload4(a.bias3 + wave * 32 + 8 * g + h4);
    __syncthreads();

    // ---- conv2: K = 64 (4 k-steps); unit (m, n): waves 0..3 take (0, w) and (2, w), waves 4..7 take (1, w - 4)
    {
        const int n2 = wave & 3;
        float4 w2[4];
#pragma unroll
        for (int g = 0; g < 4; ++g) w2[g] = gload4(a.Bp2 + ((size_t)(n2 * 4 + g) * 64 + lane) * 4);
        float4 bias2[4];
#pragma unroll
        for (int g = 0; g < 4; ++g) bias2[g] = gload4(a.bias2 + n2 * 32 + 8 * g + h4);
        const int nunits = wave < 4 ? 2 : 1;
        for (int ui = 0; ui < nunits; ++ui) {
            const int m = wave < 4 ? 2 * ui : 1;
            floatx16 u;
#pragma unroll
            for (int g = 0; g < 4; ++g) { u[4 * g] = bias2[g].x; u[4 * g + 1] = bias2[g].y; u[4 * g + 2] = bias2[g].z; u[4 * g + 3] = bias2[g].w; }
            const float* xr = Xs + (m * 32 + rlane) * SB_LDX + h4;
#pragma unroll
            for (int g = 0; g < 4; ++g) u = mfma_bf(w2[g], *reinterpret_cast<const float4*>(xr + g * 8), u);
            const int row = m * 32 + rlane;
            unsigned short* const td = Th + rowmap[row] * (2 * SB_LDT) + n2 * 32 + h4;
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const uint2 o = pack4(u[4 * g], u[4 * g + 1], u[4 * g + 2], u[4 * g + 3]);
                *reinterpret_cast<uint2*>(td + 8 * g) = o;
                if (a.C2 && row < TRv) {                       // diagnostic tap (debug mode): conv_layer2's output rows, bf16
                    typedef unsigned int u2v __attribute__((ext_vector_type(2)));
                    const u2v ov = {o.x, o.y};
                    *(__attribute__((address_space(1))) u2v*)(reinterpret_cast<unsigned short*>(a.C2) + (grow0 + row) * 128 + n2 * 32 + 8 * g + h4) = ov;
                }
            }
        }
    }
    __syncthreads();

    // ---- conv3: wave w = output channels [32 w, 32 w + 32) of all three m-tiles; 24 k-steps out of T without a barrier
    floatx16 acc[3];
#pragma unroll
    for (int m = 0; m < 3; ++m)
#pragma unroll
        for (int g = 0; g < 4; ++g) { acc[m][4 * g] = bias3[g].x; acc[m][4 * g + 1] = bias3[g].y; acc[m][4 * g + 2] = bias3[g].z; acc[m][4 * g + 3] = bias3[g].w; }
    const float* tb[3];
#pragma unroll
    for (int m = 0; m < 3; ++m) tb[m] = T + (rowmap[m * 32 + rlane] - 1) * SB_LDT + h4;     // tap t reads row + t - 1
    float4 af[3];
#pragma unroll
    for (int m = 0; m < 3; ++m) af[m] = *reinterpret_cast<const float4*>(tb[m]);
#pragma unroll
    for (int ks = 0; ks < 24; ++ks) {
        const int slot = ks & 3;
#pragma unroll
        for (int m = 0; m < 3; ++m) acc[m] = mfma_bf(bq[slot], af[m], acc[m]);
        if (ks + 4 < 24) bq[slot] = gload4(reinterpret_cast<const float*>(b3 + (ks + 4) * 1024 + lane16));
        if (ks + 1 < 24) {
            const int t1 = (ks + 1) >> 3, g1 = (ks + 1) & 7;
#pragma unroll
            for (int m = 0; m < 3; ++m) af[m] = *reinterpret_cast<const float4*>(tb[m] + t1 * SB_LDT + g1 * 8);
        }
        __builtin_amdgcn_sched_barrier(0);
    }
    __syncthreads();   // everybody has read T: the output tile may overwrite it

    // ---- ReLU, bf16, output tile, whole rows out
#pragma unroll
    for (int m = 0; m < 3; ++m)
#pragma unroll
        for (int g = 0; g < 4; ++g)
            *reinterpret_cast<uint2*>(Oh + (m * 32 + rlane) * (2 * SB_LDO) + wave * 32 + 8 * g + h4) =
                pack4(acc[m][4 * g], acc[m][4 * g + 1], acc[m][4 * g + 2], acc[m][4 * g + 3]);
    __syncthreads();
    __attribute__((address_space(1))) unsigned short* const Yg =
        (__attribute__((address_space(1))) unsigned short*)(reinterpret_cast<unsigned short*>(a.Y) + grow0 * 256);
    for (int idx = tid; idx < 96 * 32; idx += 512) {           // 256 channels = 32 x 16 B per row
        const int row = idx >> 5, q = idx & 31;
        if (row < TRv) {
            const float4 v = *reinterpret_cast<const float4*>(Ot + row * SB_LDO + q * 4);
            v4f o = {v.x, v.y, v.z, v.w};
            *(__attribute__((address_space(1))) v4f*)(Yg + (unsigned)(row * 256 + q * 8)) = o;
        }
    }
}

hipError_t launch_stem23_bf16(const Stem23Args& a, hipStream_t s)
{
    if (a.n_sites <= 0) return hipSuccess;
    const int grid = (a.n_sites + a.spt - 1) / a.spt;
    hipLaunchKernelGGL(stem23_bf16_kernel, dim3(grid), dim3(512), stem23_bf16_lds_bytes(a.W, a.spt), s, a);
    return hipGetLastError();
}

// The fused kernels need more than the default 64 KB of dynamic LDS: opt in once per device (ds_create calls this
// after hipSetDevice; function attributes are per device and must not be changed during stream capture).
hipError_t configure_fused_kernels()
{
    const void* fns[6] = {(const void*)inception_fused_kernel<1>, (const void*)inception_fused_kernel<2>,
                          (const void*)inception_fused_kernel<3>, (const void*)inception_fused_bf16_kernel<1>,
                          (const void*)inception_fused_bf16_kernel<2>, (const void*)inception_fused_bf16_kernel<3>};
    for (const void* f : fns) {
        const hipError_t e = hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
        if (e != hipSuccess) return e;
    }
    // the fp32 dense instantiation: static ring + the launch's pad (launch_gemm, CFG_FC_DENSE) pass the default 64 KB
    const hipError_t e1 = hipFuncSetAttribute((const void*)gemm_kernel<1, 3, 4, 1, 0, 2, 2, 1>, hipFuncAttributeMaxDynamicSharedMemorySize, DR_SOLO_PAD_BYTES);
    if (e1 != hipSuccess) return e1;
    const hipError_t e2 = hipFuncSetAttribute((const void*)stem23_bf16_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)STEM23_MAX_LDS);
    if (e2 != hipSuccess) return e2;
    return hipFuncSetAttribute((const void*)stem23_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)STEM23_MAX_LDS);
}

hipError_t launch_inception_fused_bf16(int tm, const FusedChain& c, hipStream_t s)
{
    if (!fused_chain_ok(c)) return hipErrorInvalidValue;
    const FusedArgs& a = c.m[0];
    if (a.n_sites <= 0) return hipSuccess;
    for (int i = 1; i < c.nmod; ++i)
        if (c.m[i].cin != a.cin) return hipErrorInvalidValue;
    const size_t lds = inception_fused_bf16_lds_bytes(tm, a.W, a.spt);
    const int grid = (a.n_sites + a.spt - 1) / a.spt;
    switch (tm) {
    case 1: hipLaunchKernelGGL(inception_fused_bf16_kernel<1>, dim3(grid), dim3(512), lds, s, c); break;
    case 2: hipLaunchKernelGGL(inception_fused_bf16_kernel<2>, dim3(grid), dim3(512), lds, s, c); break;
    case 3: hipLaunchKernelGGL(inception_fused_bf16_kernel<3>, dim3(grid), dim3(512), lds, s, c); break;
    default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------
// stem conv1: conv(K=7, stride 2, Cin=1 -> 64, SAME) + folded BN + ReLU + maxpool(3, stride 2, SAME)
// One block per site; the window sits in LDS with a zero halo (SAME padding, no bounds checks in the
// tap loop); lane = output channel, so the 64-float output rows are written as whole 256-B lines.
constexpr int STEM_HALO = 8;
// DS_SMALL_PRIO / DS_SMALL_PRIO_POST: issue priority (s_setprio) of the step's short non-matrix kernels, from entry to the end of
// the kernel. Like the BiLSTM cells (DS_CELL_PRIO) they are guests beside fused-module and dense waves that live hundreds of
// microseconds, are older, and win every oldest-first arbitration among equals, and each of them sits on a forward's critical chain.
// DS_SMALL_PRIO: the kernels inside the branches (stem1_kernel<false>, avgpool7_kernel, gather_inputs_kernel);
// DS_SMALL_PRIO_POST: the kernels behind the join (head_kernel, head_folded_kernel, scatter_outputs_kernel).
// Measured on the pipelined 512-site step against the parent, libraries alternating, four runs a side, k sites/s
// (profiles/small_kernels_ab.json; parent 459.9, its spread 0.14 %). On the parent's bodies: both at 1: 462.9 (+0.65 %), both at
// 2: 462.9, branches only: 462.2 (+0.50 %), behind the join only: 459.0 (-0.20 %). On the lean bodies below (no priority: 462.3,
// +0.51 %): both at 1 / both at 2: 465.2 / 465.1, branches only at 1 / at 2: 464.9 / 465.9. So the branch kernels ask, at the
// cells' level (2 is not above 1 by the project's bar), and the kernels behind the join do not: nothing is gained there, and
// alone it loses. Results are bit-identical (tests/test_gpu_small_kernel_bits.py).
#ifndef DS_SMALL_PRIO
#define DS_SMALL_PRIO 1
#endif
#ifndef DS_SMALL_PRIO_POST
#define DS_SMALL_PRIO_POST 0
#endif
// base + a 32-bit BYTE offset: with a wave-uniform base this is a scalar base and a 32-bit lane offset in the instruction (an element
// index would be widened to 64 bits before it is scaled, and the lane would carry the whole address)
template <typename T> __device__ __forceinline__ T* at_bytes(T* base, unsigned bytes)
{
    return (T*)((const char*)base + bytes);
}
constexpr int STEM1_WAVES = 4;
template <bool OUT_BF>
__global__ __launch_bounds__(256) void stem1_kernel(const float* __restrict__ signals, const float* __restrict__ w,
                                                     const float* __restrict__ bias, float* __restrict__ out,
                                                     int signal_len, int w1, int pad_l_conv, int wa, int pad_l_pool)
{
    extern __shared__ __attribute__((aligned(16))) float sig[];   // [STEM_HALO + signal_len + STEM_HALO + 8]
    if constexpr (!OUT_BF && DS_SMALL_PRIO != 0) __builtin_amdgcn_s_setprio(DS_SMALL_PRIO);
    const int total = signal_len + 2 * STEM_HALO + 8;
    const float* src = signals + (size_t)blockIdx.x * signal_len;          // scalar base, 32-bit lane offsets
    for (int i = threadIdx.x; i < total; i += blockDim.x) {
        const int k = i - STEM_HALO;
        sig[i] = (k >= 0 && k < signal_len) ? *at_bytes(src, 4u * (unsigned)k) : 0.0f;
    }
    __syncthreads();
    const int c = threadIdx.x & 63;
    float wk[7];
#pragma unroll
    for (int t = 0; t < 7; ++t) wk[t] = w[t * 64 + c];
    const float b = bias[c];
    // A wave walks consecutive pooled positions. Pooled position p takes the conv positions wc = 2p - pad_l_pool + {0,1,2}, each
    // reading sig[2*wc - pad_l_conv + 0..6]: the third of p is the first of p + 1, so it stays in a register (`carry`) with the
    // seven window samples behind it, and a step computes two conv positions from four new samples where it was three from eleven.
    // Every conv position is still the fma chain t = 0..6 from 0.f, and the maximum takes them in the same order.
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int chunk = (wa + STEM1_WAVES - 1) / STEM1_WAVES;
    const int p_lo = wave * chunk, p_hi = p_lo + chunk < wa ? p_lo + chunk : wa;
    if (p_lo < p_hi) {
        const float* s0 = sig + STEM_HALO + 2 * (2 * p_lo - pad_l_pool) - pad_l_conv;
        float* orow = out + (size_t)blockIdx.x * wa * (OUT_BF ? 32 : 64);     // a bf16 row is 128 bytes
        float v[11];
#pragma unroll
        for (int i = 0; i < 7; ++i) v[i] = s0[i];
        float carry = 0.0f;
#pragma unroll
        for (int t = 0; t < 7; ++t) carry = fmaf(v[t], wk[t], carry);
        for (int p = p_lo; p < p_hi; ++p, s0 += 4) {
#pragma unroll
            for (int i = 7; i < 11; ++i) v[i] = s0[i];
            const int wc0 = 2 * p - pad_l_pool;
            float best = -INFINITY;
#pragma unroll
            for (int pt = 0; pt < 3; ++pt) {
                float a = carry;
                if (pt > 0) {
                    a = 0.0f;
#pragma unroll
                    for (int t = 0; t < 7; ++t) a = fmaf(v[2 * pt + t], wk[t], a);
                }
                const int wc = wc0 + pt;
                // padded pool taps are ignored; a NaN tap wins and stays (fmaxf would drop it: a window that is NaN throughout
                // came out as relu(-inf + b) = 0). These are pre-ReLU values of either sign: no relu_max here, the IEEE maximum.
                best = (wc >= 0 && wc < w1) ? __builtin_elementwise_maximum(best, a) : best;
                if (pt == 2) carry = a;
            }
            const float y = relu_f(best + b);
            const unsigned o = (unsigned)p * 64u + (unsigned)c;
            if (OUT_BF) *at_bytes(reinterpret_cast<unsigned short*>(orow), 2u * o) = f2bf(y);
            else *at_bytes(orow, 4u * o) = y;
#pragma unroll
            for (int i = 0; i < 7; ++i) v[i] = v[i + 4];
        }
    }
    if constexpr (!OUT_BF && DS_SMALL_PRIO != 0) __builtin_amdgcn_s_setprio(0);
}

hipError_t launch_stem1(const float* signals, const float* w7x64, const float* bias64, float* out, int n,
                        int signal_len, int w1, int pad_l_conv, int wa, int pad_l_pool, int out_bf16, hipStream_t s)
{
    if (n <= 0) return hipSuccess;
    const size_t lds = (signal_len + 2 * STEM_HALO + 8) * sizeof(float);
    if (lds > 64 * 1024) return hipErrorInvalidValue;      // no opt-in to more: ds_create refuses signal_len > DS_MAX_SIGNAL_LEN
    if (out_bf16)
        hipLaunchKernelGGL(stem1_kernel<true>, dim3(n), dim3(64 * STEM1_WAVES), lds, s, signals, w7x64, bias64, out,
                           signal_len, w1, pad_l_conv, wa, pad_l_pool);
    else
        hipLaunchKernelGGL(stem1_kernel<false>, dim3(n), dim3(64 * STEM1_WAVES), lds, s, signals, w7x64, bias64, out,
                           signal_len, w1, pad_l_conv, wa, pad_l_pool);
    return hipGetLastError();
}

__global__ __launch_bounds__(256) void maxpool_s2_kernel(const float4* __restrict__ in, float4* __restrict__ out,
                                                          long total, int win, int wout, int pad_l, int ch4)
{
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const int c = (int)(i % ch4);
        const long r = i / ch4;
        const int wo = (int)(r % wout);
        const long site = r / wout;
        float4 m = make_float4(0.0f, 0.0f, 0.0f, 0.0f);      // ReLU outputs: 0 is f4max_relu's identity
#pragma unroll
        for (int t = 0; t < 3; ++t) {
            const int wi = 2 * wo + t - pad_l;
            if (wi >= 0 && wi < win) m = f4max_relu(m, in[(site * win + wi) * ch4 + c]);
        }
        out[i] = m;
    }
}

hipError_t launch_maxpool_s2(const float* in, float* out, int n, int win, int wout, int pad_l, int ch, hipStream_t s)
{
    const long total = (long)n * wout * (ch / 4);
    if (total <= 0) return hipSuccess;
    const int blocks = (int)((total + 255) / 256 < 4096 ? (total + 255) / 256 : 4096);
    hipLaunchKernelGGL(maxpool_s2_kernel, dim3(blocks), dim3(256), 0, s, (const float4*)in, (float4*)out, total, win, wout,
                       pad_l, ch / 4);
    return hipGetLastError();
}

// 7-wide average over the width axis, clipped at both ends (count = taps in bounds). One workgroup per site: a wave takes whole
// output rows, so the clipping is scalar, and a lane takes float4 columns: the site in a scalar base, (row, column) in a 32-bit
// lane offset, no division but the average's own. The sum is from 0.f over the taps in ascending order, then the IEEE division.
__global__ __launch_bounds__(256) void avgpool7_kernel(const float4* __restrict__ in, float4* __restrict__ out, int w, int ch4)
{
    if constexpr (DS_SMALL_PRIO != 0) __builtin_amdgcn_s_setprio(DS_SMALL_PRIO);
    const size_t base = (size_t)blockIdx.x * (size_t)w * (size_t)ch4;
    const float4* src = in + base;
    float4* dst = out + base;
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    for (int wo = wave; wo < w; wo += 4) {
        const int lo = wo - 3 > 0 ? wo - 3 : 0, hi = wo + 3 < w - 1 ? wo + 3 : w - 1;
        const float d = (float)(hi - lo + 1);
        for (int c = lane; c < ch4; c += 64) {
            float4 a = make_float4(0.f, 0.f, 0.f, 0.f);
            for (int wi = lo; wi <= hi; ++wi) {
                const float4 v = *at_bytes(src, 16u * (unsigned)(wi * ch4 + c));
                a.x += v.x; a.y += v.y; a.z += v.z; a.w += v.w;
            }
            *at_bytes(dst, 16u * (unsigned)(wo * ch4 + c)) = make_float4(a.x / d, a.y / d, a.z / d, a.w / d);
        }
    }
    if constexpr (DS_SMALL_PRIO != 0) __builtin_amdgcn_s_setprio(0);
}

hipError_t launch_avgpool7(const float* in, float* out, int n, int w, int ch, hipStream_t s)
{
    if (n <= 0 || w <= 0 || ch < 4) return hipSuccess;
    if ((long)w * (ch / 4) >= (1L << 27)) return hipErrorInvalidValue;      // a site's bytes in a 32-bit lane offset
    hipLaunchKernelGGL(avgpool7_kernel, dim3(n), dim3(256), 0, s, (const float4*)in, (float4*)out, w, ch / 4);
    return hipGetLastError();
}

// fc2 + sigmoid + argmax: one 256-thread block per site, float4 sweeps of the fc1 row, block reduce.
__global__ __launch_bounds__(256) void head_kernel(const float* __restrict__ fc1, const float* __restrict__ w2,
                                                    float* __restrict__ logits, float* __restrict__ act,
                                                    int* __restrict__ pred, int n, int J, int C, int nparts, size_t part_stride)
{
    __shared__ float part[4][16];
    if constexpr (DS_SMALL_PRIO_POST != 0) __builtin_amdgcn_s_setprio(DS_SMALL_PRIO_POST);
    const int site = blockIdx.x;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    // the site's row (and the same row of every partial product) in a scalar base, the lane's float4 in a 32-bit byte offset
    const char* xrow = reinterpret_cast<const char*>(fc1 + (size_t)site * J);
    const char* wrow = reinterpret_cast<const char*>(w2);
    const size_t part_bytes = part_stride * sizeof(float);
    float accv[16];
#pragma unroll
    for (int c = 0; c < 16; ++c) accv[c] = 0.0f;
    const int J4 = J >> 2;
    for (int k4 = tid; k4 < J4; k4 += 256) {
        const unsigned xo = (unsigned)k4 * 16u;
        float4 x = *reinterpret_cast<const float4*>(at_bytes(xrow, xo));
        for (int p = 1; p < nparts; ++p) {            // fc1 in partial products over ranges of K (the split dense at small forwards): summed in order
            const float4 y = *reinterpret_cast<const float4*>(at_bytes(xrow + p * part_bytes, xo));
            x.x += y.x; x.y += y.y; x.z += y.z; x.w += y.w;
        }
        const float* w = reinterpret_cast<const float*>(wrow + xo * (unsigned)C);
        if (C == 2) {
            const float4 wa = *reinterpret_cast<const float4*>(w);
            const float4 wb = *reinterpret_cast<const float4*>(w + 4);
            accv[0] = fmaf(x.x, wa.x, fmaf(x.y, wa.z, fmaf(x.z, wb.x, fmaf(x.w, wb.z, accv[0]))));
            accv[1] = fmaf(x.x, wa.y, fmaf(x.y, wa.w, fmaf(x.z, wb.y, fmaf(x.w, wb.w, accv[1]))));
        } else {
#pragma unroll
            for (int c = 0; c < 16; ++c)
                if (c < C) accv[c] += x.x * w[c] + x.y * w[C + c] + x.z * w[2 * C + c] + x.w * w[3 * C + c];
        }
    }
    for (int k = (J4 << 2) + tid; k < J; k += 256) {    // J not a multiple of 4
        const unsigned ko = (unsigned)k * 4u;
        float xk = *reinterpret_cast<const float*>(xrow + ko);
        for (int p = 1; p < nparts; ++p) xk += *reinterpret_cast<const float*>(xrow + p * part_bytes + ko);
        for (int c = 0; c < C; ++c) accv[c] += xk * *reinterpret_cast<const float*>(wrow + (ko * (unsigned)C + 4u * (unsigned)c));
    }
#pragma unroll
    for (int c = 0; c < 16; ++c) {
        if (c >= C) break;
        float a = accv[c];
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) a += __shfl_xor(a, off);
        if (lane == 0) part[wave][c] = a;
    }
    __syncthreads();
    if (tid == 0) {
        float best = 0.0f;
        int bi = 0;
        for (int c = 0; c < C; ++c) {
            const float a = (part[0][c] + part[1][c]) + (part[2][c] + part[3][c]);
            const float sg = sigmoidf_(a);
            logits[(size_t)site * C + c] = a;      // one lane, wave-uniform: scalar address arithmetic
            act[(size_t)site * C + c] = sg;
            if (c == 0 || sg > best) { best = sg; bi = c; }
        }
        pred[site] = bi;
    }
    if constexpr (DS_SMALL_PRIO_POST != 0) __builtin_amdgcn_s_setprio(0);
}

hipError_t launch_head(const float* fc1, const float* w2, float* logits, float* act, int* pred, int n, int J,
                       int class_num, hipStream_t s, int nparts, size_t part_stride)
{
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(head_kernel, dim3(n), dim3(256), 0, s, fc1, w2, logits, act, pred, n, J, class_num, nparts, part_stride);
    return hipGetLastError();
}

// Folded joint model: one workgroup per site, x = concatenation of up to three contiguous row segments.
__global__ __launch_bounds__(256) void head_folded_kernel(const HeadFoldedArgs a)
{
    __shared__ float part[4][16];
    if constexpr (DS_SMALL_PRIO_POST != 0) __builtin_amdgcn_s_setprio(DS_SMALL_PRIO_POST);
    const int site = blockIdx.x, C = a.C;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    float accv[16];
#pragma unroll
    for (int c = 0; c < 16; ++c) accv[c] = 0.0f;
    int koff = 0;
    if (a.bf16) {                                         // bf16 modes: bf16 rows, 8 values per 16 bytes
        for (int sg = 0; sg < a.nseg; ++sg) {             // uniform
        const char* x8 = reinterpret_cast<const char*>(reinterpret_cast<const unsigned short*>(a.seg[sg]) + (size_t)site * a.pitch[sg]);
        const char* wseg = reinterpret_cast<const char*>(a.w + (size_t)koff * C);      // scalar bases, 32-bit lane byte offsets
        for (int k8 = tid; k8 < (a.len[sg] >> 3); k8 += 256) {
            const float4 raw = *reinterpret_cast<const float4*>(x8 + (unsigned)k8 * 16u);
            const unsigned u[4] = {__float_as_uint(raw.x), __float_as_uint(raw.y), __float_as_uint(raw.z), __float_as_uint(raw.w)};
            const float* w = reinterpret_cast<const float*>(wseg + (unsigned)k8 * 32u * (unsigned)C);
            if (C == 2) {
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const float x0 = __uint_as_float(u[e] << 16), x1 = __uint_as_float(u[e] & 0xffff0000u);
                    const float4 wv = *reinterpret_cast<const float4*>(w + 4 * e);      // rows 2e, 2e + 1 of [k][2]
                    accv[0] = fmaf(x0, wv.x, fmaf(x1, wv.z, accv[0]));
                    accv[1] = fmaf(x0, wv.y, fmaf(x1, wv.w, accv[1]));
                }
            } else {
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const float x0 = __uint_as_float(u[e] << 16), x1 = __uint_as_float(u[e] & 0xffff0000u);
#pragma unroll
                    for (int c = 0; c < 16; ++c)
                        if (c < C) accv[c] += x0 * w[(2 * e) * C + c] + x1 * w[(2 * e + 1) * C + c];
                }
            }
        }
        koff += a.len[sg];
        }
    } else
    for (int sg = 0; sg < a.nseg; ++sg) {                 // uniform
        const int len = a.len[sg];
        const char* x4 = reinterpret_cast<const char*>(a.seg[sg] + (size_t)site * len);
        const char* wseg = reinterpret_cast<const char*>(a.w + (size_t)koff * C);
        for (int k4 = tid; k4 < (len >> 2); k4 += 256) {
            const unsigned xo = (unsigned)k4 * 16u;
            const float4 x = *reinterpret_cast<const float4*>(x4 + xo);
            const float* w = reinterpret_cast<const float*>(wseg + xo * (unsigned)C);
            if (C == 2) {
                const float4 wa = *reinterpret_cast<const float4*>(w);
                const float4 wb = *reinterpret_cast<const float4*>(w + 4);
                accv[0] = fmaf(x.x, wa.x, fmaf(x.y, wa.z, fmaf(x.z, wb.x, fmaf(x.w, wb.z, accv[0]))));
                accv[1] = fmaf(x.x, wa.y, fmaf(x.y, wa.w, fmaf(x.z, wb.y, fmaf(x.w, wb.w, accv[1]))));
            } else {
#pragma unroll
                for (int c = 0; c < 16; ++c)
                    if (c < C) accv[c] += x.x * w[c] + x.y * w[C + c] + x.z * w[2 * C + c] + x.w * w[3 * C + c];
            }
        }
        koff += len;
    }
#pragma unroll
    for (int c = 0; c < 16; ++c) {
        if (c >= C) break;
        float v = accv[c];
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
        if (lane == 0) part[wave][c] = v;
    }
    __syncthreads();
    if (tid == 0) {
        float best = 0.0f;
        int bi = 0;
        for (int c = 0; c < C; ++c) {
            const float v = (part[0][c] + part[1][c]) + (part[2][c] + part[3][c]);
            const float sgm = sigmoidf_(v);
            a.logits[(size_t)site * C + c] = v;
            a.act[(size_t)site * C + c] = sgm;
            if (c == 0 || sgm > best) { best = sgm; bi = c; }
        }
        a.pred[site] = bi;
    }
    if constexpr (DS_SMALL_PRIO_POST != 0) __builtin_amdgcn_s_setprio(0);
}

hipError_t launch_head_folded(const HeadFoldedArgs& a, hipStream_t s)
{
    if (a.n <= 0) return hipSuccess;
    hipLaunchKernelGGL(head_folded_kernel, dim3(a.n), dim3(256), 0, s, a);
    return hipGetLastError();
}

// ds_forward_device: the caller's five device arrays into the slot's contiguous input block and the slot's outputs
// back to the caller -- small launches instead of five + two copy dispatches per forward (the captured graphs read and write the
// slot's own buffers). The gather copies the elements [lo, hi) of the five arrays laid end to end ([kmer | means | stds | lens] =
// 4 n T elements, the event model's inputs, then n S signals), so that each branch's inputs can be copied on that branch's stream.
// Both copy whole ranges of 32-bit words. copy_words is one such range over the x dimension of the grid: source and destination
// are wave-uniform, so each pass is a scalar base plus the lane's constant offset, 16 bytes per lane where both ends are 16-byte
// aligned (the caller's arrays need not be) and 4 bytes otherwise; the words past the last whole 16 bytes go one per lane.
__device__ __forceinline__ void copy_words(const unsigned* __restrict__ src, unsigned* __restrict__ dst, long cnt)
{
    const unsigned tid = threadIdx.x;
    const long step = (long)gridDim.x * 256;
    if (((reinterpret_cast<uintptr_t>(src) | reinterpret_cast<uintptr_t>(dst)) & 15) == 0) {
        const long cnt4 = cnt >> 2;
        for (long i0 = (long)blockIdx.x * 256; i0 < cnt4; i0 += step) {
            const unsigned left = (unsigned)(cnt4 - i0 < 256 ? cnt4 - i0 : 256);
            if (tid < left) (reinterpret_cast<uint4*>(dst) + i0)[tid] = (reinterpret_cast<const uint4*>(src) + i0)[tid];
        }
        if (blockIdx.x == 0 && tid < (unsigned)(cnt & 3)) (dst + 4 * cnt4)[tid] = (src + 4 * cnt4)[tid];
    } else {
        for (long i0 = (long)blockIdx.x * 256; i0 < cnt; i0 += step) {
            const unsigned left = (unsigned)(cnt - i0 < 256 ? cnt - i0 : 256);
            if (tid < left) (dst + i0)[tid] = (src + i0)[tid];
        }
    }
}

// blockIdx.y + seg0 names the array: 0 .. 3 = kmer, means, stds, lens (n T words each, B T apart in the block), 4 = signals (n S)
__global__ __launch_bounds__(256) void gather_inputs_kernel(const int* __restrict__ kmer, const float* __restrict__ means,
                                                            const float* __restrict__ stds, const float* __restrict__ lens,
                                                            const float* __restrict__ signals, float* __restrict__ block,
                                                            int n, int T, int S, int B, long lo, long hi, int seg0)
{
    if constexpr (DS_SMALL_PRIO != 0) __builtin_amdgcn_s_setprio(DS_SMALL_PRIO);
    const long nt = (long)n * T;
    const long bt = (long)B * T;
    const int seg = seg0 + (int)blockIdx.y;
    const void* arr = seg == 0 ? (const void*)kmer : seg == 1 ? (const void*)means : seg == 2 ? (const void*)stds
                    : seg == 3 ? (const void*)lens : (const void*)signals;
    const long first = seg * nt, last = seg < 4 ? first + nt : first + (long)n * S;      // the array's place in [0, 4 n T + n S)
    const long from = lo > first ? lo : first, to = hi < last ? hi : last;
    if (from < to)
        copy_words(static_cast<const unsigned*>(arr) + (from - first), reinterpret_cast<unsigned*>(block) + seg * bt + (from - first), to - from);
    if constexpr (DS_SMALL_PRIO != 0) __builtin_amdgcn_s_setprio(0);
}

// blockIdx.y: 0 = act (n C words), 1 = pred (n)
__global__ __launch_bounds__(256) void scatter_outputs_kernel(const float* __restrict__ act, const int* __restrict__ pred,
                                                              float* __restrict__ act_out, int* __restrict__ pred_out, int n, int C)
{
    if constexpr (DS_SMALL_PRIO_POST != 0) __builtin_amdgcn_s_setprio(DS_SMALL_PRIO_POST);
    if (blockIdx.y == 0) copy_words(reinterpret_cast<const unsigned*>(act), reinterpret_cast<unsigned*>(act_out), (long)n * C);
    else copy_words(reinterpret_cast<const unsigned*>(pred), reinterpret_cast<unsigned*>(pred_out), n);
    if constexpr (DS_SMALL_PRIO_POST != 0) __builtin_amdgcn_s_setprio(0);
}

hipError_t launch_gather_inputs(const int* kmer, const float* means, const float* stds, const float* lens, const float* signals,
                                float* block, int n, int T, int S, int B, int col_lo, int col_hi, hipStream_t s)
{
    // [col_lo, col_hi): array boundaries as per-site offsets (0, T, 2 T, 3 T, 4 T, 4 T + S); 4 T lies between the two branches' inputs
    if (n <= 0 || col_lo < 0 || col_hi > 4 * T + S || col_lo >= col_hi) return hipSuccess;
    const long lo = (long)n * col_lo, hi = (long)n * col_hi;
    const int seg0 = std::min(col_lo / T, 4), seg1 = std::min((col_hi - 1) / T, 4);      // first and last array the range touches
    const long widest = (long)n * (seg1 == 4 ? std::max(S, seg0 < 4 ? T : 0) : T);
    const int grid = (int)std::min<long>((widest + 1023) / 1024, 1024);
    hipLaunchKernelGGL(gather_inputs_kernel, dim3(grid, seg1 - seg0 + 1), dim3(256), 0, s, kmer, means, stds, lens, signals, block, n, T, S,
                       B, lo, hi, seg0);
    return hipGetLastError();
}

hipError_t launch_scatter_outputs(const float* act, const int* pred, float* act_out, int* pred_out, int n, int C, hipStream_t s)
{
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(scatter_outputs_kernel, dim3((int)std::min<long>(((long)n * C + 1023) / 1024, 1024), 2), dim3(256), 0, s, act, pred,
                       act_out, pred_out, n, C);
    return hipGetLastError();
}

// ---- bf16-mode elementwise kernels: 8 channels (16 B) per thread ----
__global__ __launch_bounds__(256) void maxpool_s2_bf16_kernel(const float4* __restrict__ in, float4* __restrict__ out,
                                                               long total, int win, int wout, int pad_l, int ch8)
{
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const int c = (int)(i % ch8);
        const long r = i / ch8;
        const int wo = (int)(r % wout);
        const long site = r / wout;
        float4 m = make_float4(0.0f, 0.0f, 0.0f, 0.0f);      // ReLU outputs: 0 is bf8max_relu's identity
#pragma unroll
        for (int t = 0; t < 3; ++t) {
            const int wi = 2 * wo + t - pad_l;
            if (wi >= 0 && wi < win) m = bf8max_relu(m, in[(site * win + wi) * ch8 + c]);
        }
        out[i] = m;
    }
}

hipError_t launch_maxpool_s2_bf16(const float* in, float* out, int n, int win, int wout, int pad_l, int ch_ld, hipStream_t s)
{
    const long total = (long)n * wout * (ch_ld / 8);
    if (total <= 0) return hipSuccess;
    const int blocks = (int)((total + 255) / 256 < 8192 ? (total + 255) / 256 : 8192);
    hipLaunchKernelGGL(maxpool_s2_bf16_kernel, dim3(blocks), dim3(256), 0, s, (const float4*)in, (float4*)out, total, win,
                       wout, pad_l, ch_ld / 8);
    return hipGetLastError();
}

// avgpool(7, s1, SAME, divisor = valid taps) of the bf16 module output [n][w][ld_in] -> joint[n][out_off + w*ch + c] (bf16)
__global__ __launch_bounds__(256) void avgpool7_bf16_kernel(const float4* __restrict__ in, unsigned short* __restrict__ out,
                                                             long total, int w, int ch8, int ld_in8, long out_ld, int out_off)
{
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const int c = (int)(i % ch8);
        const long r = i / ch8;
        const int wo = (int)(r % w);
        const long site = r / w;
        float a[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        int cnt = 0;
        for (int t = -3; t <= 3; ++t) {
            const int wi = wo + t;
            if (wi < 0 || wi >= w) continue;
            const float4 v = in[(site * w + wi) * ld_in8 + c];
            const unsigned u[4] = {__float_as_uint(v.x), __float_as_uint(v.y), __float_as_uint(v.z), __float_as_uint(v.w)};
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                a[2 * q] += __uint_as_float(u[q] << 16);
                a[2 * q + 1] += __uint_as_float(u[q] & 0xffff0000u);
            }
            ++cnt;
        }
        const float d = (float)cnt;
        unsigned o[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) o[q] = pack_bf2(a[2 * q] / d, a[2 * q + 1] / d);
        *reinterpret_cast<uint4*>(out + site * out_ld + out_off + ((long)wo * ch8 + c) * 8) = make_uint4(o[0], o[1], o[2], o[3]);
    }
}

hipError_t launch_avgpool7_bf16(const float* in, float* joint, int n, int w, int ch, int ld_in, int joint_ld, int joint_off,
                                hipStream_t s)
{
    const long total = (long)n * w * (ch / 8);
    if (total <= 0) return hipSuccess;
    const int blocks = (int)((total + 255) / 256 < 8192 ? (total + 255) / 256 : 8192);
    hipLaunchKernelGGL(avgpool7_bf16_kernel, dim3(blocks), dim3(256), 0, s, (const float4*)in, (unsigned short*)joint, total, w,
                       ch / 8, ld_in / 8, (long)joint_ld, joint_off);
    return hipGetLastError();
}

// joint[:, 0:256] = bf16(h_fw), joint[:, 256:512] = bf16(h_bw)     (layers.py:171-172, bf16 FC operand)
template <bool SRC_BF>
__global__ __launch_bounds__(256) void pack_event_feat_bf16_kernel(const float* __restrict__ hfw, const float* __restrict__ hbw,
                                                                    unsigned short* __restrict__ joint, int n, long joint_ld)
{
    const long i = blockIdx.x * (long)blockDim.x + threadIdx.x;      // one thread per 4 values
    if (i >= (long)n * 128) return;
    const int site = (int)(i / 128), q = (int)(i % 128);
    uint2 o;
    if (SRC_BF) {        // h already bf16 ([n][256] bf16): plain copy
        const unsigned short* src = reinterpret_cast<const unsigned short*>(q < 64 ? hfw : hbw) + (size_t)site * 256 + (q & 63) * 4;
        o = *reinterpret_cast<const uint2*>(src);
    } else {
        const float* src = (q < 64 ? hfw : hbw) + (size_t)site * 256 + (q & 63) * 4;
        const float4 v = *reinterpret_cast<const float4*>(src);
        o = make_uint2(pack_bf2(v.x, v.y), pack_bf2(v.z, v.w));
    }
    *reinterpret_cast<uint2*>(joint + site * joint_ld + q * 4) = o;
}

hipError_t launch_pack_event_feat_bf16(const float* hfw, const float* hbw, float* joint, int n, int joint_ld, int src_bf16,
                                       hipStream_t s)
{
    if (n <= 0) return hipSuccess;
    const dim3 grid((unsigned)(((long)n * 128 + 255) / 256));
    if (src_bf16)
        hipLaunchKernelGGL(pack_event_feat_bf16_kernel<true>, grid, dim3(256), 0, s, hfw, hbw, (unsigned short*)joint, n, (long)joint_ld);
    else
        hipLaunchKernelGGL(pack_event_feat_bf16_kernel<false>, grid, dim3(256), 0, s, hfw, hbw, (unsigned short*)joint, n, (long)joint_ld);
    return hipGetLastError();
}

__global__ __launch_bounds__(256) void embed_table_kernel(const float* __restrict__ emb, const float* __restrict__ kernel,
                                                           float* __restrict__ table, int vocab, int esize, int ncol)
{
    const long i = blockIdx.x * (long)blockDim.x + threadIdx.x;
    if (i >= (long)vocab * ncol) return;
    const int col = (int)(i % ncol);
    const int v = (int)(i / ncol);
    float a = 0.0f;
    for (int e = 0; e < esize; ++e) a = fmaf(emb[(size_t)v * esize + e], kernel[(size_t)e * ncol + col], a);
    table[i] = a;
}

hipError_t launch_embed_table(const float* emb, const float* kernel, float* table, int vocab, int esize, int ncol,
                              hipStream_t s)
{
    const long total = (long)vocab * ncol;
    hipLaunchKernelGGL(embed_table_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, emb, kernel, table, vocab,
                       esize, ncol);
    return hipGetLastError();
}

}  // namespace ds
