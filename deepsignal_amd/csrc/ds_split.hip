// ds_split.hip -- split-operand kernels (DS_PRECISION_BF16X3): fp32-class arithmetic on the bf16 matrix pipe of gfx950.
//
// On gfx950 the fp32 MFMA (v_mfma_f32_32x32x2_f32) runs at 1/16 of the bf16 MFMA rate and there is no xf32/tf32 form
// (MI355X_MICROARCH.md, matrix-core table). An fp32 operand x is therefore carried as three bf16 TERMS
//     t0 = bf16(x), t1 = bf16(x - t0), t2 = bf16(x - t0 - t1)        (round to nearest even; both differences are exact in fp32)
// which together hold all 24 significant bits of x, and a product a * b is the fp32-accumulated sum of the six
// bf16 x bf16 products (each exact in fp32) a0 b0, a0 b1, a1 b0, a0 b2, a1 b1, a2 b0 -- the three dropped ones lie below
// 2^-24 of the product. Six v_mfma_f32_32x32x16_bf16 (6 x 32 cycles) replace the eight v_mfma_f32_32x32x2_f32 (8 x 64 cycles)
// of a 32 x 32 x 16 block: 0.375 of the matrix-pipe time at fp32-class accuracy (CPU statement:
// oracle/torch_statement.py::forward_split; tools/split_emulation.py: 1.3 - 1.9e-5 from the float64 oracle on the
// trained-regime sets where native fp32 is 2.8 - 3.3e-5). Weights are split ONCE at load (ds_engine.cpp pack_b_split),
// activations ONCE where they are produced or staged (never inside a K loop); everything between the matrix products -- bias,
// ReLU, residual add, pooling -- is fp32, and the activations that travel through global memory are the fp32 engine's fp32 rows.
//
// Reference arithmetic: deepsignal/layers.py:87-139 (inception_layer), 205-232 (the eleven modules of incept_net).
#include "ds_device.h"

namespace ds {

// ---- term helpers ---------------------------------------------------------------------------------------------------
__device__ __forceinline__ float bf_lo(unsigned p) { return __uint_as_float(p << 16); }
__device__ __forceinline__ float bf_hi(unsigned p) { return __uint_as_float(p & 0xffff0000u); }
// the three bf16 terms of four fp32 values, as three 8-byte groups of four bf16 (channel order kept)
__device__ __forceinline__ void split3x4(float x0, float x1, float x2, float x3, uint2& t0, uint2& t1, uint2& t2)
{
    unsigned a = pack_bf2(x0, x1), b = pack_bf2(x2, x3);
    t0 = make_uint2(a, b);
    float r0 = x0 - bf_lo(a), r1 = x1 - bf_hi(a), r2 = x2 - bf_lo(b), r3 = x3 - bf_hi(b);
    a = pack_bf2(r0, r1); b = pack_bf2(r2, r3);
    t1 = make_uint2(a, b);
    r0 -= bf_lo(a); r1 -= bf_hi(a); r2 -= bf_lo(b); r3 -= bf_hi(b);
    t2 = make_uint2(pack_bf2(r0, r1), pack_bf2(r2, r3));
}
// the first / last three of the six term products of one 32 x 32 x 16 block (w = the weight fragment's terms, a = the
// activation fragment's terms), small products first. Issued TRANSPOSED like every MFMA of the fused modules: mfma(weights,
// activations) gives (X W)^T, so a lane holds 4 x 4 consecutive output channels of ONE activation row.
__device__ __forceinline__ floatx16 mfma3_lo(const float4 (&w)[3], float4 a0, float4 a1, float4 a2, floatx16 c)
{
    c = mfma_bf(w[2], a0, c);
    c = mfma_bf(w[0], a2, c);
    c = mfma_bf(w[1], a1, c);
    return c;
}
__device__ __forceinline__ floatx16 mfma3_hi(const float4 (&w)[3], float4 a0, float4 a1, floatx16 c)
{
    c = mfma_bf(w[1], a0, c);
    c = mfma_bf(w[0], a1, c);
    c = mfma_bf(w[0], a0, c);
    return c;
}

// ---- DS_PRECISION_FP16X2: the same kernels on TWO fp16 terms ------------------------------------------------------------
//     h0 = fp16(x), h1 = fp16(x - h0)        (round to nearest even, subnormal terms kept; the difference is exact in fp32)
// hold 22 significant bits of x, and a product is the fp32-accumulated sum of the three fp16 x fp16 products a1 b0, a0 b1, a0 b0
// (small first): three v_mfma_f32_32x32x16_f16 per 32 x 32 x 16 block at the cycles of the bf16 form, 4 operand bytes per element
// instead of 6. No scaling: the conversion does not saturate, so an operand beyond +-65504 becomes Inf, h1 = -Inf, and the site
// comes out NaN -- never a wrong finite number. (CPU statement: tests/fp16x2_statement.py.)
typedef _Float16 halfx8 __attribute__((ext_vector_type(8)));
typedef _Float16 halfx2_t __attribute__((ext_vector_type(2)));
__device__ __forceinline__ floatx16 mfma_hf(float4 a, float4 b, floatx16 c)
{
    return __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(halfx8, a), __builtin_bit_cast(halfx8, b), c, 0, 0, 0);
}
// two floats -> one dword of two fp16, round to nearest even, overflow to Inf (a plain conversion: never the round-toward-zero pack)
__device__ __forceinline__ unsigned pack_hf2(float a, float b)
{
    const float2_t f = {a, b};
    return __builtin_bit_cast(unsigned, __builtin_convertvector(f, halfx2_t));
}
__device__ __forceinline__ float hf_lo(unsigned p) { return (float)__builtin_bit_cast(halfx2_t, p).x; }
__device__ __forceinline__ float hf_hi(unsigned p) { return (float)__builtin_bit_cast(halfx2_t, p).y; }

// for_terms<NT>(f) calls f(p) for p = 0 .. NT - 1 with p a compile-time constant: the statements stand in the instantiated body one after
// the other, as if written out per term. The kernels use it, an unrolled `for` over the terms, or a getter (lo_of / hi_of below) from
// place to place: the arithmetic is the same, but hipcc's instruction order and register allocation follow the shape of the source, and
// each place has the shape that leaves the three-term kernels' device code as it was when the terms were written out by hand
// (tools/compare_device_asm.py; profiles/fp16x2_device_asm.md).
template <int P> struct TermIndex { constexpr operator int() const { return P; } };
template <int N, class Fn>
__device__ __forceinline__ void for_terms(Fn&& f)
{
    if constexpr (N > 0) { for_terms<N - 1>(f); f(TermIndex<N - 1>{}); }
}

// The term format of a kernel body: NT terms per operand, NP products per MAC, issued as a `lo` group (the small products) and a
// `hi` group -- every kernel of a format issues the products of one accumulator in this order, so all its tilings give the same bits.
struct TermsBf3 {
    static constexpr int NT = 3, NP = 6;
    // product P of the pinned sequence: weight term WI, activation term AI (mfma3_lo / mfma3_hi order)
    static constexpr int wi(int p) { return p == 0 ? 2 : p == 1 ? 0 : p == 2 ? 1 : p == 3 ? 1 : 0; }
    static constexpr int ai(int p) { return p == 0 ? 0 : p == 1 ? 2 : p == 2 ? 1 : p == 3 ? 0 : p == 4 ? 1 : 0; }
    static __device__ __forceinline__ floatx16 mfma(float4 a, float4 b, floatx16 c) { return mfma_bf(a, b, c); }
    static __device__ __forceinline__ void split4(float x0, float x1, float x2, float x3, uint2 (&t)[3]) { split3x4(x0, x1, x2, x3, t[0], t[1], t[2]); }
    static __device__ __forceinline__ floatx16 lo(const float4 (&w)[3], const float4 (&a)[3], floatx16 c) { return mfma3_lo(w, a[0], a[1], a[2], c); }
    static __device__ __forceinline__ floatx16 hi(const float4 (&w)[3], const float4 (&a)[3], floatx16 c) { return mfma3_hi(w, a[0], a[1], c); }
    // the same with the activation terms behind a getter a(p), for fragments that are not stored term-contiguous
    template <class G> static __device__ __forceinline__ floatx16 lo_of(const float4 (&w)[3], G&& a, floatx16 c) { return mfma3_lo(w, a(TermIndex<0>{}), a(TermIndex<1>{}), a(TermIndex<2>{}), c); }
    template <class G> static __device__ __forceinline__ floatx16 hi_of(const float4 (&w)[3], G&& a, floatx16 c) { return mfma3_hi(w, a(TermIndex<0>{}), a(TermIndex<1>{}), c); }
};
struct TermsHf2 {
    static constexpr int NT = 2, NP = 3;
    static constexpr int wi(int p) { return p == 1 ? 1 : 0; }      // (w0, a1) (w1, a0) | (w0, a0)
    static constexpr int ai(int p) { return p == 0 ? 1 : 0; }
    static __device__ __forceinline__ floatx16 mfma(float4 a, float4 b, floatx16 c) { return mfma_hf(a, b, c); }
    static __device__ __forceinline__ void split4(float x0, float x1, float x2, float x3, uint2 (&t)[2])
    {
        const unsigned a = pack_hf2(x0, x1), b = pack_hf2(x2, x3);
        t[0] = make_uint2(a, b);
        t[1] = make_uint2(pack_hf2(x0 - hf_lo(a), x1 - hf_hi(a)), pack_hf2(x2 - hf_lo(b), x3 - hf_hi(b)));
    }
    static __device__ __forceinline__ floatx16 lo(const float4 (&w)[2], const float4 (&a)[2], floatx16 c)
    {
        c = mfma_hf(w[0], a[1], c);
        c = mfma_hf(w[1], a[0], c);
        return c;
    }
    static __device__ __forceinline__ floatx16 hi(const float4 (&w)[2], const float4 (&a)[2], floatx16 c) { return mfma_hf(w[0], a[0], c); }
    template <class G> static __device__ __forceinline__ floatx16 lo_of(const float4 (&w)[2], G&& a, floatx16 c)
    {
        const float4 t[2] = {a(TermIndex<0>{}), a(TermIndex<1>{})};
        return lo(w, t, c);
    }
    template <class G> static __device__ __forceinline__ floatx16 hi_of(const float4 (&w)[2], G&& a, floatx16 c) { return mfma_hf(w[0], a(TermIndex<0>{}), c); }
};

// ---------------------------------------------------------------------------------------------------------------------
// Fused inception modules, split operands. Tile, chaining and phases are those of inception_fused_kernel (ds_kernels.hip): one
// workgroup (8 waves) owns a tile of whole sites (<= 96 rows) and takes it through the modules of one width class; only a chain's
// first module may take the stride-2 max pool of its input while staging;
//   P1  [rows x cin] x [cin x 256]: wave w owns n-tile w for all m-tiles, K in chunks of 16 channels = ONE bf16 k-step.
//       The staging waves (0 .. 2 TM - 1) load the chunk's fp32 rows ONCE, park a raw copy in LDS (T2's region, idle during P1), and
//       one step later read the row and its two neighbours back from it, take the 3-tap max (branch 1's maxpool(3, 1, SAME), padded
//       taps ignored = the own row), split both the plain and the pooled values into terms and write ONE staged row
//       [plain t0 | t1 | t2 | pooled t0 | t1 | t2] x 32 B: every wave's fragment reads are three ds_read_b128 at immediate
//       offsets from one address (waves 6, 7: the pooled half), no wave pools or splits inside its MFMA stream. Per chunk and wave:
//       3 weight fragments (one per term, global -> VGPR), 3 x TM activation fragments, 6 x TM MFMAs; one barrier per chunk.
//   P2  the 1x3 / 1x5 convs from the 32-channel intermediates, which the P1 epilogue wrote to LDS as terms (T1, zero halo rows =
//       SAME padding), dealt by (conv, n-tile): a wave takes its weight fragments through all the m-tiles it owns. Branch 5's
//       64-channel intermediate goes to LDS as terms as well (T2); its last 1x1 accumulates on top of the stem accumulators.
// LDS (bytes): staged chunks 2 x rows x 208 (later the fp32 b1|b2 output tile) | T2 rows x 400 (raw chunks during P1) | T1
// (spt (W + 4) + 5) x 592: 143 - 147 KB for 96-row tiles, one workgroup per CU. Every row stride is an odd number of 16-byte slots.
// What bounds it (round 6, profiles/r06_chain_p1_experiments.md): a P1 step takes ~1,660 cycles for 1,152 of MFMA; barrier, transform
// arithmetic and staged writes each cost nothing when removed alone, the 30 KiB of weight fragments and rows a step asks the L2 for do
// (18 B/clk per CU against 26 at full matrix rate), and eight re-orderings of the step's work all took the same time. Per module 47 - 53 k
// cycles: P1 25 k in its loop + 4.5 - 8 k of start-up, P1 epilogue + barrier 6 - 7.7 k, P2 11.6 k (7.7 k of MFMA).
constexpr int S_LDY = 400;      // b1|b2 output tile row: 96 floats + 4
constexpr int S_LDR = 80;       // raw fp32 chunk row: 16 floats + 16 B
constexpr int S_T1P = 192;      // bytes between the terms of a T1 row (96 channels x 2 B, whatever the number of terms)
constexpr int S_T2P = 128;      // ... of a T2 row (64 channels x 2 B)
#ifndef DS_SPLIT_VD
#define DS_SPLIT_VD 4       // register stages of the stagers' row loads (chunk c + VD is requested at step c)
#endif
#ifndef DS_SPLIT_BD
#define DS_SPLIT_BD 2       // register stages of a wave's P1 weight fragments (chunk c + BD - 1 is requested at step c)
#endif
#ifndef DS_SPLIT_SW0
#define DS_SPLIT_SW0 0          // the two waves whose phase stamps a debug build records (tools/stamps.py prints them as "wave 0" / "wave 7")
#define DS_SPLIT_SW1 7
#endif
template <int R> struct SplitRole { static constexpr int value = R; };
// Row strides by term format (three bf16 terms | two fp16 terms), each an odd number of 16-byte slots:
template <class F> struct ChainRows {
    static constexpr int LDP = 2 * F::NT * 32 + 16;          // staged chunk row: 2 NT x 32 B + 16              208 | 144
    static constexpr int LD1 = F::NT * S_T1P + 16;           // T1 row: NT terms x 96 channels x 2 B + 16       592 | 400
    static constexpr int LD2 = F::NT * S_T2P + 16;           // T2 row: NT terms x 64 channels x 2 B + 16       400 | 272
    // the first region holds the two staged chunks during P1 and the fp32 b1|b2 output tile after it: per tile row the larger of
    // both (two terms: the output tile's 400 B, not the 288 of two staged rows)
    static constexpr int LD0 = 2 * LDP > S_LDY ? 2 * LDP : S_LDY;
    static_assert(2 * S_LDR <= LD2, "the raw chunk copies of P1 live in T2's region");
    static size_t lds_bytes(int tm, int W, int spt)
    {
        const int tr32 = tm * 32;
        return (size_t)tr32 * LD0 + (size_t)tr32 * LD2 + (size_t)(spt * (W + 4) + 5) * LD1 + (size_t)tr32 * 4 + 192 * 4;
    }
};

size_t inception_fused_split_lds_bytes(int tm, int W, int spt) { return ChainRows<TermsBf3>::lds_bytes(tm, W, spt); }

// weights of one second-stage conv unit: ntaps x 2 k-steps x NT terms (<= 10 NT fragments); the packed panel of an n-tile holds
// ks k-steps of NT 1 KiB fragments each (pack_b_split)
template <class F>
__device__ __forceinline__ void fuseds_unit_prefetch(const float* __restrict__ Bp, int ntaps, int nt, int lane, float4 (&ub)[10 * F::NT])
{
    constexpr int NT = F::NT;
    const int ks = (ntaps * 32 + 63) / 64 * 4;
    const float* bsrc = Bp + ((size_t)(nt * ks) * NT * 64 + lane) * 4;
#pragma unroll
    for (int g = 0; g < 10 * NT; ++g)
        if (g < ntaps * 2 * NT) ub[g] = gload4(bsrc + g * 256);
}

// one second-stage conv on NM m-tiles at once: one set of weights, NM accumulators, TWO fragment buffers: the three reads of the next
// (tap, k-step, m-tile) group are issued in front of the six MFMAs of the current one and land while those run (192 cycles of MFMA
// per group against ~100 of LDS latency); left to itself hipcc issues a group's reads directly in front of its MFMAs and every group
// waits for the LDS (6.8 k cycles for 108 MFMAs with one wave per SIMD active).
template <class F, int NTAPS, int NM>
__device__ __forceinline__ void fuseds_conv_units(const char* T1, const int (&rm)[NM], int cbyte, int lane, const float4 (&ub)[10 * F::NT], floatx16 (&acc)[NM])
{
    constexpr int NT = F::NT, S_LD1 = ChainRows<F>::LD1;
    const char* base[NM];
#pragma unroll
    for (int m = 0; m < NM; ++m) base[m] = T1 + (rm[m] - NTAPS / 2) * S_LD1 + cbyte + (lane >> 5) * 16;
    float4 fr[2][NT];
#pragma unroll
    for (int p = 0; p < NT; ++p) fr[0][p] = *reinterpret_cast<const float4*>(base[0] + p * S_T1P);
    int cur = 0;
#pragma unroll
    for (int t = 0; t < NTAPS; ++t)
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int q = (t * 2 + j) * NT;
            float4 w[NT];
            for_terms<NT>([&](auto p) __attribute__((always_inline)) { w[p] = ub[q + p]; });
#pragma unroll
            for (int m = 0; m < NM; ++m) {
                // next group: (t, j, m + 1), or m-tile 0 of the next k-step / tap
                const int mn = m + 1 < NM ? m + 1 : 0;
                const int jn = m + 1 < NM ? j : (j + 1) & 1;
                const int tn = (m + 1 < NM || j == 0) ? t : t + 1;
                if (tn < NTAPS) {
                    const char* arow = base[mn] + tn * S_LD1 + jn * 32;
#pragma unroll
                    for (int p = 0; p < NT; ++p) fr[cur ^ 1][p] = *reinterpret_cast<const float4*>(arow + p * S_T1P);
                }
                acc[m] = F::lo(w, fr[cur], acc[m]);
                acc[m] = F::hi(w, fr[cur], acc[m]);
                cur ^= 1;
                __builtin_amdgcn_sched_barrier(0);
            }
        }
}

// ---------------------------------------------------------------------------------------------------------------------
// conv_layer2 (1x1, 64 -> 128) + conv_layer3 (1x3, 128 -> 256), BN folded, ReLU (layers.py:192-203), split operands: the
// structure of stem23_kernel (ds_kernels.hip) -- a tile of whole sites (<= 96 rows), 8 waves, conv2's rows never leave LDS (zero halo
// row on either side of every site = conv3's SAME padding), conv3 with wave w = output channels [32 w, 32 w + 32) of all three
// m-tiles and its weights streamed global -> VGPR -- with the input rows split into terms while they are staged and conv2's rows
// split in its epilogue. LDS: input terms 96 x 400 B + conv2 terms (spt (W + 2) + 3) x 784 B = 117 KB, one workgroup per CU.
// Per tile conv3 streams 576 KB of weight fragments (24 k-steps x 3 terms x 8 n-tiles) for 27.6 k cycles of MFMA per SIMD (matrix
// pipe 0.51 busy).
// (two fp16 terms: 272 and 528 B, 17 and 33 sixteen-byte slots -- odd like the three-term strides; two thirds of the bytes. The tile stays as shipped.)
template <class F> struct Stem23Rows {
    static constexpr int SX = F::NT * 128 + 16;      // input term row: NT x 64 channels x 2 B + 16 (three terms: 400)
    static constexpr int ST = F::NT * 256 + 16;      // conv2 term row: NT x 128 channels x 2 B + 16 (three terms: 784 = 49 x 16 B)
    static size_t lds_bytes(int W, int spt) { return (size_t)96 * SX + (size_t)(spt * (W + 2) + 3) * ST + 96 * 4; }
};
size_t stem23_split_lds_bytes(int W, int spt) { return Stem23Rows<TermsBf3>::lds_bytes(W, spt); }

// =====================================================================================================================
// BiLSTM cells and the joint model's dense(J, J), split operands (stage 2 of the split-operand engine).
//
// Both are plain GEMMs whose operands already lie in global memory as 1 KiB MFMA-fragment images, so they share one main loop:
// the structure of lstm_cell_bf16_kernel (ds_kernels.hip) -- workgroup tile 64 MTW rows x 64 NTW columns, 4 waves as 2 x 2,
// fragments global -> LDS by LDS-DMA into a ring of three stages, requests two stages ahead, ONE barrier per stage behind a
// counted vmcnt -- with every fragment in three terms: per k-step (16 k) a workgroup takes 3 (2 MTW + 2 NTW) KiB and issues
// 6 MTW NTW MFMAs per wave. The activation operand is fragment-major with the three terms of a k-step next to each other,
//     [m-tile of 32 rows][k-step of 16][term][64 lanes][8 bf16]      (lane (r, half) holds k = 16 s + 8 half .. + 7 of row 32 m + r),
// which is what a cell's epilogue writes for h (split once, where it is produced) and what pack_joint_split_kernel writes for the
// joint row; the weights are pack_b_split's panels [n-tile][k-step][term][64][8].
// One workgroup per CU means one wave per SIMD: hipcc's read -> wait -> MFMA schedule and the requests' issue time in front of the
// MFMAs cost these kernels 12 - 25 % until SplitRing::run pinned the order (round 5). What bounds them since is what a CU takes in
// from the L2 (round 6): at full matrix rate a tile asks for 2048 (M + N) / (M N) B/clk -- 32 at 128 x 128, where
// the cells move 23; 18.7 at 256 x 192, where the dense is bound by the matrix pipe -- and the same 128 x 128 tile by EIGHT waves (two per
// SIMD, WM x WN = 4 x 2) takes the same time. The split cells use the 128 x 128 tile: slower alone than 64 x 64, faster in the pipelined step;
// 128 x 256 (24 B/clk, half the workgroups, 108 KB rings) is 5 % slower there.
// (per term format F: F::NT term fragments of 1 KiB per k-step -- 3 KiB in three bf16 terms, 2 KiB in two fp16 terms; an m-tile of a
// split h buffer is 16 k-steps = 256 units)

#ifndef DS_SPLIT_LSTM_SLOTS
#define DS_SPLIT_LSTM_SLOTS 3
#endif
#ifndef DS_SPLIT_DENSE_SLOTS
#define DS_SPLIT_DENSE_SLOTS 4
#endif
// WM x WN waves (= 4), each MTW x NTW tiles of 32 x 32; NSLOT ring slots: stage st + NSLOT is requested into the slot of
// stage st once every wave has read it
template <int MTW, int NTW, int WM = 2, int WN = 2, int NSLOT = 3, class F = TermsBf3>
struct SplitRing {
    static constexpr int NT = F::NT, NP = F::NP;
    static constexpr int SPLIT_KSTEP_BYTES = NT * 1024;       // the term fragments of one k-step
    static constexpr int SPLIT_MT_BYTES = 16 * SPLIT_KSTEP_BYTES;
    static constexpr int NW = WM * WN;                       // waves per workgroup: 4, or 8 (two per SIMD: one wave's waits and requests under the other's MFMAs)
    static_assert(NW == 4 || NW == 8, "four or eight waves per workgroup");
    static constexpr int FRA = WM * MTW, FRB = WN * NTW;
    static constexpr int NF1 = NT * (FRA + FRB);              // 1 KiB fragments per k-step
    // one k-step per ring stage. The fragments of a stage are dealt to the waves round robin; where NF1 is not a multiple of NW (the
    // 64 x 128 tile: 18 over 4) waves >= NF1 % NW have one fragment fewer: they send a filler request into a pad, so that every wave
    // counts the same vmcnt
    static constexpr int LPS = (NF1 + NW - 1) / NW;           // LDS-DMA requests per wave and stage
    static constexpr int STAGE = NF1 * 256;                  // floats
    static constexpr int PAD_BYTES = NF1 % NW != 0 ? NW * 1024 : 0;
    static_assert(NSLOT >= 3 && (NSLOT - 1) * LPS <= 63, "vmcnt holds six bits");
    static constexpr size_t LDS_BYTES = (size_t)NSLOT * STAGE * 4 + PAD_BYTES;
    mutable const char* rs[LPS];          // request sources of stage 0, moved to the second A segment when the stages reach it
    mutable bool in_seg1 = false;
    bool is_a[LPS];
    long dseg;
    int s0;
    unsigned ring_lds, lane16;
    int wave;

    // A operand: k-steps [0, s0) from a0, the rest from a1 (both [m-tile][k-step][term] images, m-tile stride a_mt bytes);
    // this workgroup's m-tiles mt0 .. mt0 + FRA - 1 (clamped to mtiles - 1), n-tiles nt0 .. nt0 + FRB - 1 of panel B
    __device__ __forceinline__ void init(float* ring, int wave_, int lane, const char* a0, const char* a1, int s0_, long a_mt, int mt0, int mtiles,
                                         const char* B, int kg_stride, int nt0)
    {
        wave = wave_;
        s0 = s0_;
        lane16 = (unsigned)lane * 16;
        ring_lds = (unsigned)(size_t)(__attribute__((address_space(3))) float*)ring;
        dseg = (a1 - a0) - (long)s0_ * SPLIT_KSTEP_BYTES;
#pragma unroll
        for (int j = 0; j < LPS; ++j) {
            // fragment wave_ + NW j of the stage (past the last one: this wave's filler request repeats it). k0, the k-step inside the stage, is
            // 0; written as a quotient hipcc folds it late and keeps the shipped scalar address arithmetic (as a literal it reassociates
            // the panel offset into a 64-bit multiply chain)
            const int q = min(wave_ + NW * j, NF1 - 1), k0 = q / NF1, f = q - k0 * NF1;
            is_a[j] = f < NT * FRA;
            if (f < NT * FRA) {
                const int m = min(mt0 + f / NT, mtiles - 1);
                rs[j] = a0 + (size_t)m * a_mt + (f % NT) * 1024;
            } else {
                const int g = f - NT * FRA;
                rs[j] = B + ((size_t)(nt0 + g / NT) * kg_stride + k0) * SPLIT_KSTEP_BYTES + (g % NT) * 1024;
            }
        }
    }
    // ---- requests: the source of request J is (wave-uniform base rs[J]) + (lane offset + stage offset, ONE vector add per
    // stage): no scalar address arithmetic per request; no branch either -- past the last stage the requests repeat it into the slot
    // that has just been freed, and a wave without a fragment 4 J + wave refetches its last one into a pad
    __device__ __forceinline__ unsigned stage_voff(int sreq) const
    {
        if (!in_seg1 && sreq >= s0) {
#pragma unroll
            for (int j = 0; j < LPS; ++j)
                if (is_a[j]) rs[j] += dseg;
            in_seg1 = true;
        }
        return lane16 + (unsigned)sreq * SPLIT_KSTEP_BYTES;
    }
    template <int J>
    __device__ __forceinline__ void request3(unsigned voff, unsigned rdst) const
    {
        unsigned dst = rdst + J * (NW * 1024);
        if (NF1 % NW != 0 && J == LPS - 1 && wave >= NF1 % NW) dst = ring_lds + NSLOT * STAGE * 4 + wave * 1024;
        asm volatile("s_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %0, %1" ::"v"(voff), "s"(rs[J]), "s"(dst) : "memory");      // (m0: saved and restored around the run of requests by the caller; hipcc rejects m0 as a clobber -- "reserved register" -- so tests/test_kernel_resources.py holds what the save/restore relies on: no SGPR spill, hence no compiler use of m0, in these kernels)
    }
    template <int J>
    __device__ __forceinline__ void request3_all(unsigned voff, unsigned rdst) const
    {
        if constexpr (J < LPS) { request3<J>(voff, rdst); request3_all<J + 1>(voff, rdst); }
    }
    __device__ __forceinline__ void prologue(int nstages) const
    {
        if (nstages <= 0) return;
        unsigned keep_m0;
        asm volatile("s_mov_b32 %0, m0" : "=s"(keep_m0));
#pragma unroll
        for (int s = 0; s < NSLOT; ++s) {
            const unsigned voff = stage_voff(min(s, nstages - 1));
            request3_all<0>(voff, __builtin_amdgcn_readfirstlane(ring_lds + (s * STAGE + wave * 256) * 4));
        }
        asm volatile("s_mov_b32 m0, %0" ::"s"(keep_m0));
    }

    // The K loop holds a stage's fragments DOUBLE-BUFFERED IN REGISTERS. With one wave per SIMD (one workgroup per CU: the 128 x 96 dense
    // tile, the 128 x 128 cell tile) nothing else issues while a wave waits, so a loop that takes one stage at a time pays per k-step, one
    // after the other: the barrier, the requests, the LDS latency of the first fragments, then the MFMAs (dense(6032, 6032), 512 sites:
    // 1,080 cycles per k-step WITHOUT any operand traffic, for 576 of MFMA). Here iteration st holds stage st in registers; it waits until
    // stage st + 1 has landed, passes the barrier (everybody's share of st + 1 has landed, everybody has READ stage st: its slot is free),
    // requests stage st + NSLOT into that slot and then issues the LDS reads of stage st + 1 BETWEEN the MFMAs of stage st -- the interleave
    // is pinned instruction by instruction (sched_barrier); hipcc's own schedule reads a fragment, waits for it and issues its MFMA, one
    // after the other, in 20 registers: every LDS latency is exposed. NSLOT stages are requested ahead.
    // The MFMAs of one accumulator are issued in mfma3_lo / mfma3_hi order: bit-identical to a plain loop over the k-steps.
    typedef float4 Frag[MTW + NTW][NT];
    __device__ __forceinline__ void read_frags(const float* fa0, const float* fb0, int slot, Frag& f) const
    {
        const float* fa = fa0 + slot * STAGE;
        const float* fb = fb0 + slot * STAGE;
#pragma unroll
        for (int i = 0; i < MTW; ++i)
#pragma unroll
            for (int p = 0; p < NT; ++p) f[i][p] = *reinterpret_cast<const float4*>(fa + (i * NT + p) * 256);
#pragma unroll
        for (int j = 0; j < NTW; ++j)
#pragma unroll
            for (int p = 0; p < NT; ++p) f[MTW + j][p] = *reinterpret_cast<const float4*>(fb + (j * NT + p) * 256);
    }
    static constexpr int req_pos(int j)        // request j of a stage goes behind MFMA (j NM) / LPS + 1 of the pinned sequence
    {
        const int nm = NP * MTW * NTW, p = (j * nm + LPS - 1) / LPS + 1;
        return p < nm ? p : nm - 1;
    }
    template <int M, int J>
    __device__ __forceinline__ void piped_req(unsigned voff, unsigned rdst) const
    {
        if constexpr (J < LPS) {
            if constexpr (req_pos(J) == M) request3<J>(voff, rdst);
            piped_req<M, J + 1>(voff, rdst);
        }
    }
    static constexpr bool ROLL = MTW >= 3;
    // LDS reads of the next stage behind one MFMA of the pinned sequence: one, except where a stage has more term fragments than MFMAs
    // (two fp16 terms on the 64 x 64 tile: four fragments, three MFMAs)
    static constexpr int RPM = ROLL ? 1 : (NT * (MTW + NTW) + NP * MTW * NTW - 1) / (NP * MTW * NTW);
    static constexpr int read_frag(int m)
    {
        if (!ROLL) return m < NT * (MTW + NTW) ? m : -1;
        // the weight fragments and the LAST m-tile's activations first (that m-tile's MFMAs close the sequence), then m-tile i's
        // activations behind its last MFMA
        if (m < NT * NTW) return (MTW + m / NT) * NT + m % NT;
        if (m < NT * NTW + NT) return (MTW - 1) * NT + (m - NT * NTW);
        for (int i = 0; i + 1 < MTW; ++i) {
            const int base = (i + 1) * NP * NTW;
            if (m >= base && m < base + NT) return i * NT + (m - base);
        }
        return -1;
    }
    static_assert(!ROLL || NT * NTW + NT <= NP * NTW, "the early reads end before the first m-tile's MFMAs do");
    template <int RF>
    __device__ __forceinline__ void piped_read(const float* fa, const float* fb, Frag& nxt) const
    {
        if constexpr (RF >= 0) {
            constexpr int F_ = RF / NT, TERM = RF % NT;
            nxt[F_][TERM] = *reinterpret_cast<const float4*>((F_ < MTW ? fa + (F_ * NT + TERM) * 256 : fb + ((F_ - MTW) * NT + TERM) * 256));
        }
    }
    // element M of the pinned sequence
    template <int M>
    __device__ __forceinline__ void piped_seq(unsigned voff, unsigned rdst, const float* fa, const float* fb, const Frag& cur, Frag& nxt,
                                              floatx16 (&acc)[MTW][NTW]) const
    {
        constexpr int NT_ = MTW * NTW, NM = NP * NT_;
        if constexpr (M < NM) {
            // small tiles: product-major (every MFMA of a round goes to another accumulator). Tiles of three and more m-tiles per wave:
            // m-tile-major, so that an activation fragment is dead after its 6 NTW MFMAs and the next stage's copy can take its
            // registers (both stages' fragments live at once are 168 registers beside 192 of accumulators: hipcc spilled inside the loop)
            constexpr int P = ROLL ? (M % (NP * NTW)) / NTW : M / NT_, I = ROLL ? M / (NP * NTW) : (M % NT_) / NTW, J = M % NTW;
            // products in the format's lo / hi order (three bf16 terms: (w2, a0) (w0, a2) (w1, a1) | (w1, a0) (w0, a1) (w0, a0))
            constexpr int WI = F::wi(P), AI = F::ai(P);
            acc[I][J] = F::mfma(cur[MTW + J][WI], cur[I][AI], acc[I][J]);
            // NT fragment + term of the next stage's LDS read(s) behind this MFMA, or -1
            piped_read<read_frag(M * RPM)>(fa, fb, nxt);
            if constexpr (RPM > 1) piped_read<read_frag(M * RPM + 1)>(fa, fb, nxt);
            static_assert(RPM <= 2, "at most two reads behind one MFMA");
            piped_req<M, 0>(voff, rdst);
            __builtin_amdgcn_sched_barrier(0);
            piped_seq<M + 1>(voff, rdst, fa, fb, cur, nxt, acc);
        }
    }
    // one iteration: registers `cur` hold stage st (slot = its ring slot), `nxt` take stage st + 1
    __device__ __forceinline__ void piped(int st, int slot, int nstages, const float* fa0, const float* fb0, const Frag& cur, Frag& nxt, floatx16 (&acc)[MTW][NTW]) const
    {
        asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)" ::"n"((NSLOT - 2) * LPS) : "memory");
        __builtin_amdgcn_s_barrier();
        // the order is pinned instruction by instruction: MFMA m (round robin over the accumulators, the six products of one accumulator
        // in mfma3_lo / mfma3_hi order), behind it LDS read m of the next stage, and every NM / LPS MFMAs one LDS-DMA request. In one
        // burst behind the barrier the four waves' 21 requests held every wave for 350 cycles per k-step in front of its MFMAs
        // (s_memtime: wait 150, barrier 20 - 50, requests 350, reads + MFMAs 600 of 1,150)
        const unsigned voff = stage_voff(min(st + NSLOT, nstages - 1));
        const unsigned rdst = __builtin_amdgcn_readfirstlane(ring_lds + (slot * STAGE + wave * 256) * 4);
        const int nslot = slot + 1 == NSLOT ? 0 : slot + 1;
        const float* fa = fa0 + nslot * STAGE;
        const float* fb = fb0 + nslot * STAGE;
        unsigned keep_m0;
        asm volatile("s_mov_b32 %0, m0" : "=s"(keep_m0));
        __builtin_amdgcn_sched_barrier(0);
        piped_seq<0>(voff, rdst, fa, fb, cur, nxt, acc);
        asm volatile("s_mov_b32 m0, %0" ::"s"(keep_m0));
        __builtin_amdgcn_sched_barrier(0);      // (the next iteration's lgkmcnt(0) stays behind this iteration's last MFMAs)
    }
    __device__ __forceinline__ void run(int nstages, const float* fa0, const float* fb0, floatx16 (&acc)[MTW][NTW]) const
    {
        if (nstages <= 0) return;
        // (prologue() has requested stages 0 .. NSLOT - 1)
        asm volatile("s_waitcnt vmcnt(%0)" ::"n"((NSLOT - 1) * LPS) : "memory");
        __builtin_amdgcn_s_barrier();
        Frag f0, f1;
        read_frags(fa0, fb0, 0, f0);
        int slot = 0, st = 0;
        // every stage through the same pinned sequence, two per trip (the register sets swap roles) -- the last one reads a "next stage"
        // nobody uses: a separate tail of plain MFMAs made hipcc keep the 256 x 192 tile's accumulators in two places and spill inside the loop
        for (int p = 0; p < (nstages >> 1); ++p) {
            piped(st, slot, nstages, fa0, fb0, f0, f1, acc);
            ++st; slot = slot + 1 == NSLOT ? 0 : slot + 1;
            piped(st, slot, nstages, fa0, fb0, f1, f0, acc);
            ++st; slot = slot + 1 == NSLOT ? 0 : slot + 1;
        }
        if (nstages & 1) piped(st, slot, nstages, fa0, fb0, f0, f1, acc);
        asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");      // (the filler requests and reads of the last iterations)
    }
};

// Workgroup tile = (32 WM MTW) rows x (32 WN NTW) columns; the launcher picks it by forward size.
template <int MTW, int NTW, int WM, int WN, class F = TermsBf3>
struct DenseRing {           // (the 256 x 192 tile's stage is 42 KiB: three slots)
    typedef SplitRing<MTW, NTW, WM, WN, (MTW * NTW > 4 ? 3 : DS_SPLIT_DENSE_SLOTS), F> R;
};

// ---- the kernels, once per term format: ds_split_kernels.inc holds every __global__ function of this file and is compiled twice, with
// DS_TF = the format and DS_TK(stem) = the kernel's name in it. (One template body behind two thin __global__ wrappers keeps neither the
// names nor the device code of the three-term kernels: hipcc orders the inlined body's instructions differently and allocates other
// registers. Recorded profiles and the resource tests key on the names; tools/compare_device_asm.py holds the code.)
#define DS_TF TermsBf3
#define DS_TK(stem) stem##_split_kernel
#define DS_TK_XPROJ lstm_xproj_kernel
#include "ds_split_kernels.inc"
#undef DS_TF
#undef DS_TK
#undef DS_TK_XPROJ
#define DS_TF TermsHf2
#define DS_TK(stem) stem##_fp16x2_kernel
#define DS_TK_XPROJ lstm_xproj_fp16x2_kernel
#include "ds_split_kernels.inc"
#undef DS_TF
#undef DS_TK
#undef DS_TK_XPROJ

hipError_t launch_stem23_split(TermFormat fmt, const Stem23Args& a, hipStream_t s)
{
    if (a.n_sites <= 0) return hipSuccess;
    // (the planner sizes the tile by the three-term rows for either format: tile shapes stay as shipped)
    if (a.spt * a.W > 96 || stem23_split_lds_bytes(a.W, a.spt) > 160 * 1024) return hipErrorInvalidValue;
    const int grid = (a.n_sites + a.spt - 1) / a.spt;
    if (fmt == TERMS_FP16X2) hipLaunchKernelGGL(stem23_fp16x2_kernel, dim3(grid), dim3(512), Stem23Rows<TermsHf2>::lds_bytes(a.W, a.spt), s, a);
    else hipLaunchKernelGGL(stem23_split_kernel, dim3(grid), dim3(512), stem23_split_lds_bytes(a.W, a.spt), s, a);
    return hipGetLastError();
}

hipError_t launch_lstm_xproj(TermFormat fmt, const LstmXproj& X, hipStream_t s)
{
    if (X.n <= 0 || X.mtiles <= 0) return hipSuccess;
    if (fmt == TERMS_FP16X2) hipLaunchKernelGGL(lstm_xproj_fp16x2_kernel, dim3(X.mtiles * 8, X.nsteps, 2), dim3(256), 0, s, X);
    else hipLaunchKernelGGL(lstm_xproj_kernel, dim3(X.mtiles * 8, X.nsteps, 2), dim3(256), 0, s, X);
    return hipGetLastError();
}

hipError_t launch_lstm_cells_split(LstmTile tile, TermFormat fmt, const LstmLaunch& L, hipStream_t s)
{
    if (L.ncell <= 0 || L.mtiles <= 0) return hipSuccess;
    const dim3 grid(L.ncell * lstm_tiles_per_cell(tile, L.mtiles));
    if (fmt == TERMS_FP16X2) {
        switch (tile) {
        case LT_S11: hipLaunchKernelGGL((lstm_cell_fp16x2_kernel<1, 1>), grid, dim3(256), (SplitRing<1, 1, 2, 2, DS_SPLIT_LSTM_SLOTS, TermsHf2>::LDS_BYTES), s, L); break;
        case LT_S12: hipLaunchKernelGGL((lstm_cell_fp16x2_kernel<1, 2>), grid, dim3(256), (SplitRing<1, 2, 2, 2, DS_SPLIT_LSTM_SLOTS, TermsHf2>::LDS_BYTES), s, L); break;
        case LT_S22: hipLaunchKernelGGL((lstm_cell_fp16x2_kernel<2, 2>), grid, dim3(256), (SplitRing<2, 2, 2, 2, DS_SPLIT_LSTM_SLOTS, TermsHf2>::LDS_BYTES), s, L); break;
        case LT_S28: hipLaunchKernelGGL((lstm_cell_fp16x2_kernel<1, 2, 4, 2>), grid, dim3(512), (SplitRing<1, 2, 4, 2, DS_SPLIT_LSTM_SLOTS, TermsHf2>::LDS_BYTES), s, L); break;
        default: return hipErrorInvalidValue;
        }
        return hipGetLastError();
    }
    switch (tile) {
    case LT_S11: hipLaunchKernelGGL((lstm_cell_split_kernel<1, 1>), grid, dim3(256), (SplitRing<1, 1, 2, 2, DS_SPLIT_LSTM_SLOTS>::LDS_BYTES), s, L); break;
    case LT_S12: hipLaunchKernelGGL((lstm_cell_split_kernel<1, 2>), grid, dim3(256), (SplitRing<1, 2, 2, 2, DS_SPLIT_LSTM_SLOTS>::LDS_BYTES), s, L); break;
    case LT_S22: hipLaunchKernelGGL((lstm_cell_split_kernel<2, 2>), grid, dim3(256), (SplitRing<2, 2, 2, 2, DS_SPLIT_LSTM_SLOTS>::LDS_BYTES), s, L); break;
    // the same 128 x 128 workgroup tile by EIGHT waves (4 x 2, each 32 x 64): two waves per SIMD of the one workgroup a CU holds
    case LT_S28: hipLaunchKernelGGL((lstm_cell_split_kernel<1, 2, 4, 2>), grid, dim3(512), (SplitRing<1, 2, 4, 2, DS_SPLIT_LSTM_SLOTS>::LDS_BYTES), s, L); break;
    case LT_F1: case LT_F4: case LT_LDS1: case LT_LDS2: case LT_B11: case LT_B12: case LT_B22: case LT_COUNT:
        return hipErrorInvalidValue;      // launch_lstm_cells' (ds_kernels.hip)
    }
    return hipGetLastError();
}

hipError_t launch_dense_split(TermFormat fmt, const SplitDense& d, hipStream_t s)
{
    if (d.n <= 0) return hipSuccess;
    if (d.ksteps <= 0 || (d.N & 3) || d.ntiles_alloc < 4) return hipErrorInvalidValue;
    if (d.splits < 1 || d.splits > d.ksteps || (!d.wide && d.splits != 1)) return hipErrorInvalidValue;
    const long total = (long)d.mtiles * 32 * d.ksteps * 2;
    if (fmt == TERMS_FP16X2) {
        // the same two tiles on two fp16 terms (2 KiB per k-step and fragment row)
        hipLaunchKernelGGL(pack_joint_fp16x2_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, d);
        if (d.wide) {
            typedef DenseRing<4, 3, 2, 2, TermsHf2>::R R;
            if (d.ntiles_alloc < R::FRB) return hipErrorInvalidValue;
            const int mblocks = (d.mtiles + R::FRA - 1) / R::FRA, nblocks = (d.ntiles + R::FRB - 1) / R::FRB;
            hipLaunchKernelGGL((dense_fp16x2_kernel<4, 3, 2, 2>), dim3(mblocks * nblocks * d.splits), dim3(256), R::LDS_BYTES, s, d);
        } else {
            typedef DenseRing<1, 3, 4, 1, TermsHf2>::R R;
            const int mblocks = (d.mtiles + R::FRA - 1) / R::FRA, nblocks = (d.ntiles + R::FRB - 1) / R::FRB;
            hipLaunchKernelGGL((dense_fp16x2_kernel<1, 3, 4, 1>), dim3(mblocks * nblocks), dim3(256), R::LDS_BYTES, s, d);
        }
        return hipGetLastError();
    }
    hipLaunchKernelGGL(pack_joint_split_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, d);
    if (d.wide) {
        // 256 x 192 (waves 2 x 2, each 128 x 96), K in d.splits ranges: half the operand bytes per MFMA of the 128 x 96 tile; the partial
        // products go to d.C + range * d.part_stride and their reader adds them up (launch_head)
        typedef DenseRing<4, 3, 2, 2>::R R;
        if (d.ntiles_alloc < R::FRB) return hipErrorInvalidValue;
        const int mblocks = (d.mtiles + R::FRA - 1) / R::FRA, nblocks = (d.ntiles + R::FRB - 1) / R::FRB;
        hipLaunchKernelGGL((dense_split_kernel<4, 3, 2, 2>), dim3(mblocks * nblocks * d.splits), dim3(256), R::LDS_BYTES, s, d);
    } else {
        // 128 x 96 (waves 4 x 1): 252 workgroups at 512 sites (mid-round's tile; narrow output widths)
        typedef DenseRing<1, 3, 4, 1>::R R;
        const int mblocks = (d.mtiles + R::FRA - 1) / R::FRA, nblocks = (d.ntiles + R::FRB - 1) / R::FRB;
        hipLaunchKernelGGL((dense_split_kernel<1, 3, 4, 1>), dim3(mblocks * nblocks), dim3(256), R::LDS_BYTES, s, d);
    }
    return hipGetLastError();
}

static bool split_chain_ok(const FusedChain& c)
{
    if (c.nmod <= 0 || c.nmod > FUSED_CHAIN_MAX) return false;
    for (int i = 0; i < c.nmod; ++i) {
        if (i > 0 && c.m[i].pool_win != 0) return false;                     // only a chain's first module may pool its input
        if (c.m[i].cin != 240 && c.m[i].cin != 256) return false;            // P1 is unrolled over 15 or 16 chunks (every module of the model)
        if (i > 0 && (c.m[i].W != c.m[0].W || c.m[i].spt != c.m[0].spt || c.m[i].n_sites != c.m[0].n_sites || c.m[i].X != c.m[i - 1].Y))
            return false;
    }
    return true;
}

hipError_t configure_split_kernels()
{
    const void* fns[10] = {(const void*)dense_split_kernel<4, 3, 2, 2>, (const void*)stem23_split_kernel, (const void*)inception_fused_split_kernel<1>, (const void*)inception_fused_split_kernel<2>,
                          (const void*)inception_fused_split_kernel<3>, (const void*)lstm_cell_split_kernel<1, 1>,
                          (const void*)lstm_cell_split_kernel<1, 2>, (const void*)lstm_cell_split_kernel<2, 2>, (const void*)lstm_cell_split_kernel<1, 2, 4, 2>,
                          (const void*)dense_split_kernel<1, 3, 4, 1>};
    for (const void* f : fns) {
        const hipError_t e = hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
        if (e != hipSuccess) return e;
    }
    const void* hfns[10] = {(const void*)dense_fp16x2_kernel<4, 3, 2, 2>, (const void*)stem23_fp16x2_kernel, (const void*)inception_fused_fp16x2_kernel<1>,
                           (const void*)inception_fused_fp16x2_kernel<2>, (const void*)inception_fused_fp16x2_kernel<3>, (const void*)lstm_cell_fp16x2_kernel<1, 1>,
                           (const void*)lstm_cell_fp16x2_kernel<1, 2>, (const void*)lstm_cell_fp16x2_kernel<2, 2>, (const void*)lstm_cell_fp16x2_kernel<1, 2, 4, 2>,
                           (const void*)dense_fp16x2_kernel<1, 3, 4, 1>};
    for (const void* f : hfns) {
        const hipError_t e = hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

hipError_t launch_inception_fused_split(TermFormat fmt, int tm, const FusedChain& c, hipStream_t s)
{
    if (!split_chain_ok(c)) return hipErrorInvalidValue;
    const FusedArgs& a = c.m[0];
    if (a.n_sites <= 0) return hipSuccess;
    const size_t lds = inception_fused_split_lds_bytes(tm, a.W, a.spt);       // (the planner's bound, for either format)
    if (lds > 160 * 1024) return hipErrorInvalidValue;
    const int grid = (a.n_sites + a.spt - 1) / a.spt;
    if (fmt == TERMS_FP16X2) {
        const size_t hl = ChainRows<TermsHf2>::lds_bytes(tm, a.W, a.spt);
        switch (tm) {
        case 1: hipLaunchKernelGGL(inception_fused_fp16x2_kernel<1>, dim3(grid), dim3(512), hl, s, c); break;
        case 2: hipLaunchKernelGGL(inception_fused_fp16x2_kernel<2>, dim3(grid), dim3(512), hl, s, c); break;
        case 3: hipLaunchKernelGGL(inception_fused_fp16x2_kernel<3>, dim3(grid), dim3(512), hl, s, c); break;
        default: return hipErrorInvalidValue;
        }
        return hipGetLastError();
    }
    switch (tm) {
    case 1: hipLaunchKernelGGL(inception_fused_split_kernel<1>, dim3(grid), dim3(512), lds, s, c); break;
    case 2: hipLaunchKernelGGL(inception_fused_split_kernel<2>, dim3(grid), dim3(512), lds, s, c); break;
    case 3: hipLaunchKernelGGL(inception_fused_split_kernel<3>, dim3(grid), dim3(512), lds, s, c); break;
    default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

}  // namespace ds
