// ds_split_kernels.inc -- the split-operand kernels of ds_split.hip, written once and compiled once per term format. NOT a translation
// unit: ds_split.hip includes it with
//     DS_TF          the term format (TermsBf3: three bf16 terms, six products per MAC | TermsHf2: two fp16 terms, three products)
//     DS_TK(stem)    the kernel's name in that format (stem##_split_kernel | stem##_fp16x2_kernel), DS_TK_XPROJ likewise
// and everything a body needs by format -- term count, row strides, the split, the products and their order -- comes from F = DS_TF.

// ---- fused inception modules (layout and phases: the comment above ChainRows in ds_split.hip)
template <int TM>
__global__ __launch_bounds__(512, 2) void DS_TK(inception_fused)(const FusedChain c)
{
    using F = DS_TF;
    constexpr int NT = F::NT, S_LDP = ChainRows<F>::LDP, S_LD1 = ChainRows<F>::LD1, S_LD2 = ChainRows<F>::LD2;
    constexpr int TR32 = TM * 32;
    extern __shared__ __attribute__((aligned(16))) float smem[];
    char* const sm = reinterpret_cast<char*>(smem);
    char* const Pst = sm;                                // [2][TR32][S_LDP] staged chunks
    char* const Ys = sm;                                 // [TR32][S_LDY] b1|b2 output tile, aliases the staged chunks once P1 is done
    char* const T2 = sm + TR32 * ChainRows<F>::LD0;      // [TR32][S_LD2]
    char* const Raw = T2;                                // [2][TR32][S_LDR] raw fp32 chunks during P1 (T2 is written in P2a)
    char* const T1 = T2 + TR32 * S_LD2;                  // [spt*(W+4)+5][S_LD1] (5 spare rows: a dump row for padding rows + its halo)
    const int W = c.m[0].W, spt = c.m[0].spt;            // the same for every module of a chain (ds_internal.h FusedChain)
    int* const rowmap = reinterpret_cast<int*>(T1 + (spt * (W + 4) + 5) * S_LD1);      // [TR32] tile row -> T1 row
    float* const Bs = reinterpret_cast<float*>(rowmap + TR32);                         // [3][64] biases of b5b | b3b | b4b
    const int site0 = blockIdx.x * spt;
    const int nhere = min(spt, c.m[0].n_sites - site0);
    const int TRv = nhere * W;                           // valid rows of this tile
    const size_t grow0 = (size_t)site0 * W;
    auto lds_barrier = []() __attribute__((always_inline)) { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); };
    // once per workgroup: T1 zeroed (every module rewrites the interior rows completely and never touches the halos) and the
    // tile's row map
    for (int i = threadIdx.x; i < (spt * (W + 4) + 5) * (S_LD1 / 16); i += 512)
        reinterpret_cast<float4*>(T1)[i] = make_float4(0.f, 0.f, 0.f, 0.f);
    if (threadIdx.x < TR32)   // rows past the tile's last site map to the dump row, so LDS writes need no predicate
        rowmap[threadIdx.x] = (int)threadIdx.x < TRv ? ((int)threadIdx.x / W) * (W + 4) + 2 + (int)threadIdx.x % W : spt * (W + 4) + 2;

    for (int mi = 0; mi < c.nmod; ++mi) {
    const FusedArgs& a = c.m[mi];
    // every per-lane quantity derives from this opaque copy of the thread index (hipcc otherwise hoists loop-invariant per-lane
    // addresses out of the module loop and holds them in registers for the whole kernel)
    int tid_opaque = threadIdx.x, wave_opaque = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    asm volatile("" : "+v"(tid_opaque), "+s"(wave_opaque));
    const int tid = tid_opaque, lane = tid & 63, wave = wave_opaque;
    const int cin = a.cin;
    const gptr1w Yg = (gptr1w)(a.Y + grow0 * 240);     // wave-uniform base; per-lane offsets stay 32-bit
    const bool stamp = a.dbg != nullptr && lane == 0 && (wave == DS_SPLIT_SW0 || wave == DS_SPLIT_SW1) && blockIdx.x < DBG_MAX_WGS;
#define DS_STAMP(i) do { if (stamp) (a.dbg + ((size_t)blockIdx.x * 2 + (wave == DS_SPLIT_SW1)) * 8)[i] = __builtin_amdgcn_s_memtime(); } while (0)
    DS_STAMP(0);
    if (tid >= 256 && tid < 448) {
        const int q = tid - 256;
        Bs[q] = gload((q < 64 ? a.bias5b : q < 128 ? a.bias3b : a.bias4b) + (q & 63));
    }

    // ---- P1 staging cursor: thread -> (row, 16-byte slot of the chunk's 64 B); rows past the tile end re-read row TRv-1
    // waves 0 .. 2 TM - 1 stage TR32 x 4 sixteen-byte slots, four lanes a row (a row's 64 B of a chunk are one contiguous request).
    // (Sixteen consecutive lanes on sixteen rows at one slot makes the 8-byte term writes and the raw copy's accesses tile the LDS
    // banks exactly -- SQ_LDS_BANK_CONFLICT is 36 % of the kernel's LDS-active cycles with this mapping -- but scatters every
    // row load over sixteen lines per sixteen lanes: measured 373 against 345 us per step. The conflicts are the cheaper evil.)
    const int sr = tid >> 2, sq = tid & 3;
    const int rr = sr < TRv ? sr : TRv - 1;
    const int wr = rr % W;
    // plain input: one row per staged row. Pooled input (the module right after maxpool_layer2 / 3, layers.py:211-213,224-226): the
    // staged row (site s, w) is the max of the input rows 2 w - pad + {0, 1, 2} of site s that exist (padded taps ignored), taken
    // while loading -- the stride-2 pool costs no launch and no buffer, as in the fp32 kernel
    const bool pooled_in = a.pool_win > 0;        // wave-uniform per module
    const float* pc;
    int oq = 0, orr = 0;                          // float offsets of the second / third tap from the first (0 = the same row again)
    if (!pooled_in) {
        pc = a.X + (grow0 + rr) * cin + sq * 4;
    } else {
        const int s_ = rr / W;
        const int i0 = 2 * wr - a.pool_pad;
        const int ia = i0 < 0 ? i0 + 1 : i0;                               // first existing tap
        const int ib = i0 + 1 < a.pool_win ? (i0 + 1 < 0 ? ia : i0 + 1) : ia;
        const int ic = i0 + 2 < a.pool_win ? i0 + 2 : ib;
        pc = a.X + ((size_t)(site0 + s_) * a.pool_win + ia) * cin + sq * 4;
        oq = (ib - ia) * cin; orr = (ic - ia) * cin;
    }
    const int om = wr > 0 ? -S_LDR : 0;           // previous / next row of the same site in the raw LDS copy, or the own row at a site edge
    const int op = wr < W - 1 ? S_LDR : 0;
    // this wave's P1 weights: n-tile `wave`, 16 k-steps x 3 terms of 1 KiB (K padded to 256 in the pack)
    const float* bp = a.Bp1 + ((size_t)wave * 16 * NT * 64 + lane) * 4;

    const int h4 = 4 * (lane >> 5), rlane = lane & 31;
    floatx16 acc[TM];
    {
        float4 bv[4];
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            bv[g] = gload4(a.bias1 + wave * 32 + 8 * g + h4);                  // bias1 is zero-padded to 256
            if (wave < 2) {                                                     // b5 stem columns also carry the tail's BN shift
                const float4 t = gload4(a.bias5c + wave * 32 + 8 * g + h4);     // (zero-padded to 64)
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

    const int nchunks = cin / KC;      // 15 or 16
    __builtin_assume(nchunks >= 15 && nchunks <= 16);
    // The staging waves (the first 2 TM: one 16-byte slot per thread) and the others run two instantiations of the loop, so that
    // inside either no vector-memory instruction sits under a per-thread condition: hipcc counts s_waitcnt vmcnt conservatively
    // across such a branch (as if the loads had not been issued), which made every step wait for the row loads it had just
    // requested -- 46 k cycles of P1 instead of ~20 k.
    auto run_p1 = [&](auto role_tag) __attribute__((always_inline)) {
        // ROLE 1: a staging wave (waves 0 .. 2 TM - 1: TR32 x 4 sixteen-byte slots, one per thread). ROLE 0: the others.
        // A CU's vector-memory path delivers ~32 B/clk (DESIGN.md 4) and a step has 1,152 cycles of MFMA: the 24 KB of weight
        // fragments per step already take two thirds of that, so a chunk's rows are loaded from global memory ONCE (6 KB) -- the
        // two neighbour rows branch 1's pool needs come out of a raw fp32 copy of the chunk in LDS (Raw, which lives in T2's
        // region: T2 is not in use during P1). Chunk k: requested at step k - VD, raw copy written at step k - 2, transformed
        // (3-tap max, terms) at step k - 1 into the staged buffer, consumed by the MFMAs of step k; every hand-over crosses one of
        // the per-step barriers.
        constexpr int ROLE = decltype(role_tag)::value;
        constexpr bool STG = ROLE != 0;
        constexpr int VD = DS_SPLIT_VD;
        constexpr int BD = DS_SPLIT_BD;
        float4 vo[VD];                      // the stager's 16 B of its row, chunks in flight
        float4 bq[BD][NT];
        float4 af[2][NT][TM];
        // waves 6, 7 (branch 1) read the pooled half of a staged row
        const char* const fsrc = Pst + rlane * S_LDP + (lane >> 5) * 16 + (wave >= 6 ? NT * 32 : 0);
        char* const sdst = Pst + sr * S_LDP + sq * 8;
        char* const rdst = Raw + sr * S_LDR + sq * 16;
        auto load_a = [&](int V) __attribute__((always_inline)) {
            if (STG) {
                vo[V] = gload4(pc);
                if (pooled_in) vo[V] = f4max_relu(f4max_relu(vo[V], gload4(pc + oq)), gload4(pc + orr));      // wave-uniform branch
                pc += KC;
            }
        };
        auto raw_a = [&](int X, int V) __attribute__((always_inline)) {
            if (STG) *reinterpret_cast<float4*>(rdst + X * TR32 * S_LDR) = vo[V];
        };
        auto store_a = [&](int X) __attribute__((always_inline)) {
            if (STG) {
                const char* r = rdst + X * TR32 * S_LDR;
                const float4 o = *reinterpret_cast<const float4*>(r);
                const float4 m = *reinterpret_cast<const float4*>(r + om);
                const float4 n = *reinterpret_cast<const float4*>(r + op);
                char* d = sdst + X * TR32 * S_LDP;
                uint2 t[NT];
                F::split4(o.x, o.y, o.z, o.w, t);
                for_terms<NT>([&](auto p) __attribute__((always_inline)) { *reinterpret_cast<uint2*>(d + 32 * p) = t[p]; });
                {
                    const float4 pm = f4max_relu(f4max_relu(o, m), n);
                    F::split4(pm.x, pm.y, pm.z, pm.w, t);
                }
                for_terms<NT>([&](auto p) __attribute__((always_inline)) { *reinterpret_cast<uint2*>(d + NT * 32 + 32 * p) = t[p]; });
            }
        };
        auto load_b = [&](int Bi) __attribute__((always_inline)) {
            for_terms<NT>([&](auto p) __attribute__((always_inline)) { bq[Bi][p] = gload4(bp + 256 * p); });
            bp += 256 * NT;
        };
        auto read_frags = [&](int X) __attribute__((always_inline)) {
#pragma unroll
            for (int mt = 0; mt < TM; ++mt) {
                const char* q = fsrc + X * TR32 * S_LDP + mt * 32 * S_LDP;
#pragma unroll
                for (int p = 0; p < NT; ++p) af[X][p][mt] = *reinterpret_cast<const float4*>(q + 32 * p);
            }
        };
#pragma unroll
        for (int i = 0; i < VD; ++i) load_a(i);                  // chunks 0 .. VD - 1
#pragma unroll
        for (int i = 0; i < BD - 1; ++i) load_b(i);              // weight fragments of chunks 0 .. BD - 2
        raw_a(0, 0);
        raw_a(1, 1 % VD);
        lds_barrier();
        store_a(0);
        lds_barrier();
        read_frags(0);
#pragma unroll
        for (int cc = 0; cc < 16; ++cc) {
            if (cc < nchunks) {                                   // wave-uniform; only cc = 15 is really conditional
                const int X = cc & 1;
                const bool has1 = cc + 1 < nchunks, has2 = cc + 2 < nchunks;
                if (has2) raw_a(X, (cc + 2) % VD);                // the raw copy chunk cc lived in was last read at step cc - 1
                if (cc + VD < nchunks) load_a(cc % VD);           // chunk cc + VD into the register stage chunk cc left two steps ago
                if (cc + BD - 1 < nchunks) load_b((cc + BD - 1) % BD);
                if (has1) store_a(X ^ 1);
#pragma unroll
                for (int mt = 0; mt < TM; ++mt) acc[mt] = F::lo_of(bq[cc % BD], [&](auto p) __attribute__((always_inline)) { return af[X][p][mt]; }, acc[mt]);
                __builtin_amdgcn_sched_barrier(0);
                lds_barrier();
                if (has1) read_frags(X ^ 1);
#pragma unroll
                for (int mt = 0; mt < TM; ++mt) acc[mt] = F::hi_of(bq[cc % BD], [&](auto p) __attribute__((always_inline)) { return af[X][p][mt]; }, acc[mt]);
                if (has1) __builtin_amdgcn_sched_group_barrier(0x100, NT * TM, 0);      // the next chunk's fragment reads lead the half-step
                __builtin_amdgcn_sched_barrier(0);
            }
        }
    };
    if (wave < 2 * TM) run_p1(SplitRole<1>{}); else run_p1(SplitRole<0>{});      // wave-uniform
    DS_STAMP(1);
    lds_barrier();   // all fragment reads of the staging area are done before the output tile aliases it
    DS_STAMP(2);

    // ---- P2 jobs (wave-uniform). A CU's vector-memory path is the scarce resource of this kernel (~32 B/clk against 24 KB of P1
    // weight fragments per 1,152-cycle step), so the second-stage convs are dealt by (conv, n-tile) and a wave takes ITS weight
    // fragments (18 or 30 KiB) through all the m-tiles it owns -- the unit table of inception_fused_kernel, one (conv, m-tile,
    // n-tile) per wave, re-loaded them per m-tile: 420 KB per module and tile against 216 KB here:
    //   waves 0, 1   P2a: b5b (1x3, 32 -> 64), n-tile = wave, all m-tiles -> T2;      P2b: the residual tail on the stem accumulators
    //   waves 2, 3   P2a: b3b (1x3, 32 -> 48), n-tile = wave - 2, all m-tiles
    //   waves 4, 5   P2a: the b1|b2 tile's stores (with waves 6, 7);                   P2b: b4b (1x5, 32 -> 48), n-tile = wave - 4, m-tile 0
    //   waves 6, 7   P2a: the b1|b2 tile's stores;                                     P2b: b4b, n-tile = wave - 6, m-tiles 1 .. TM - 1
    // MFMAs per SIMD and phase at TM = 3: P2a 108 | 108 | 108 | 108, P2b 72 + 60 | 72 + 60 | 120 | 120.
    float4 pf[10 * NT];                              // this wave's unit weights
    // (defined on every path: a register array that is only loaded under a wave-uniform condition is "undefined on some
    // paths", and hipcc keeps such a value live around the whole module loop)
#pragma unroll
    for (int g = 0; g < 10 * NT; ++g) pf[g] = make_float4(0.f, 0.f, 0.f, 0.f);
    // Vector-memory operations retire in issue order (one vmcnt counter for loads and stores) and hipcc counts conservatively
    // across control flow, so a weight fragment requested BEHIND a store is only usable once that store is acknowledged: every
    // wave requests its weights here, in front of all its stores.
    if (wave < 2) fuseds_unit_prefetch<F>(a.Bp5b, 3, wave, lane, pf);
    else if (wave < 4) fuseds_unit_prefetch<F>(a.Bp3b, 3, wave - 2, lane, pf);
    else fuseds_unit_prefetch<F>(a.Bp4b, 5, (wave - 4) & 1, lane, pf);

    // ---- P1 epilogue (bias already inside acc): route the 256 columns. b3a | b4a | b5a go to T1 as terms, b1|b2 through an
    // fp32 LDS tile and leave as whole 384-B row segments; the b5 stem stays in the accumulators of waves 0, 1.
    if (wave >= 3 && wave <= 5) {            // wave-uniform: n-tiles 3,4,5 -> T1, through the row map
#pragma unroll
        for (int mt = 0; mt < TM; ++mt) {
            char* d = T1 + rowmap[mt * 32 + rlane] * S_LD1 + ((wave * 32 - 96) + h4) * 2;
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                uint2 t[NT];
                F::split4(relu_f(acc[mt][4 * g]), relu_f(acc[mt][4 * g + 1]), relu_f(acc[mt][4 * g + 2]), relu_f(acc[mt][4 * g + 3]), t);
#pragma unroll
                for (int p = 0; p < NT; ++p) *reinterpret_cast<uint2*>(d + 16 * g + p * S_T1P) = t[p];
            }
        }
    } else if (wave != 0) {                  // n-tiles 1,2 (b5s tail | b2) and 6,7 (b1 | padding) -> output tile
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const int col = wave * 32 + 8 * g + h4;          // groups of 4 never straddle 48 / 240
            if (col >= 48 && col < 240) {
                const int ycol = col < 96 ? col : col - 192;        // position inside Y[:, 0:96) (b1 first, then b2)
#pragma unroll
                for (int mt = 0; mt < TM; ++mt)
                    *reinterpret_cast<float4*>(Ys + (mt * 32 + rlane) * S_LDY + ycol * 4) =
                        make_float4(relu_f(acc[mt][4 * g]), relu_f(acc[mt][4 * g + 1]), relu_f(acc[mt][4 * g + 2]),
                                    relu_f(acc[mt][4 * g + 3]));
            }
        }
    }
    DS_STAMP(3);
    lds_barrier();   // T1 and the b1|b2 tile complete
    DS_STAMP(4);
    // a job: conv KIND (1 b5b, 2 b3b, 3 b4b) on NM m-tiles from m0, n-tile nt, the weights in pf; the NM accumulator chains are
    // interleaved (a single unit is a chain of dependent LDS reads and MFMAs, i.e. latency)
    auto run_job = [&](auto kind_tag, auto nm_tag, int m0, int nt, const float4 (&wts)[10 * NT]) __attribute__((always_inline)) {
        constexpr int KIND = decltype(kind_tag)::value, NM = decltype(nm_tag)::value;
        if constexpr (NM > 0) {
            floatx16 u[NM];
            const float* bsrc = Bs + (KIND == 1 ? 0 : KIND == 2 ? 64 : 128) + nt * 32 + h4;
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const float4 t = *reinterpret_cast<const float4*>(bsrc + 8 * g);
#pragma unroll
                for (int m = 0; m < NM; ++m) { u[m][4 * g] = t.x; u[m][4 * g + 1] = t.y; u[m][4 * g + 2] = t.z; u[m][4 * g + 3] = t.w; }
            }
            int rm[NM];
#pragma unroll
            for (int m = 0; m < NM; ++m) rm[m] = rowmap[(m0 + m) * 32 + rlane];
            // T1 channels: b3a 0..31, b4a 32..63, b5a 64..95
            fuseds_conv_units<F, KIND == 3 ? 5 : 3, NM>(T1, rm, KIND == 1 ? 128 : KIND == 2 ? 0 : 64, lane, wts, u);
#pragma unroll
            for (int m = 0; m < NM; ++m) {
                const int row = (m0 + m) * 32 + rlane;
                if (KIND == 1) {          // 1x3, 32 -> 64, ReLU, to T2 as terms                  layers.py:127-131
                    char* d = T2 + row * S_LD2 + (nt * 32 + h4) * 2;
#pragma unroll
                    for (int g = 0; g < 4; ++g) {
                        uint2 t[NT];
                        F::split4(relu_f(u[m][4 * g]), relu_f(u[m][4 * g + 1]), relu_f(u[m][4 * g + 2]), relu_f(u[m][4 * g + 3]), t);
                        for_terms<NT>([&](auto p) __attribute__((always_inline)) { *reinterpret_cast<uint2*>(d + 16 * g + p * S_T2P) = t[p]; });
                    }
                } else {
                    // KIND 2: 1x3, 32 -> 48, ReLU, to Y[96,144)   layers.py:106-110
                    // KIND 3: 1x5, 32 -> 48, ReLU, to Y[144,192)  layers.py:115-119
                    const int ybase = KIND == 2 ? 96 : 144;
                    if (row < TRv) {
#pragma unroll
                        for (int g = 0; g < 4; ++g)
                            if (nt * 32 + 8 * g < 48) {      // wave-uniform: 48 output channels = n-tile 0 and half of n-tile 1
                                v4f o = {relu_f(u[m][4 * g]), relu_f(u[m][4 * g + 1]), relu_f(u[m][4 * g + 2]), relu_f(u[m][4 * g + 3])};
                                *(__attribute__((address_space(1))) v4f*)(Yg + (unsigned)(row * 240 + ybase + nt * 32 + 8 * g + h4)) = o;
                            }
                    }
                }
            }
        }
    };

    // ---- P2a | barrier (T2 complete) | P2b, one code path per wave role with the barrier INSIDE the paths (every path passes exactly
    // one): the stem accumulators are then live in the path of waves 0, 1 only and each role's registers are its own (round 5: 250 ->
    // fewer VGPRs, which pays for the second fragment buffer of fuseds_conv_units)
    auto tail_and_store = [&]() __attribute__((always_inline)) {
        // branch 5 tail: 1x1 64 -> 48 (BN, no ReLU) accumulated on top of the stem conv held in acc,
        // then relu(stem + tail)                                                         layers.py:132-138
        const char* const tb = T2 + rlane * S_LD2 + (lane >> 5) * 16;
        float4 fr[2][NT];
#pragma unroll
        for (int p = 0; p < NT; ++p) fr[0][p] = *reinterpret_cast<const float4*>(tb + p * S_T2P);
        int cur = 0;
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            float4 w[NT];
            for_terms<NT>([&](auto p) __attribute__((always_inline)) { w[p] = pf[NT * g + p]; });
#pragma unroll
            for (int mt = 0; mt < TM; ++mt) {
                const int mn = mt + 1 < TM ? mt + 1 : 0, gn = mt + 1 < TM ? g : g + 1;
                if (gn < 4) {      // the next group's fragments, in front of this group's MFMAs
                    const char* q = tb + mn * 32 * S_LD2 + gn * 32;
#pragma unroll
                    for (int p = 0; p < NT; ++p) fr[cur ^ 1][p] = *reinterpret_cast<const float4*>(q + p * S_T2P);
                }
                acc[mt] = F::lo(w, fr[cur], acc[mt]);
                acc[mt] = F::hi(w, fr[cur], acc[mt]);
                cur ^= 1;
                __builtin_amdgcn_sched_barrier(0);
            }
        }
#pragma unroll
        for (int mt = 0; mt < TM; ++mt) {
            const int row = mt * 32 + rlane;
            if (row < TRv) {
#pragma unroll
                for (int g = 0; g < 4; ++g)
                    if (wave * 32 + 8 * g < 48) {
                        v4f o = {relu_f(acc[mt][4 * g]), relu_f(acc[mt][4 * g + 1]), relu_f(acc[mt][4 * g + 2]),
                                 relu_f(acc[mt][4 * g + 3])};
                        *(__attribute__((address_space(1))) v4f*)(Yg + (unsigned)(row * 240 + 192 + wave * 32 + 8 * g + h4)) = o;
                    }
            }
        }
    };
    if (wave < 2) {
        run_job(SplitRole<1>{}, SplitRole<TM>{}, 0, wave, pf);
        // the tail's twelve weight fragments travel in the unit registers (behind the job's MFMAs; its results are LDS writes)
#pragma unroll
        for (int g = 0; g < 4 * NT; ++g) pf[g] = gload4(a.Bp5c + ((size_t)(wave * 4 * NT + g) * 64 + lane) * 4);
        DS_STAMP(5);
        lds_barrier();   // T2 complete
        DS_STAMP(6);
        tail_and_store();
    } else if (wave < 4) {
        run_job(SplitRole<2>{}, SplitRole<TM>{}, 0, wave - 2, pf);
        lds_barrier();
    } else {
        // the b1|b2 tile leaves as whole 384-byte row segments, by the four waves whose second-stage job waits for P2b; every
        // thread issues the same number of stores (slots past the tile's last one repeat it)
        constexpr int NFL = (TR32 * 24 + 255) / 256;
        const int last = TRv * 24 - 1, t4 = tid - 256;
#pragma unroll
        for (int i = 0; i < NFL; ++i) {
            const int idx = min(t4 + i * 256, last);
            const int row = idx / 24, q = idx - row * 24;
            const float4 v = *reinterpret_cast<const float4*>(Ys + row * S_LDY + q * 16);
            v4f o = {v.x, v.y, v.z, v.w};
            *(__attribute__((address_space(1))) v4f*)(Yg + (unsigned)(row * 240 + q * 4)) = o;
        }
        DS_STAMP(5);
        lds_barrier();
        DS_STAMP(6);
        if (wave >= 6) run_job(SplitRole<3>{}, SplitRole<TM - 1>{}, 1, wave - 6, pf);
        else run_job(SplitRole<3>{}, SplitRole<1>{}, 0, wave - 4, pf);
    }
    DS_STAMP(7);
#undef DS_STAMP
    // the next module reads the rows this one has stored (other waves' stores included: __syncthreads drains vmcnt) and
    // re-uses every LDS region
    if (mi + 1 < c.nmod) __syncthreads();
    }   // modules of the chain
}

// ---- conv_layer2 + conv_layer3 (the comment above Stem23Rows in ds_split.hip)
__global__ __launch_bounds__(512, 2) void DS_TK(stem23)(const Stem23Args a)
{
    using F = DS_TF;
    constexpr int NT = F::NT, S23_SX = Stem23Rows<F>::SX, S23_ST = Stem23Rows<F>::ST;
    extern __shared__ __attribute__((aligned(16))) float smem[];
    char* const Xs = reinterpret_cast<char*>(smem);                  // [96][S23_SX]
    char* const T = Xs + 96 * S23_SX;                               // [spt * (W + 2) + 3][S23_ST]
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int W = a.W, spt = a.spt;
    const int trows = spt * (W + 2) + 3;                            // last three rows: halo | dump row (padding rows of the tile) | halo
    int* const rowmap = reinterpret_cast<int*>(T + trows * S23_ST);
    const int site0 = blockIdx.x * spt;
    const int nhere = min(spt, a.n_sites - site0);
    const int TRv = nhere * W;
    const size_t grow0 = (size_t)site0 * W;
    const int h4 = 4 * (lane >> 5), rlane = lane & 31, hb = (lane >> 5) * 16;
    auto lds_barrier = []() __attribute__((always_inline)) { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); };

    // ---- stage: zero T (halo rows must be zero; the rest is overwritten), row map, input rows as terms
    for (int i = tid; i < trows * (S23_ST / 16); i += 512) reinterpret_cast<float4*>(T)[i] = make_float4(0.f, 0.f, 0.f, 0.f);
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
            uint2 t[NT];
            F::split4(v[i].x, v[i].y, v[i].z, v[i].w, t);
            char* d = Xs + row * S23_SX + q * 8;
#pragma unroll
            for (int p = 0; p < NT; ++p) *reinterpret_cast<uint2*>(d + 128 * p) = t[p];
        }
    }
    // conv3 weights of the first two k-steps and both bias vectors are requested before the barrier
    const float* const b3 = a.Bp3 + ((size_t)wave * 24 * NT * 64 + lane) * 4;       // n-tile `wave`: 24 k-steps x NT terms of 1 KiB
    float4 bq[2][NT];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int p = 0; p < NT; ++p) bq[i][p] = gload4(b3 + (i * NT + p) * 256);
    float4 bias3[4];
#pragma unroll
    for (int g = 0; g < 4; ++g) bias3[g] = gload4(a.bias3 + wave * 32 + 8 * g + h4);
    // conv2: unit u = (m, n); waves 0..3 take (0, w) and (2, w), waves 4..7 take (1, w - 4): three units per SIMD
    const int n2 = wave & 3;
    float4 w2[4 * NT];
#pragma unroll
    for (int g = 0; g < 4 * NT; ++g) w2[g] = gload4(a.Bp2 + ((size_t)(n2 * 4 * NT + g) * 64 + lane) * 4);      // 4 k-steps x NT terms
    float4 bias2[4];
#pragma unroll
    for (int g = 0; g < 4; ++g) bias2[g] = gload4(a.bias2 + n2 * 32 + 8 * g + h4);
    lds_barrier();
    {
        const int nunits = wave < 4 ? 2 : 1;
        for (int ui = 0; ui < nunits; ++ui) {
            const int m = wave < 4 ? 2 * ui : 1;
            floatx16 u;
#pragma unroll
            for (int g = 0; g < 4; ++g) { u[4 * g] = bias2[g].x; u[4 * g + 1] = bias2[g].y; u[4 * g + 2] = bias2[g].z; u[4 * g + 3] = bias2[g].w; }
            const char* xr = Xs + (m * 32 + rlane) * S23_SX + hb;
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                float4 x[NT], w[NT];
#pragma unroll
                for (int p = 0; p < NT; ++p) { x[p] = *reinterpret_cast<const float4*>(xr + 128 * p + g * 32); w[p] = w2[NT * g + p]; }
                u = F::lo(w, x, u);
                u = F::hi(w, x, u);
            }
            const int row = m * 32 + rlane;
            char* const td = T + rowmap[row] * S23_ST + (n2 * 32 + h4) * 2;
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const float4 o = make_float4(relu_f(u[4 * g]), relu_f(u[4 * g + 1]), relu_f(u[4 * g + 2]), relu_f(u[4 * g + 3]));
                uint2 t[NT];
                F::split4(o.x, o.y, o.z, o.w, t);
#pragma unroll
                for (int p = 0; p < NT; ++p) *reinterpret_cast<uint2*>(td + 16 * g + 256 * p) = t[p];
                if (a.C2 && row < TRv) {                       // diagnostic tap (debug mode): conv_layer2's output rows
                    const v4f ov = {o.x, o.y, o.z, o.w};
                    *(__attribute__((address_space(1))) v4f*)(a.C2 + (grow0 + row) * 128 + n2 * 32 + 8 * g + h4) = ov;
                }
            }
        }
    }
    lds_barrier();

    // ---- conv3: 24 k-steps (3 taps x 8) without a barrier: the whole activation tile is resident; weights through a register ring
    // two k-steps deep, activation fragments one k-step ahead
    floatx16 acc[3];
#pragma unroll
    for (int m = 0; m < 3; ++m)
#pragma unroll
        for (int g = 0; g < 4; ++g) { acc[m][4 * g] = bias3[g].x; acc[m][4 * g + 1] = bias3[g].y; acc[m][4 * g + 2] = bias3[g].z; acc[m][4 * g + 3] = bias3[g].w; }
    const char* tb[3];
#pragma unroll
    for (int m = 0; m < 3; ++m) tb[m] = T + (rowmap[m * 32 + rlane] - 1) * S23_ST + hb;     // tap t reads row + t - 1
    float4 af[2][3][NT];
#pragma unroll
    for (int m = 0; m < 3; ++m)
#pragma unroll
        for (int p = 0; p < NT; ++p) af[0][m][p] = *reinterpret_cast<const float4*>(tb[m] + p * 256);
#pragma unroll
    for (int ks = 0; ks < 24; ++ks) {
        const int cur = ks & 1;
        if (ks + 1 < 24) {
            const int t1 = (ks + 1) >> 3, g1 = (ks + 1) & 7;
#pragma unroll
            for (int m = 0; m < 3; ++m)
#pragma unroll
                for (int p = 0; p < NT; ++p) af[cur ^ 1][m][p] = *reinterpret_cast<const float4*>(tb[m] + t1 * S23_ST + g1 * 32 + p * 256);
        }
#pragma unroll
        for (int m = 0; m < 3; ++m) {
            acc[m] = F::lo(bq[cur], af[cur][m], acc[m]);
            acc[m] = F::hi(bq[cur], af[cur][m], acc[m]);
        }
        if (ks + 2 < 24) {
#pragma unroll
            for (int p = 0; p < NT; ++p) bq[cur][p] = gload4(b3 + ((ks + 2) * NT + p) * 256);
        }
        __builtin_amdgcn_sched_barrier(0);       // pins the ring: requests stay two k-steps ahead of their MFMAs
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

// ---- the BiLSTM cells of one wavefront diagonal (layers.py:45-72), split operands: h and the weights in F::NT terms, F::NP
// products per MAC, fp32 accumulate; the layer-0 table row / rank-1 terms, the gates and the cell state are fp32 as in the fp32
// kernel (lstm_acc_init / lstm_gates are shared with it); h is split once, in the epilogue that produces it.
template <int MTW, int NTW, int WM = 2, int WN = 2>
__global__ __launch_bounds__(64 * WM * WN, (SplitRing<MTW, NTW, WM, WN, DS_SPLIT_LSTM_SLOTS, DS_TF>::LDS_BYTES > 80 * 1024) ? 1 : 2) void DS_TK(lstm_cell)(const LstmLaunch L_)
{
    using F = DS_TF;
    const LstmLaunch* const Lp = &L_;
    typedef SplitRing<MTW, NTW, WM, WN, DS_SPLIT_LSTM_SLOTS, F> R;
    constexpr int NT = F::NT, SPLIT_KSTEP_BYTES = R::SPLIT_KSTEP_BYTES, SPLIT_MT_BYTES = R::SPLIT_MT_BYTES;
    extern __shared__ __attribute__((aligned(16))) float ring[];    // [NSLOT * STAGE]
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int mi = wave % WM, nj = wave / WM;
    const int bid = lstm_logical_tile(blockIdx.x, gridDim.x, Lp->cls_tiles[0], Lp->cls_tiles[1]);
    const int mtiles = Lp->mtiles;
    const int mblocks = (mtiles + R::FRA - 1) / R::FRA;
    constexpr int NGROUPS = 32 / R::FRB;
    const int per_cell = mblocks * NGROUPS;
    const int ci = bid / per_cell, rem = bid - ci * per_cell;
    const int ng = rem % NGROUPS, mb = rem / NGROUPS;          // the n-groups of one m-block are neighbours (lstm_cell_bf16_kernel)
    const LstmCell& C = Lp->cell[ci];
    const int half = lane >> 5, r31 = lane & 31;
    const int n = Lp->n, T = Lp->T;
    const unsigned lane4 = (unsigned)lane * 4;
    const bool has_x = C.ax != nullptr, has_h = C.ah != nullptr;
    const int KS = (has_x ? 16 : 0) + (has_h ? 16 : 0);       // k-steps: x rows first, then h rows (TF kernel order)
    R rg;
    rg.init(ring, wave, lane, reinterpret_cast<const char*>(has_x ? C.ax : C.ah), reinterpret_cast<const char*>(has_h ? C.ah : C.ax),
            has_x ? 16 : 0, SPLIT_MT_BYTES, mb * R::FRA, mtiles, reinterpret_cast<const char*>(C.Bp), C.kg_stride, ng * R::FRB);
    rg.prologue(KS);

    int mt[MTW];
    bool valid[MTW];
#pragma unroll
    for (int i = 0; i < MTW; ++i) {
        const int raw = mb * R::FRA + mi * MTW + i;
        valid[i] = raw < mtiles;
        mt[i] = valid[i] ? raw : mtiles - 1;
    }
    floatx16 acc[MTW][NTW];
    float4 cp[MTW][NTW];
    {
        int ntl[NTW], rowc[MTW];
#pragma unroll
        for (int j = 0; j < NTW; ++j) ntl[j] = ng * R::FRB + nj * NTW + j;
#pragma unroll
        for (int i = 0; i < MTW; ++i) rowc[i] = min(mt[i] * 32 + r31, n - 1);
        if (C.xinit) {                                     // wave-uniform: layer 0 behind lstm_xproj_kernel's image (DS_TUNE_LSTM_XPROJ_ALL)
#pragma unroll
            for (int i = 0; i < MTW; ++i)
#pragma unroll
                for (int j = 0; j < NTW; ++j) lstm_acc_load(C.xinit, mt[i], ntl[j], lane4, acc[i][j]);
        } else {
            // (bias and the rank-1 rows on the SCALAR path -- s_load_dwordx8 + selects instead of ~80 L2-hot float4 per lane -- was built and
            // measured in round 6, git 755c1c9: 383 against 373 us per step alone, pipelined +- 0: eight dependent scalar round trips)
#pragma unroll
            for (int i = 0; i < MTW; ++i)
#pragma unroll
                for (int j = 0; j < NTW; ++j) lstm_acc_init(C, ntl[j] * 8 + 4 * half, rowc[i], T, acc[i][j]);
        }
    }
    const bool c_zero = C.c_zero != 0;
#pragma unroll
    for (int i = 0; i < MTW; ++i)
#pragma unroll
        for (int j = 0; j < NTW; ++j) {
            cp[i][j] = make_float4(0.f, 0.f, 0.f, 0.f);
            if (!c_zero) cp[i][j] = gload4(C.c + (size_t)mt[i] * LSTM_MT_FLOATS + (unsigned)(ng * R::FRB + nj * NTW + j) * 256 + lane4);
        }
    // every compiler-visible load is retired here: the loop's vmcnt waits count the LDS-DMA requests only (lstm_cell_bf16_kernel)
#pragma unroll
    for (int i = 0; i < MTW; ++i)
#pragma unroll
        for (int j = 0; j < NTW; ++j) {
            asm volatile("" : "+v"(cp[i][j].x), "+v"(cp[i][j].y), "+v"(cp[i][j].z), "+v"(cp[i][j].w));
            asm volatile("" : "+v"(acc[i][j]));
        }
    rg.run(KS, ring + (mi * MTW * NT) * 256 + lane4, ring + (NT * R::FRA + nj * NTW * NT) * 256 + lane4, acc);

    // ---- gates (fp32), new state; c fragment-major fp32, h fragment-major in three terms (8 bytes per lane and term), optional
    // row-major fp32 h for the joint model
#pragma unroll
    for (int i = 0; i < MTW; ++i) {
        if (!valid[i]) continue;
        const int row = mt[i] * 32 + r31;
#pragma unroll
        for (int j = 0; j < NTW; ++j) {
            const int ntile = ng * R::FRB + nj * NTW + j;
            float4 cn, hn;
            lstm_gates(acc[i][j], cp[i][j], cn, hn);
            const v4f co = {cn.x, cn.y, cn.z, cn.w};
            *(__attribute__((address_space(1))) v4f*)(C.c + (size_t)mt[i] * LSTM_MT_FLOATS + (unsigned)ntile * 256 + lane4) = co;
            uint2 t[NT];
            F::split4(hn.x, hn.y, hn.z, hn.w, t);
            char* const hb = reinterpret_cast<char*>(C.h_out) + (size_t)mt[i] * SPLIT_MT_BYTES + (unsigned)(ntile >> 1) * SPLIT_KSTEP_BYTES +
                             (unsigned)(((ntile & 1) * 32 + r31) * 16 + half * 8);
            typedef unsigned int u2v __attribute__((ext_vector_type(2)));
            for_terms<NT>([&](auto p) __attribute__((always_inline)) { *(__attribute__((address_space(1))) u2v*)(hb + 1024 * p) = u2v{t[p].x, t[p].y}; });
            if (C.h_row && row < n) {
                const v4f hr = {hn.x, hn.y, hn.z, hn.w};
                *(__attribute__((address_space(1))) v4f*)(C.h_row + (size_t)row * 256 + ntile * 8 + 4 * half) = hr;
            }
        }
    }
}

// ---- layer 0's accumulator-initial values for every step of both directions, and the first step's cells (ds_internal.h LstmXproj).
// One wave = one 32-site x 8-unit tile of one (direction, step): lstm_acc_init's arithmetic (the bits a cell would compute itself),
// stored as the four 1 KiB fragments lstm_acc_load reads back; step 0 (h = 0, c = 0: no matrix product) goes through the gates here
// and leaves c and the split h image exactly as lstm_cell_split_kernel's epilogue does.
__global__ __launch_bounds__(256) void DS_TK_XPROJ(const LstmXproj X)
{
    using F = DS_TF;
    constexpr int NT = F::NT, SPLIT_KSTEP_BYTES = NT * 1024, SPLIT_MT_BYTES = 16 * SPLIT_KSTEP_BYTES;
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int dir = blockIdx.z, sidx = blockIdx.y;
    const int mtile = blockIdx.x >> 3, ntile = (blockIdx.x & 7) * 4 + wave;
    const int half = lane >> 5, r31 = lane & 31;
    const unsigned lane4 = (unsigned)lane * 4;
    const int t = dir == 0 ? sidx : X.T - 1 - sidx;
    LstmCell C = X.cell[dir];
    C.t = t;
    const int row = mtile * 32 + r31;
    floatx16 acc;
    lstm_acc_init(C, ntile * 8 + 4 * half, row < X.n ? row : X.n - 1, X.T, acc);
    if (sidx > 0) {
        float* const p = X.xinit[dir] + (size_t)t * X.x_step + ((size_t)(mtile * 32 + ntile) * 4) * 256 + lane4;
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const v4f o = {acc[4 * g], acc[4 * g + 1], acc[4 * g + 2], acc[4 * g + 3]};
            *(__attribute__((address_space(1))) v4f*)(p + g * 256) = o;
        }
        return;
    }
    float4 cn, hn;
    lstm_gates(acc, make_float4(0.f, 0.f, 0.f, 0.f), cn, hn);
    const v4f co = {cn.x, cn.y, cn.z, cn.w};
    *(__attribute__((address_space(1))) v4f*)(C.c + (size_t)mtile * LSTM_MT_FLOATS + (unsigned)ntile * 256 + lane4) = co;
    uint2 tt[NT];
    F::split4(hn.x, hn.y, hn.z, hn.w, tt);
    char* const hb = reinterpret_cast<char*>(C.h_out + (size_t)t * X.h_step) + (size_t)mtile * SPLIT_MT_BYTES + (unsigned)(ntile >> 1) * SPLIT_KSTEP_BYTES +
                     (unsigned)(((ntile & 1) * 32 + r31) * 16 + half * 8);
    typedef unsigned int u2v __attribute__((ext_vector_type(2)));
    for_terms<NT>([&](auto p) __attribute__((always_inline)) { *(__attribute__((address_space(1))) u2v*)(hb + 1024 * p) = u2v{tt[p].x, tt[p].y}; });
}

// ---- dense(J, J) of the joint model (layers.py:257-259: no bias, no activation), split operands. A = the joint rows
// [h_fw(T-1) | h_bw(0) | signal features] as a fragment-major term image (pack_joint_split_kernel), B = W1's panels.
__global__ __launch_bounds__(256) void DS_TK(pack_joint)(const SplitDense d)
{
    using F = DS_TF;
    constexpr int NT = F::NT, SPLIT_KSTEP_BYTES = NT * 1024;
    // one thread per (row, k-step half): 8 consecutive k of one row -> the 16 bytes of its lane slot in each of the three term fragments.
    // A wave = the 64 lane slots of ONE (m-tile, k-step): its three stores are whole 1 KiB fragments (with the k-step half fastest over
    // the threads every store was a lone 16 bytes: 38 MB written for the image's 18.5 MB, PMC)
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    const int ksteps = d.ksteps;
    const long total = (long)d.mtiles * 32 * ksteps * 2;
    if (idx >= total) return;
    const int half = (int)((idx >> 5) & 1);
    const long t = idx >> 6;
    const int ks = (int)(t % ksteps);
    const int row = (int)(t / ksteps) * 32 + (int)(idx & 31);
    const int k0 = ks * 16 + half * 8;
    float v[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) v[e] = 0.0f;
    if (row < d.n) {
        // the joint row's three segments (lengths are multiples of 8)
        const float* p = nullptr;
        int k = k0;
        if (k < d.len[0]) p = d.seg[0] + (size_t)row * d.len[0] + k;
        else if ((k -= d.len[0]) < d.len[1]) p = d.seg[1] + (size_t)row * d.len[1] + k;
        else { k -= d.len[1]; p = d.seg[2] + (size_t)row * d.len[2] + k; }
        const float4 x = gload4(p), y = gload4(p + 4);
        v[0] = x.x; v[1] = x.y; v[2] = x.z; v[3] = x.w; v[4] = y.x; v[5] = y.y; v[6] = y.z; v[7] = y.w;
    }
    uint2 ta[NT], tb[NT];
    F::split4(v[0], v[1], v[2], v[3], ta);
    F::split4(v[4], v[5], v[6], v[7], tb);
    char* dst = d.A + ((size_t)(row >> 5) * ksteps + ks) * SPLIT_KSTEP_BYTES + (size_t)(half * 32 + (row & 31)) * 16;
    for_terms<NT>([&](auto p) __attribute__((always_inline)) { *reinterpret_cast<uint4*>(dst + 1024 * p) = make_uint4(ta[p].x, ta[p].y, tb[p].x, tb[p].y); });
}

template <int MTW, int NTW, int WM, int WN>
__global__ __launch_bounds__(256, (DenseRing<MTW, NTW, WM, WN, DS_TF>::R::LDS_BYTES > 80 * 1024) ? 1 : 2) void DS_TK(dense)(const SplitDense d)
{
    using F = DS_TF;
    typedef typename DenseRing<MTW, NTW, WM, WN, F>::R R;
    constexpr int NT = F::NT, SPLIT_KSTEP_BYTES = R::SPLIT_KSTEP_BYTES;
    extern __shared__ __attribute__((aligned(16))) float ring[];
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int mi = wave % WM, nj = wave / WM;
    const int mblocks = (d.mtiles + R::FRA - 1) / R::FRA;
    const int nblocks = (d.ntiles + R::FRB - 1) / R::FRB;
    const int tiles = mblocks * nblocks, total = tiles * d.splits;      // logical workgroup = (K range, n-block, m-block), m fastest
    // XCD-aware order (workgroup b runs on XCD b % 8): every XCD takes a contiguous run of logical tiles; the m-blocks of one weight
    // panel are neighbours, so a panel streams into one L2 once
    // (workgroup b runs on XCD b % 8; XCD x takes total / 8 tiles, the first total % 8 XCDs one more; PMC: with the m-blocks of a panel on
    // different XCDs the 128 x 96 launch fetched 913 MB from the memory side for 218 MB of weights)
    const int bx = blockIdx.x & 7, bq = blockIdx.x >> 3, per = total >> 3, rem8 = total & 7;
    const int b = bx * per + min(bx, rem8) + bq;
    const int ks = b / tiles, bt = b - ks * tiles;
    const int nb = bt / mblocks, mb = bt - nb * mblocks;
    const int k0 = (int)((long)ks * d.ksteps / d.splits), k1 = (int)((long)(ks + 1) * d.ksteps / d.splits);
    const int half = lane >> 5, r31 = lane & 31;
    const unsigned lane4 = (unsigned)lane * 4;
    const int nstages = k1 - k0;
    R rg;
    rg.init(ring, wave, lane, d.A + (size_t)k0 * SPLIT_KSTEP_BYTES, d.A + (size_t)k0 * SPLIT_KSTEP_BYTES, nstages, (long)d.ksteps * SPLIT_KSTEP_BYTES, mb * R::FRA,
            d.mtiles, d.Bp + (size_t)k0 * SPLIT_KSTEP_BYTES, d.kg_stride, min(nb * R::FRB, d.ntiles_alloc - R::FRB));
    float* const Cp = d.C + (size_t)ks * d.part_stride;
    rg.prologue(nstages);
    floatx16 acc[MTW][NTW];
#pragma unroll
    for (int i = 0; i < MTW; ++i)
#pragma unroll
        for (int j = 0; j < NTW; ++j)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.0f;
    rg.run(nstages, ring + (mi * MTW * NT) * 256 + lane4, ring + (NT * R::FRA + nj * NTW * NT) * 256 + lane4, acc);
    const int nt_base = min(nb * R::FRB, d.ntiles_alloc - R::FRB);
#pragma unroll
    for (int i = 0; i < MTW; ++i) {
        const int mtile = mb * R::FRA + mi * MTW + i;
        const int row = mtile * 32 + r31;
        if (mtile >= d.mtiles || row >= d.n) continue;
#pragma unroll
        for (int j = 0; j < NTW; ++j) {
            const int ntile = nt_base + nj * NTW + j;
            if (ntile < nb * R::FRB) continue;             // (a clamped last block recomputes columns its neighbour owns: not stored twice)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const int col = ntile * 32 + 8 * g + 4 * half;
                if (col < d.N) {
                    const v4f o = {acc[i][j][4 * g], acc[i][j][4 * g + 1], acc[i][j][4 * g + 2], acc[i][j][4 * g + 3]};
                    *(__attribute__((address_space(1))) v4f*)(Cp + (size_t)row * d.N + col) = o;
                }
            }
        }
    }
}
