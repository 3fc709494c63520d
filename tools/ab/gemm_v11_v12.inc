// gemm_v11_v12.inc -- A/B-library-only code of csrc/gemm.hip (v11 (32x32x16 MFMAs) and v12 (whole-line staging)).
// Included by csrc/gemm.hip inside its `#ifdef KD_AB_BUILD` block at this position (it uses that
// file's internal helpers); the product libkdstep.so never compiles it.  Build: csrc/build.py --ab.

// =============================================================================
// v11: v8's tile, ring, DMA and barriers (256x256, four waves of 128x128, the 4-slot BK = 32
// LDS-DMA ring, three stages in flight) on 32x32x16 MFMAs, K-major x K-major operands (every
// forward GEMM of the step).  Why: with one wave per SIMD a 16x16x32 MFMA holds the SIMD's
// vector issue for 8 of its 16 cycles, so a k-step's 64 MFMAs leave 512 issue cycles for its
// 8 LDS-DMA pieces (~60 cycles each among MFMAs) and 16 fragment reads, and v8's step measures
// ~1,240 cycles against 1,024 of MFMA; a 32x32x16 MFMA holds issue for 8 of its 32 cycles, so
// the same step (32 MFMAs of 32 cycles) has 768 free issue cycles.  Per step and wave: 8 units
// of 4 MFMAs (unit q: k-half h = q >> 2, row block bi = q & 3, column blocks 0..3), each unit
// carrying one DMA piece of stage t+4 and two fragment reads of stage t+1 (A block q >> 1,
// k-half q & 1, and the same for B).  Fragments: lane l reads row (l & 31), 16-B chunk
// 2h + (l >> 5) of the [rows][32 k] image (v8's swizzle f4 is conflict-free for this read:
// every 16-lane ds_read_b128 group covers the 16 (row & 3, chunk) slots once).  Accumulators:
// f32x16 [4][4] in AGPRs (C^T blocks), viewed as f32x4 [4][16] by the L32 epilogue.
// =============================================================================
typedef __attribute__((ext_vector_type(16))) float f32x16;

__device__ __forceinline__ void mfma32_agpr(f32x16& acc, const bf16x8& a, const bf16x8& b) {
    asm volatile("v_mfma_f32_32x32x16_bf16 %0, %1, %2, %0" : "+a"(acc) : "v"(a), "v"(b));
}

// the tile's last MFMA with its result-latency drain in the same asm statement (mfma_agpr_last;
// 64 wait states >= the 32x32x16's 16-pass latency with margin)
__device__ __forceinline__ void mfma32_agpr_last(f32x16& acc, const bf16x8& a, const bf16x8& b, int last) {
    asm volatile("v_mfma_f32_32x32x16_bf16 %0, %1, %2, %0\n\t"
                 "s_cmp_eq_u32 %3, 0\n\t"
                 "s_cbranch_scc1 .Lkd_mfma32_nodrain%=\n\t"
                 "s_nop 15\n\t"
                 "s_nop 15\n\t"
                 "s_nop 15\n\t"
                 "s_nop 15\n"
                 ".Lkd_mfma32_nodrain%=:"
                 : "+a"(acc) : "v"(a), "v"(b), "s"(__builtin_amdgcn_readfirstlane(last)) : "scc");
}

// 32x32x16 operand fragment (K-major [rows][32 k] stage image): rows rb..rb+31, k-half h
__device__ __forceinline__ bf16x8 frag32(const char* tile, int rb, int h, int lane) {
    const int r = rb + (lane & 31);
    const int c = 2 * h + (lane >> 5);
    return *(const bf16x8*)(tile + r * 64 + ((c ^ f4(r)) << 4));
}

// EXP: v8's build flags (gemm.hip G8_*), of which G8_SWIGLU and G8_ROWSTATS are built here
template <int EXP>
__device__ __forceinline__ void g11_tile(GemmP p, int tm, int tn, char* smem) {
    constexpr bool RSTATS = EXP & G8_ROWSTATS;
    constexpr bool glu = EXP & G8_SWIGLU;
    constexpr int SA = 256 * BK2 * 2, SS = 2 * SA;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wid >> 1, wn = wid & 1;
    const int m0 = tm * 256, n0 = tn * 256;
    const int K = p.K;
    const int nk = (K + BK2 - 1) / BK2, nk_full = K / BK2;
    const __amdgpu_buffer_rsrc_t rsAk = make_rsrc(p.A + (int64_t)m0 * p.lda, rec_bytes(min(256, p.M - m0), p.lda));
    const int nb = tn * 128;
    const __amdgpu_buffer_rsrc_t rsBk = glu ? make_rsrc(p.B, rec_bytes(p.N, p.ldb))
                                            : make_rsrc(p.B + (int64_t)n0 * p.ldb, rec_bytes(min(256, p.N - n0), p.ldb));
    uint32_t va[4], vb[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        va[u] = voff8<false>(wid * 4 + u, lane, p.lda, m0, p.M);
        vb[u] = voff8<false>(wid * 4 + u, lane, p.ldb, n0, p.N);
        if (glu) {   // tile row r -> weight row (r < 128 ? nb + r : I + nb + r - 128); same LDS swizzle
            const int row = 16 * (wid * 4 + u) + (lane >> 2);
            const int gc = (lane & 3) ^ f4(row);
            const int wrow = row < 128 ? nb + row : p.glu + nb + row - 128;
            vb[u] = (uint32_t)((int64_t)wrow * p.ldb * 2 + gc * 16);
        }
    }
    // one DMA instruction (u: 0..3 operand A, 4..7 operand B) of stage st into slot sl
    auto dma = [&](int st, int sl, int u, auto full_tag) {
        constexpr bool FULL = decltype(full_tag)::value;
        const bool isA = u < 4;
        const int i = wid * 4 + (u & 3);
        char* dst = smem + sl * SS + (isA ? 0 : SA) + i * 1024;
        uint32_t v = isA ? va[u & 3] : vb[u & 3];
        int soff = st * BK2 * 2;
        if (!FULL) {
            const int kleft = K - st * BK2;   // valid k of this stage (<= 0: past the end)
            if (kleft < BK2) {                // zero the chunks at k >= K
                const int row = 16 * i + (lane >> 2);
                const int gc = (lane & 3) ^ f4(row);
                if (gc * 8 >= kleft) v = OOB;
                if (kleft <= 0) soff = 0;
            }
        }
        __builtin_amdgcn_raw_ptr_buffer_load_lds(isA ? rsAk : rsBk, (lds_void_t*)dst, 16, v, soff, 0, 0);
    };
    using FullT = std::integral_constant<bool, true>;
    using PartT = std::integral_constant<bool, false>;
    f32x16 acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = (f32x16){};
    const int ra = wm * 128, cb = wn * 128;
#pragma unroll
    for (int st = 0; st < NS8; ++st)
#pragma unroll
        for (int u = 0; u < 8; ++u) dma(st, st, u, PartT{});
    wait_vm<24>();   // stage 0 landed (stages 1..3 may stay in flight)
    __builtin_amdgcn_s_barrier();
    // fragment sets: index 2 * block + k-half
    bf16x8 xa[8], xb[8], ya[8], yb[8];
#pragma unroll
    for (int q = 0; q < 8; ++q) {
        xa[q] = frag32(smem, ra + (q >> 1) * 32, q & 1, lane);
        xb[q] = frag32(smem + SA, cb + (q >> 1) * 32, q & 1, lane);
    }
#define KD_G11_SYNC()                                      \
    {                                                      \
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); \
        wait_vm<16>();                                     \
        __builtin_amdgcn_s_barrier();                      \
    }
    KD_G11_SYNC()
    __builtin_amdgcn_sched_barrier(0);
#define KD_G11_STEP(SL, CA, CB, NA, NB, FT)                                                                  \
    {                                                                                                         \
        const int t_ = t + (SL);                                                                              \
        const char* na_ = smem + (((SL) + 1) % NS8) * SS;                                                     \
        _Pragma("unroll") for (int q = 0; q < 8; ++q) {                                                       \
            const int h_ = q >> 2, bi_ = q & 3;                                                               \
            mfma32_agpr(acc[bi_][0], CB[0 + h_], CA[2 * bi_ + h_]); KD_SB                                     \
            dma(t_ + NS8, (SL), q, FT{});                                                                     \
            KD_SB                                                                                             \
            mfma32_agpr(acc[bi_][1], CB[2 + h_], CA[2 * bi_ + h_]); KD_SB                                     \
            NA[q] = frag32(na_, ra + (q >> 1) * 32, q & 1, lane);                                             \
            KD_SB                                                                                             \
            mfma32_agpr(acc[bi_][2], CB[4 + h_], CA[2 * bi_ + h_]); KD_SB                                     \
            NB[q] = frag32(na_ + SA, cb + (q >> 1) * 32, q & 1, lane);                                        \
            if (q == 7) KD_G11_SYNC()                                                                         \
            KD_SB                                                                                             \
            if (q == 7) mfma32_agpr_last(acc[bi_][3], CB[6 + h_], CA[2 * bi_ + h_], t_ + 1 == nk);            \
            else mfma32_agpr(acc[bi_][3], CB[6 + h_], CA[2 * bi_ + h_]);                                      \
            KD_SB                                                                                             \
        }                                                                                                     \
    }
    int t = 0;
    for (; t + 2 * NS8 <= nk_full; t += NS8) {   // every DMA of these steps lies inside K
        KD_G11_STEP(0, xa, xb, ya, yb, FullT)
        KD_G11_STEP(1, ya, yb, xa, xb, FullT)
        KD_G11_STEP(2, xa, xb, ya, yb, FullT)
        KD_G11_STEP(3, ya, yb, xa, xb, FullT)
    }
    for (; t + NS8 <= nk; t += NS8) {
        KD_G11_STEP(0, xa, xb, ya, yb, PartT)
        KD_G11_STEP(1, ya, yb, xa, xb, PartT)
        KD_G11_STEP(2, xa, xb, ya, yb, PartT)
        KD_G11_STEP(3, ya, yb, xa, xb, PartT)
    }
    const int rem = nk - t;
    if (rem > 0) KD_G11_STEP(0, xa, xb, ya, yb, PartT)
    if (rem > 1) KD_G11_STEP(1, ya, yb, xa, xb, PartT)
    if (rem > 2) KD_G11_STEP(2, xa, xb, ya, yb, PartT)
#undef KD_G11_STEP
#undef KD_G11_SYNC
    // drain the ring (out-of-range DMAs still write LDS) and the MFMA pipe before the
    // accumulators are read back (asm MFMAs are invisible to the hazard recognizer)
    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)\n\ts_nop 15\n\ts_nop 15\n\ts_nop 15\n\ts_nop 15" ::: "memory");
    __builtin_amdgcn_sched_barrier(0);
    __syncthreads();
    const f32x4 (&acc4)[4][16] = *reinterpret_cast<const f32x4(*)[4][16]>(&acc);
    if (glu) epilogue_glu<128, 128, 4, 16, NTH8, true>(p, acc4, smem, m0, nb, wm, wn, lane, tid);
    else epilogue2<256, 256, 2, 2, 128, 128, 4, 16, NTH8, true, RSTATS, true>(p, acc4, smem, m0, n0, wm, wn, lane, tid);
}

template <int EXP = 0>
__global__ void __launch_bounds__(NTH8, 1) k_gemm11(GemmP p_) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tiles_m = (p_.M + 255) / 256, tiles_n = (p_.N + 255) / 256;
    GemmP p = p_;
    if (p.gy > 1) {   // split-K: this grid row owns K range [k0, k0 + kchunk) -> fp32 partial plane
        const int64_t k0 = (int64_t)blockIdx.y * p.kchunk;
        p.K = (int)min((int64_t)p.K - k0, p.kchunk);
        p.A += k0;
        p.B += k0;
        p.C = (float*)p.C + (int64_t)blockIdx.y * p.split_stride;
    }
    int tm, tn;
    tile_of(p.gx, tiles_m, tiles_n, tm, tn, p.tile0, p.gm);
    g11_tile<EXP>(p, tm, tn, smem);
}

// =============================================================================
// v12: v8 (256x256 tile, four waves of 128x128 on 16x16x32 MFMAs, AGPR accumulators, the same
// 128 KiB of ring) with WHOLE-CACHE-LINE staging of K-major operands.  v8's K-major DMA
// instruction covers 16 rows x 64 B (one BK = 32 stage), half of a 128-B line per row; the
// diagnostic build that reads 8 rows x 128 B per instruction instead (same instructions and
// bytes, forced variant 25) ran 8-10 % faster on the big forward shapes (profiles/r04, the
// hipBLASLt kernel stages BK = 64 for the same reason).  Here the ring holds two PAIRS of
// stages (stages 2q, 2q+1 = 64 k): a pair image is [256 rows][128 B] per operand (k 0..63 of
// each row, 16-B chunk c at physical chunk c ^ swp(row), swp(r) = (r >> 1) & 7: every
// 16-lane group of a ds_read_b128 fragment read covers the 16 (row & 1, chunk) bank slots once),
// filled by instructions of 8 rows x 128 B (lane l: row 8i + (l >> 3), logical chunk
// (l & 7) ^ swp(row) -> lane-linear LDS position).  Compute stays per BK = 32 stage (64 MFMAs
// per step, fragments of stage t+1 read during step t).  Pair q (in pair slot q % 2) can only be
// refilled once stage 2q-3 is in registers, so pair q is issued in the odd step 2q-3, 16 DMA
// instructions per wave (two per unit), and must land by the end of step 2q-2: step ends wait
// vmcnt(0) after even steps and vmcnt(16) after odd ones.
// =============================================================================
__device__ __forceinline__ int swp(int r) { return (r >> 1) & 7; }

// 16x16x32 operand fragment of stage half h (k 32h..32h+31) from a pair image [rows][128 B]
__device__ __forceinline__ bf16x8 frag_pair(const char* img, int rb, int h, int lane) {
    const int r = rb + (lane & 15);
    const int c = 4 * h + (lane >> 4);
    return *(const bf16x8*)(img + r * 128 + ((c ^ swp(r)) << 4));
}

constexpr int G12_NOBARRIER = 256;
template <int EXP>
__device__ __forceinline__ void g12_tile(GemmP p, int tm, int tn, char* smem) {
    constexpr bool RSTATS = EXP & G8_ROWSTATS;
    constexpr bool glu = EXP & G8_SWIGLU;
    // G12_NOBARRIER (forced variant 27; v12's own flag, the value v8 uses for pre-tiled B): no barrier
    // at the end of odd steps.  The only cross-wave
    // hazards are per PAIR: RAW (pair q, issued in step 2q-3, is first read in step 2q-1: every
    // wave's vmcnt(0) + the barrier at the end of EVEN step 2q-2) and WAR (pair q+2 overwrites
    // pair q's slot in odd step 2q+1, after every wave's last read of pair q in step 2q: the
    // lgkmcnt(0) + barrier at the end of even step 2q); the odd-step barrier guards nothing.
    constexpr bool NOB = EXP & G12_NOBARRIER;
    constexpr int PA = 256 * 128;       // one operand's pair image (32 KiB)
    constexpr int PS = 2 * PA;          // a pair slot (64 KiB); two of them
    const int tid = threadIdx.x, lane = tid & 63;
    const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wid >> 1, wn = wid & 1;
    const int m0 = tm * 256, n0 = tn * 256;
    const int K = p.K;
    const int nk = (K + BK2 - 1) / BK2, nk_full = K / BK2;
    const __amdgpu_buffer_rsrc_t rsA = make_rsrc(p.A + (int64_t)m0 * p.lda, rec_bytes(min(256, p.M - m0), p.lda));
    const int nb = tn * 128;
    const __amdgpu_buffer_rsrc_t rsB = glu ? make_rsrc(p.B, rec_bytes(p.N, p.ldb))
                                           : make_rsrc(p.B + (int64_t)n0 * p.ldb, rec_bytes(min(256, p.N - n0), p.ldb));
    // wave w fills rows 64w .. 64w + 63 of each operand: instruction j (0..7) rows 64w + 8j + (l >> 3);
    // the lane's swizzled chunk depends on j only through j & 1, the row step goes to soffset
    const int rlo = 64 * wid + (lane >> 3);
    const int brow = glu ? (wid < 2 ? nb : p.glu + nb - 128) : 0;   // weight row of tile row 0 of this wave's half
    uint32_t va[2], vb[2];
    int gcl[2];
#pragma unroll
    for (int e = 0; e < 2; ++e) {
        const int gc = (lane & 7) ^ swp(rlo + 8 * e);
        gcl[e] = gc;
        va[e] = (uint32_t)((int64_t)rlo * p.lda * 2 + gc * 16);
        vb[e] = (uint32_t)((int64_t)(brow + rlo) * p.ldb * 2 + gc * 16);
    }
    // instruction j of operand (isA) of pair q into pair slot ps
    auto dma = [&](int q, int ps, int j, bool isA, auto full_tag) {
        constexpr bool FULL = decltype(full_tag)::value;
        char* dst = smem + ps * PS + (isA ? 0 : PA) + (wid * 8 + j) * 1024;
        uint32_t v = isA ? va[j & 1] : vb[j & 1];
        const int64_t ld = isA ? p.lda : p.ldb;
        int kq = q * 64;
        if (!FULL) {
            const int kleft = K - kq;     // valid k of this pair (<= 0: past the end)
            if (gcl[j & 1] * 8 >= kleft) v = OOB;
            if (kleft <= 0) kq = 0;
        }
        const int soff = __builtin_amdgcn_readfirstlane((int)(8 * j * ld * 2 + kq * 2));
        __builtin_amdgcn_raw_ptr_buffer_load_lds(isA ? rsA : rsB, (lds_void_t*)dst, 16, v, soff, 0, 0);
    };
    using FullT = std::integral_constant<bool, true>;
    using PartT = std::integral_constant<bool, false>;
    f32x4 acc[8][8];
#pragma unroll
    for (int i = 0; i < 8; ++i)
#pragma unroll
        for (int j = 0; j < 8; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};
    const int ra = wm * 128, cb = wn * 128;
    // prologue: pairs 0 and 1 (stages 0..3) into pair slots 0 and 1; pair 0 landed
#pragma unroll
    for (int q = 0; q < 2; ++q)
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            dma(q, q, j, true, PartT{});
            dma(q, q, j, false, PartT{});
        }
    wait_vm<16>();
    __builtin_amdgcn_s_barrier();
    bf16x8 xa[8], xb[8], ya[8], yb[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) {
        xa[u] = frag_pair(smem, ra + u * 16, 0, lane);
        xb[u] = frag_pair(smem + PA, cb + u * 16, 0, lane);
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_sched_barrier(0);
#define KD_G12_SYNC(ODD)                                   \
    if (!(NOB && (ODD))) {                                 \
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); \
        if (ODD) wait_vm<16>();                            \
        else wait_vm<0>();                                 \
        __builtin_amdgcn_s_barrier();                      \
    }
    // step t + SL (SL = 0..3 of a group of four; t % 4 == 0): stage t+SL is in registers (CA, CB);
    // stage t+SL+1 is read from pair slot ((SL+1) >> 1) & 1, half (SL+1) & 1; odd SL issue pair
    // (t+SL+3)/2 into pair slot ((SL+3) >> 1) & 1
#define KD_G12_STEP(SL, CA, CB, NA, NB, FT)                                                                  \
    {                                                                                                         \
        const int t_ = t + (SL);                                                                              \
        const char* na_ = smem + ((((SL) + 1) >> 1) & 1) * PS;                                                \
        constexpr int nh_ = ((SL) + 1) & 1;                                                                   \
        constexpr bool odd_ = (SL) & 1;                                                                       \
        const int q_ = (t_ + 3) >> 1;                                                                         \
        constexpr int qs_ = (((SL) + 3) >> 1) & 1;                                                            \
        _Pragma("unroll") for (int u = 0; u < 8; ++u) {                                                       \
            mfma_agpr(acc[u][0], CB[0], CA[u]); KD_SB                                                         \
            if (odd_) dma(q_, qs_, u, true, FT{});                                                            \
            KD_SB                                                                                             \
            mfma_agpr(acc[u][1], CB[1], CA[u]); KD_SB                                                         \
            if (u < 4) NA[2 * u] = frag_pair(na_, ra + 2 * u * 16, nh_, lane);                                \
            KD_SB                                                                                             \
            mfma_agpr(acc[u][2], CB[2], CA[u]); mfma_agpr(acc[u][3], CB[3], CA[u]); KD_SB                     \
            if (u < 4) NB[2 * u] = frag_pair(na_ + PA, cb + 2 * u * 16, nh_, lane);                           \
            KD_SB                                                                                             \
            mfma_agpr(acc[u][4], CB[4], CA[u]); KD_SB                                                         \
            if (odd_) dma(q_, qs_, u, false, FT{});                                                           \
            KD_SB                                                                                             \
            mfma_agpr(acc[u][5], CB[5], CA[u]); KD_SB                                                         \
            if (u < 4) NA[2 * u + 1] = frag_pair(na_, ra + (2 * u + 1) * 16, nh_, lane);                      \
            KD_SB                                                                                             \
            mfma_agpr(acc[u][6], CB[6], CA[u]); KD_SB                                                         \
            if (u < 4) NB[2 * u + 1] = frag_pair(na_ + PA, cb + (2 * u + 1) * 16, nh_, lane);                 \
            if (u == 7) KD_G12_SYNC(odd_)                                                                     \
            KD_SB                                                                                             \
            if (u == 7) mfma_agpr_last(acc[u][7], CB[7], CA[u], t_ + 1 == nk);                                \
            else mfma_agpr(acc[u][7], CB[7], CA[u]);                                                          \
            KD_SB                                                                                             \
        }                                                                                                     \
    }
    int t = 0;
    for (; t + 8 <= nk_full; t += 4) {   // every pair these steps issue (up to stage t + 7) lies inside K
        KD_G12_STEP(0, xa, xb, ya, yb, FullT)
        KD_G12_STEP(1, ya, yb, xa, xb, FullT)
        KD_G12_STEP(2, xa, xb, ya, yb, FullT)
        KD_G12_STEP(3, ya, yb, xa, xb, FullT)
    }
    for (; t + 4 <= nk; t += 4) {
        KD_G12_STEP(0, xa, xb, ya, yb, PartT)
        KD_G12_STEP(1, ya, yb, xa, xb, PartT)
        KD_G12_STEP(2, xa, xb, ya, yb, PartT)
        KD_G12_STEP(3, ya, yb, xa, xb, PartT)
    }
    const int rem = nk - t;
    if (rem > 0) KD_G12_STEP(0, xa, xb, ya, yb, PartT)
    if (rem > 1) KD_G12_STEP(1, ya, yb, xa, xb, PartT)
    if (rem > 2) KD_G12_STEP(2, xa, xb, ya, yb, PartT)
#undef KD_G12_STEP
#undef KD_G12_SYNC
    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)\n\ts_nop 15\n\ts_nop 15" ::: "memory");
    __builtin_amdgcn_sched_barrier(0);
    __syncthreads();
    if (glu) epilogue_glu<128, 128, 8, 8, NTH8>(p, acc, smem, m0, nb, wm, wn, lane, tid);
    else epilogue2<256, 256, 2, 2, 128, 128, 8, 8, NTH8, true, RSTATS>(p, acc, smem, m0, n0, wm, wn, lane, tid);
}

template <int EXP = 0>
__global__ void __launch_bounds__(NTH8, 1) k_gemm12(GemmP p_) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tiles_m = (p_.M + 255) / 256, tiles_n = (p_.N + 255) / 256;
    GemmP p = p_;
    if (p.gy > 1) {   // split-K: this grid row owns K range [k0, k0 + kchunk) -> fp32 partial plane
        const int64_t k0 = (int64_t)blockIdx.y * p.kchunk;
        p.K = (int)min((int64_t)p.K - k0, p.kchunk);
        p.A += k0;
        p.B += k0;
        p.C = (float*)p.C + (int64_t)blockIdx.y * p.split_stride;
    }
    int tm, tn;
    tile_of(p.gx, tiles_m, tiles_n, tm, tn, p.tile0, p.gm);
    g12_tile<EXP>(p, tm, tn, smem);
}

