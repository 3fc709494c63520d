// gemm_glu_epi_v0.inc -- A/B-library-only code of csrc/gemm.hip (the round-4 SwiGLU epilogue (KD_GLU_EPI_V0)).
// Included by csrc/gemm.hip inside its `#ifdef KD_AB_BUILD` block at this position (it uses that
// file's internal helpers); the product libkdstep.so never compiles it.  Build: csrc/build.py --ab.


// the round-4 SwiGLU epilogue before the packed rewrite (G8_GLU_V0 / KD_GLU_EPI_V0=1: A/B only)
template <int TM, int TN, int MT, int NT, int NTHR, bool L32 = false>
__device__ __forceinline__ void epilogue_glu_v0(const GemmP& p, const f32x4 (&acc)[MT][NT], char* smem, int m0, int nb, int wm,
                                             int wn, int lane, int tid) {
    float alpha = p.alpha;
    if (p.alpha_dev) alpha *= *p.alpha_dev;
    f32x4 bcol[NT];
#pragma unroll
    for (int j = 0; j < NT; ++j) bcol[j] = (f32x4){0.f, 0.f, 0.f, 0.f};
    constexpr int RS = 256 * 2 + 16;
    epi_to_lds<KD_ACT_NONE, TM, TN, MT, NT, false, L32>(acc, smem, RS, alpha, bcol, wm, wn, lane, 0, 256);
    __syncthreads();
    const int I = p.glu;
    const bool full = m0 + 256 <= p.M;
    if (p.aux) {
#pragma unroll 4
        for (int idx = tid; idx < 256 * 32; idx += NTHR) {
            const int lr = idx >> 5, c = idx & 31, row = m0 + lr;
            if (!full && row >= p.M) continue;
            const int col = c < 16 ? nb + c * 8 : I + nb + (c - 16) * 8;
            *(bf16x8*)(p.aux + (int64_t)row * p.ld_aux + col) = *(const bf16x8*)(smem + lr * RS + c * 16);
        }
    }
#pragma unroll 4
    for (int idx = tid; idx < 256 * 16; idx += NTHR) {
        const int lr = idx >> 4, c = idx & 15, row = m0 + lr;
        if (!full && row >= p.M) continue;
        const bf16x8 g = *(const bf16x8*)(smem + lr * RS + c * 16);
        const bf16x8 u = *(const bf16x8*)(smem + lr * RS + 256 + c * 16);
        bf16x8 o;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const float gf = (float)g[e];
            o[e] = (bf16)(silu_fast(gf) * (float)u[e]);
        }
        *(bf16x8*)((bf16*)p.C + (int64_t)row * p.ldc + nb + c * 8) = o;
    }
}
