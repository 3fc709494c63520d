// Student generate(): single-token decode attention over a KV cache, and the greedy token
// choice with the logits processors the reference's evaluation sets (gfx950).
//
// Replaces, in LlavaOnevisionForConditionalGeneration.generate as called by
// evaluation/onevisionv3/evaluate_onevision.py:185-195 (max_new_tokens=32,
// repetition_penalty=1.2, no_repeat_ngram_size=2, greedy: do_sample is unset, so temperature
// is inert):
//   k_attn_decode   the SDPA of one new query row against the cached keys/values of every
//                   layer (Qwen2 GQA, scale hd^-0.5, fp32 softmax)
//   k_gen_select    RepetitionPenaltyLogitsProcessor (score < 0 ? score * p : score / p on every
//                   token id present in the sequence, float32), NoRepeatNGramLogitsProcessor
//                   (bans every token that would repeat an n-gram of the sequence), then the
//                   greedy argmax (lowest index on ties, as torch.argmax), appended to the
//                   device-resident sequence (no host sync per token).
// and their batched forms for generate_batch() (up to 16 prompts per step, per-row lengths on the
// device, batch-invariant): k_gemv_batch (bf16 MFMA, the batch as M), k_attn_decode_part_batch,
// k_gen_select_batch, k_rope_rows; and for generate_grouped() (one image prefill shared by its
// questions) the suffix rows of a chunk: k_gemv_slabs (k_gemv_batch for more than 16 rows, row for
// row the same bits) and k_attn_extend_part (ragged suffix queries against prefix + own suffix);
// and for an allowed set of token ids (the evaluation's RestrictedLogitsProcessor,
// evaluate_onevision.py:141-158) k_gemv_gather / k_gemv_batch_gather (the lm_head over the allowed
// rows only, with the full head's bits) and k_gen_select_ids (the choice among the allowed ids);
// and for do_sample=True k_gen_sample (temperature, top-k, top-p and a Philox draw in place of the
// argmax, over a full row or the compact allowed row).
//
// Each algorithm has one body.  The single-row and the batched form of a kernel differ in where a
// row's pointers and length come from, not in what is computed, so they share a __forceinline__
// device function and keep only their own setup and stores:
//   gen_select_row   flags, processors, argmax: k_gen_select, k_gen_select_batch
//   gen_flags_row, gen_flags_ids, gen_processed
//                    the processors' flag passes and the processed score of an entry: the selects
//                    and k_gen_sample
//   gen_ngram_scan, gen_block_argmax, gen_row / gen_row_store
//                    the n-gram prefix match of both flag passes, the block argmax of both selects,
//                    and the row frame (pointer, clamped length, stores) of the batched choosers
//   gb_row_rstd, gb_stage_slab, gb_wave_order_sum, gb_store
//                    the 16-row slab of k_gemv_batch and k_gemv_slabs, which is why a row of
//                    kd_gemv_rows has kd_gemv_batch's bits; k_gemv_batch_reduce serves both
//   k_rope_rows      also kd_rope_row (one row)
// and the launchers share dispatch_epi / dispatch_hd (runtime value -> template instance) and
// check_gemv_args / check_attn_args.  The one pair left as two copies is the dot-product loop of
// k_gemv and k_gemv_wide (a workgroup per output; k_gemv_rows before kd_gemv_rows took that name
// for something else): shared, it was measurably slower (see there).
#include "common.h"

#include <algorithm>
#include <climits>
#include <cmath>
#include <string>
#include <type_traits>

namespace kd {

namespace {

constexpr int NT = 256;

// Split-KV decode attention (flash-decoding): workgroup (h, c) handles keys [c*CH, c*CH + CH)
// of query head h and writes its partial (max, sum, unnormalised output) to the workspace;
// k_attn_decode_combine merges the partials of a head.  Chunks at or past n exit after writing
// an empty partial, so the grid depends only on smax (fixed under graph capture).
// The step's own key/value row (k_new/v_new [HKV, hdp]) stands in for cache position n - 1 and
// is stored there by chunk 0 of the first query head of each KV group (read by later steps only).
// n = *cur_dev when cur_dev is given: the position lives on the device.
constexpr int CH = 64;   // keys per workgroup: 4 lanes per key for the scores, 4 key groups for P.V

template <int HD>
__global__ void __launch_bounds__(NT) k_attn_decode_part(const bf16* __restrict__ q, const bf16* __restrict__ k_new,
                                                         const bf16* __restrict__ v_new, bf16* __restrict__ kc,
                                                         bf16* __restrict__ vc, float* __restrict__ part, int H,
                                                         int HKV, int hdp, int smax, int n,
                                                         const int* __restrict__ cur_dev, float scale) {
    __shared__ float p_s[CH];
    __shared__ float red[8];
    __shared__ float acc_s[NT];
    if (cur_dev) n = *cur_dev;
    const int h = blockIdx.x, c = blockIdx.y, nch = gridDim.y, kvh = h / (H / HKV);
    float* pp = part + ((size_t)h * nch + c) * (HD + 2);
    const int j0 = c * CH;
    bf16* K = kc + (size_t)kvh * smax * hdp;
    bf16* V = vc + (size_t)kvh * smax * hdp;
    const bf16* kn = k_new + (size_t)kvh * hdp;
    const bf16* vn = v_new + (size_t)kvh * hdp;
    if (c == 0 && h % (H / HKV) == 0)
        for (int d = threadIdx.x; d < hdp; d += NT) {
            K[(size_t)(n - 1) * hdp + d] = kn[d];
            V[(size_t)(n - 1) * hdp + d] = vn[d];
        }
    if (j0 >= n) {   // empty chunk
        if (threadIdx.x == 0) { pp[0] = -INFINITY; pp[1] = 0.f; }
        if (threadIdx.x < HD) pp[2 + threadIdx.x] = 0.f;
        return;
    }
    // scores: key j0 + threadIdx/4, lane quarter (threadIdx & 3) covers HD/4 dims
    constexpr int DQ = HD / 4;
    const int kj = j0 + (threadIdx.x >> 2), qd = (threadIdx.x & 3) * DQ;
    float s = -INFINITY;
    if (kj < n) {
        const bf16* kr = (kj == n - 1 ? kn : K + (size_t)kj * hdp) + qd;
        const bf16* qh = q + (size_t)h * hdp + qd;
        float a = 0.f;
#pragma unroll
        for (int d = 0; d < DQ; d += 8) {
            const bf16x8 k8 = *(const bf16x8*)(kr + d);
            const bf16x8 q8 = *(const bf16x8*)(qh + d);
#pragma unroll
            for (int e = 0; e < 8; ++e) a += (float)q8[e] * (float)k8[e];
        }
        a += __shfl_xor(a, 1, 64);
        a += __shfl_xor(a, 2, 64);
        s = a * scale;
    }
    const float m = block_max<NT / 64>(s, red);
    const float pv = kj < n ? __expf(s - m) : 0.f;
    if ((threadIdx.x & 3) == 0) p_s[threadIdx.x >> 2] = pv;
    const float l = block_sum<NT / 64>((threadIdx.x & 3) == 0 ? pv : 0.f, red);   // barriers publish p_s
    constexpr int G = NT / HD;
    const int d = threadIdx.x % HD, g = threadIdx.x / HD;
    float acc = 0.f;
    const int jend = min(CH, n - j0);
    for (int jj = g; jj < jend; jj += G) {
        const int j = j0 + jj;
        acc += p_s[jj] * (float)(j == n - 1 ? vn[d] : V[(size_t)j * hdp + d]);
    }
    acc_s[threadIdx.x] = acc;
    __syncthreads();
    if (g == 0) {
        float tsum = 0.f;
#pragma unroll
        for (int i = 0; i < G; ++i) tsum += acc_s[i * HD + d];
        pp[2 + d] = tsum;
        if (d == 0) { pp[0] = m; pp[1] = l; }
    }
}

constexpr int MAX_CH = 512;   // chunks per head (smax <= 32768)

// Merge the nch partials of head h: chunk maxima and weights staged in LDS (one load round
// trip), then 256 threads = HD dims x (256 / HD) chunk groups accumulate in parallel.
template <int HD>
__global__ void __launch_bounds__(NT) k_attn_decode_combine(const float* __restrict__ part, int nch,
                                                            bf16* __restrict__ o) {
    __shared__ float ms[MAX_CH], red[8], acc_s[NT];
    const int h = blockIdx.x;
    const float* pp = part + (size_t)h * nch * (HD + 2);
    float m = -INFINITY;
    for (int c = threadIdx.x; c < nch; c += NT) {
        ms[c] = pp[(size_t)c * (HD + 2)];
        m = fmaxf(m, ms[c]);
    }
    m = block_max<NT / 64>(m, red);
    float l = 0.f;
    for (int c = threadIdx.x; c < nch; c += NT) {
        const float w = ms[c] == -INFINITY ? 0.f : __expf(ms[c] - m);
        ms[c] = w;
        l += w * pp[(size_t)c * (HD + 2) + 1];
    }
    l = block_sum<NT / 64>(l, red);   // barriers publish the weights in ms[]
    constexpr int G = NT / HD;
    const int d = threadIdx.x % HD, g = threadIdx.x / HD;
    float acc = 0.f;
    for (int c = g; c < nch; c += G) acc += ms[c] * pp[(size_t)c * (HD + 2) + 2 + d];
    acc_s[threadIdx.x] = acc;
    __syncthreads();
    if (g == 0) {
        float tsum = 0.f;
#pragma unroll
        for (int i = 0; i < G; ++i) tsum += acc_s[i * HD + d];
        o[(size_t)h * HD + d] = (bf16)(tsum / l);
    }
}

// Stage the token row x[K] into LDS as fp32; with norm_w, as kd_norm_fwd's RMSNorm output
// (bf16(x * rsqrt(mean(x^2) + eps) * w), rounded to bf16 as the unfused kernel stores it), so the
// norm costs no launch of its own.
__device__ __forceinline__ void stage_x(const bf16* __restrict__ x, const bf16* __restrict__ norm_w, float eps, int K,
                                        float* xs, float* red) {
    float ss = 0.f;
    for (int k = threadIdx.x; k < K; k += NT) {
        const float v = (float)x[k];
        xs[k] = v;
        ss += v * v;
    }
    if (norm_w) {
        const float rstd = rsqrtf(block_sum<NT / 64>(ss, red) / K + eps);
        for (int k = threadIdx.x; k < K; k += NT) xs[k] = (float)(bf16)(xs[k] * rstd * (float)norm_w[k]);
    }
    __syncthreads();
}

// Decode GEMV: y[n] = epilogue(sum_k x[k] * W[n][k]) for one token row, one wave per output
// (two weight rows, n and I + n, for the SwiGLU form).  Weight rows are read once, 16 B per lane,
// so the decode step streams its weights at HBM rate instead of running 256-row GEMM tiles at
// M = 1.  EPI: 0 none, 1 + bias[n], 2 + residual[n], 3 silu(row n) * (row I + n).
//
// k_gemv and k_gemv_wide keep their own copy of the dot-product loop and the epilogue on purpose.
// With the two behind one __forceinline__ body (k stride and reduction as parameters) hipcc
// schedules the loop differently (same registers, same occupancy, same bits), and these 5 - 9 us
// kernels, ~100 launches per token, came out 3 - 7 % slower in a kernel trace: generate() lost
// 0.8 ms of 48 (profiles/decode_dedupe/bench_ab.txt).  A change to one loop belongs in the other,
// and a change to k_gemv's in k_gemv_gather, whose logits must stay k_gemv's bit for bit.
template <int EPI>
__global__ void __launch_bounds__(NT) k_gemv(const bf16* __restrict__ x, const bf16* __restrict__ W, int64_t ldw,
                                             const bf16* __restrict__ extra, bf16* __restrict__ y, int N, int K,
                                             int I, const bf16* __restrict__ norm_w, float eps) {
    extern __shared__ float xs[];
    __shared__ float red[8];
    stage_x(x, norm_w, eps, K, xs, red);
    const int n = blockIdx.x * (NT / 64) + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (n >= N) return;
    const bf16* r0 = W + (size_t)n * ldw;
    const bf16* r1 = W + (size_t)(I + n) * ldw;
    float a0 = 0.f, a1 = 0.f;
    for (int k = lane * 8; k < K; k += 512) {
        const bf16x8 w0 = *(const bf16x8*)(r0 + k);
#pragma unroll
        for (int e = 0; e < 8; ++e) a0 += xs[k + e] * (float)w0[e];
        if constexpr (EPI == 3) {
            const bf16x8 w1 = *(const bf16x8*)(r1 + k);
#pragma unroll
            for (int e = 0; e < 8; ++e) a1 += xs[k + e] * (float)w1[e];
        }
    }
    a0 = wave_sum(a0);
    if constexpr (EPI == 3) a1 = wave_sum(a1);
    if (lane == 0) {
        float v = a0;
        if constexpr (EPI == 1 || EPI == 2) v += (float)extra[n];
        if constexpr (EPI == 3) v = silu_fast(a0) * a1;
        y[n] = (bf16)v;
    }
}

// Workgroup-per-output form of k_gemv for few output rows with long K (o_proj / down_proj of the
// 0.5B student: N = 896, K up to 4864): 256 threads split K, block reduction, so N workgroups
// instead of N / 4 keep every CU streaming.  (k_gemv_rows until the public kd_gemv_rows, which is
// k_gemv_slabs below, took that name for something else.)
template <int EPI>
__global__ void __launch_bounds__(NT) k_gemv_wide(const bf16* __restrict__ x, const bf16* __restrict__ W, int64_t ldw,
                                                  const bf16* __restrict__ extra, bf16* __restrict__ y, int K, int I,
                                                  const bf16* __restrict__ norm_w, float eps) {
    extern __shared__ float xs[];
    __shared__ float red[8];
    stage_x(x, norm_w, eps, K, xs, red);
    const int n = blockIdx.x;
    const bf16* r0 = W + (size_t)n * ldw;
    const bf16* r1 = W + (size_t)(I + n) * ldw;
    float a0 = 0.f, a1 = 0.f;
    for (int k = threadIdx.x * 8; k < K; k += NT * 8) {
        const bf16x8 w0 = *(const bf16x8*)(r0 + k);
#pragma unroll
        for (int e = 0; e < 8; ++e) a0 += xs[k + e] * (float)w0[e];
        if constexpr (EPI == 3) {
            const bf16x8 w1 = *(const bf16x8*)(r1 + k);
#pragma unroll
            for (int e = 0; e < 8; ++e) a1 += xs[k + e] * (float)w1[e];
        }
    }
    a0 = block_sum<NT / 64>(a0, red);
    if constexpr (EPI == 3) a1 = block_sum<NT / 64>(a1, red);
    if (threadIdx.x == 0) {
        float v = a0;
        if constexpr (EPI == 1 || EPI == 2) v += (float)extra[n];
        if constexpr (EPI == 3) v = silu_fast(a0) * a1;
        y[n] = (bf16)v;
    }
}

// NoRepeatNGramLogitsProcessor, the scan of both flag passes: the last (ngram - 1) tokens as a
// prefix; ban(t) for the token t that followed every earlier occurrence of that prefix (only once
// cur_len + 1 >= ngram).
template <class Ban>
__device__ __forceinline__ void gen_ngram_scan(const int64_t* __restrict__ seq, int len, int ngram, Ban ban) {
    if (ngram > 0 && len + 1 >= ngram)
        for (int i = threadIdx.x; i + ngram <= len; i += blockDim.x) {
            bool match = true;
            for (int k = 0; k < ngram - 1; ++k) match &= seq[i + k] == seq[len - ngram + 1 + k];
            if (match) ban(seq[i + ngram - 1]);
        }
}

// The token choice of one row by one workgroup of 1024 threads: V bytes of flags (bit 0 = seen,
// bit 1 = banned) from the len ids of seq, then the processed-score argmax, which thread 0 returns
// (the other threads' value is not the row's).  The vector paths need 16-byte aligned logits and
// flags (the single-row workspace always is; row b of a batch may not be) and fall back to bytes.
// The flag pass of gen_select_row, shared with the sampling kernel (k_gen_sample): ends on a barrier.
__device__ __forceinline__ void gen_flags_row(int V, const int64_t* __restrict__ seq, int len, float penalty, int ngram,
                                              uint8_t* __restrict__ flags) {
    {   // clear the flags, 16 B per store
        const int v16 = ((uintptr_t)flags & 15) == 0 ? V >> 4 : 0;
        for (int i = threadIdx.x; i < v16; i += blockDim.x) ((u32x4*)flags)[i] = u32x4{0u, 0u, 0u, 0u};
        for (int i = (v16 << 4) + threadIdx.x; i < V; i += blockDim.x) flags[i] = 0;
    }
    __syncthreads();
    // RepetitionPenaltyLogitsProcessor: every id of the sequence (prompt + generated)
    if (penalty != 1.0f)
        for (int i = threadIdx.x; i < len; i += blockDim.x) {
            const int64_t t = seq[i];
            if (t >= 0 && t < V) flags[t] |= 1;
        }
    __syncthreads();   // the two processors OR different bits into the same bytes
    gen_ngram_scan(seq, len, ngram, [&](int64_t t) {
        if (t >= 0 && t < V) flags[t] |= 2;
    });
    __syncthreads();
}

// The processed fp32 score of one entry from its flags (bit 0 = seen: the repetition penalty,
// correctly rounded; bit 1 = banned): every token choice, greedy or sampled, goes through this.
__device__ __forceinline__ float gen_processed(float s, uint32_t f, float penalty) {
    if (f & 1) s = s < 0.f ? __fmul_rn(s, penalty) : __fdiv_rn(s, penalty);
    if (f & 2) s = -INFINITY;
    return s;
}

// The block argmax of the greedy kernels (1024 threads): every thread's (best, bi) in, the row's
// winner out on thread 0 (the other threads' values are not the row's): the larger score, the lower
// index on a tie, NaN never wins.  An index that no score ever set (0x7fffffff) becomes 0, what
// torch.argmax returns for a row of -inf.
__device__ __forceinline__ int gen_block_argmax(float& best, int bi) {
    __shared__ float sv[16];
    __shared__ int si[16];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const float ov = __shfl_xor(best, off, 64);
        const int oi = __shfl_xor(bi, off, 64);
        if (ov > best || (ov == best && oi < bi)) { best = ov; bi = oi; }
    }
    const int w = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) { sv[w] = best; si[w] = bi; }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int k = 1; k < (int)(blockDim.x >> 6); ++k)
            if (sv[k] > best || (sv[k] == best && si[k] < bi)) { best = sv[k]; bi = si[k]; }
        if (bi == 0x7fffffff) bi = 0;
    }
    return bi;
}

// The frame of the batched choosers (k_gen_select_batch, k_gen_select_ids, k_gen_sample), row
// b = blockIdx.x: its sequence (row stride smax) and length cur_dev[b], kept inside the row so that
// the ids read never leave it; gen_row_store (thread 0) writes the token.  A full row (len == smax)
// still reports its token in out[b].
struct GenRow {
    int64_t* seq;
    int len;
};
__device__ __forceinline__ GenRow gen_row(int64_t* __restrict__ seq_all, int smax, const int* __restrict__ cur_dev) {
    const int b = blockIdx.x;
    return {seq_all + (size_t)b * smax, max(0, min(cur_dev[b], smax))};
}
__device__ __forceinline__ void gen_row_store(const GenRow& r, int smax, int* __restrict__ cur_dev,
                                              int64_t* __restrict__ out, int64_t tok) {
    if (r.len < smax) r.seq[r.len] = tok;
    if (out) out[blockIdx.x] = tok;
    cur_dev[blockIdx.x] = r.len + 1;
}

__device__ __forceinline__ int gen_select_row(const bf16* __restrict__ logits, int V, const int64_t* __restrict__ seq,
                                              int len, float penalty, int ngram, uint8_t* __restrict__ flags) {
    gen_flags_row(V, seq, len, penalty, ngram, flags);
    float best = -INFINITY;
    int bi = 0x7fffffff;
    auto consider = [&](int i, float s, uint32_t f) {
        s = gen_processed(s, f, penalty);
        if (s > best || (s == best && i < bi)) { best = s; bi = i; }   // NaN never wins
    };
    // 8 logits (16 B) + 8 flags per step
    const int v8 = (((uintptr_t)logits & 15) == 0 && ((uintptr_t)flags & 7) == 0) ? V >> 3 : 0;
    for (int c = threadIdx.x; c < v8; c += blockDim.x) {
        const bf16x8 lv = ((const bf16x8*)logits)[c];
        const u32x2 fv = ((const u32x2*)flags)[c];
#pragma unroll
        for (int e = 0; e < 8; ++e) consider(c * 8 + e, (float)lv[e], ((e < 4 ? fv.x : fv.y) >> (8 * (e & 3))) & 255u);
    }
    for (int i = (v8 << 3) + threadIdx.x; i < V; i += blockDim.x) consider(i, (float)logits[i], flags[i]);
    return gen_block_argmax(best, bi);
}

// seq [len + 1] int64 (the new token is written at seq[len]); len = *cur_dev, then incremented,
// when cur_dev is given.
__global__ void __launch_bounds__(1024) k_gen_select(const bf16* __restrict__ logits, int V, int64_t* __restrict__ seq,
                                                     int len, int* __restrict__ cur_dev, float penalty, int ngram,
                                                     uint8_t* __restrict__ flags, int64_t* __restrict__ out) {
    if (cur_dev) len = *cur_dev;
    const int bi = gen_select_row(logits, V, seq, len, penalty, ngram, flags);
    if (threadIdx.x == 0) {
        seq[len] = bi;
        if (out) *out = bi;
        if (cur_dev) *cur_dev = len + 1;
    }
}

// ------------------------------------------------------------ batched decode (nb <= 16 rows) ----
// Every per-row quantity below is computed by code whose arithmetic and order depend on the row's
// own data only: never on nb, nor on the slot the row occupies (batch invariance, include/kdstep.h).

// Split-KV decode attention of row b = blockIdx.z with the row's own length cur_dev[b], cache
// [HKV, smax, hdp] and partial block: k_attn_decode_part's split, but one workgroup serves up to
// AB_R query heads of a KV head (blockIdx.x = kv head x head group), so the chunk's K and V tiles
// are read once for the GQA group instead of once per query head (at nb = 16 the per-head form
// spent more of the step here than in the linears).  q / k_new / v_new are head-major over the
// batch ([H | HKV, nb, hdp]: what kd_qkv_split(B = 1, S = nb) writes).  The partials are laid out
// [nb * H, nch, HD + 2], so k_attn_decode_combine merges them on a grid of nb * H.
constexpr int AB_R = 8;
template <int HD>
__global__ void __launch_bounds__(NT) k_attn_decode_part_batch(const bf16* __restrict__ q, const bf16* __restrict__ k_new,
                                                               const bf16* __restrict__ v_new, bf16* __restrict__ kc,
                                                               bf16* __restrict__ vc, float* __restrict__ part, int H,
                                                               int HKV, int hdp, int smax, int nb,
                                                               const int* __restrict__ cur_dev, float scale) {
    __shared__ __attribute__((aligned(16))) float q_s[AB_R][HD];
    __shared__ float p_s[AB_R][CH];
    __shared__ float m_s[AB_R], l_s[AB_R];
    __shared__ float acc_s[AB_R][NT];
    const int R = H / HKV, ng = (R + AB_R - 1) / AB_R;
    const int kvh = blockIdx.x / ng, g8 = blockIdx.x - kvh * ng, c = blockIdx.y, b = blockIdx.z, nch = gridDim.y;
    const int h0 = kvh * R + g8 * AB_R, Rg = min(AB_R, R - g8 * AB_R);   // query heads [h0, h0 + Rg)
    const int n = cur_dev[b], j0 = c * CH;
    const size_t hstride = (size_t)nch * (HD + 2);
    float* pp = part + (((size_t)b * H + h0) * nch + c) * (HD + 2);   // head h0 + r: + r * hstride
    if (j0 >= n || n > smax) {   // empty chunk; a length outside [1, smax] touches no cache row
        for (int i = threadIdx.x; i < Rg * (HD + 2); i += NT) {
            const int r = i / (HD + 2), e = i - r * (HD + 2);
            pp[r * hstride + e] = e == 0 ? -INFINITY : 0.f;
        }
        return;
    }
    bf16* K = kc + ((size_t)b * HKV + kvh) * smax * hdp;
    bf16* V = vc + ((size_t)b * HKV + kvh) * smax * hdp;
    const bf16* kn = k_new + ((size_t)kvh * nb + b) * hdp;
    const bf16* vn = v_new + ((size_t)kvh * nb + b) * hdp;
    if (c == 0 && g8 == 0)
        for (int d = threadIdx.x; d < hdp; d += NT) {
            K[(size_t)(n - 1) * hdp + d] = kn[d];
            V[(size_t)(n - 1) * hdp + d] = vn[d];
        }
    // this thread's share of the V tile, issued before the scores: dim d of keys g, g + G, ...
    constexpr int G = NT / HD, NV = CH / G;
    const int d = threadIdx.x % HD, g = threadIdx.x / HD;
    const int jend = min(CH, n - j0);
    float vr[NV];
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        // every load unconditional (keys past the chunk's end re-read the row's own v_new): a load
        // under a lane-dependent branch waits for its own round trip, NV of them in a row
        const int jj = g + i * G, j = min(j0 + jj, n - 1);
        const bf16* src = j == n - 1 ? vn + d : V + (size_t)j * hdp + d;
        const float v = (float)*src;
        vr[i] = jj < jend ? v : 0.f;
    }
    for (int i = threadIdx.x; i < AB_R * HD; i += NT) {   // heads past Rg: zeros (computed, never stored)
        const int r = i / HD, dd = i - r * HD;
        q_s[r][dd] = r < Rg ? (float)q[((size_t)(h0 + r) * nb + b) * hdp + dd] : 0.f;
    }
    __syncthreads();
    // scores: key j0 + threadIdx/4, lane quarter (threadIdx & 3) covers HD/4 dims of every head
    constexpr int DQ = HD / 4;
    const int kj = j0 + (threadIdx.x >> 2), qd = (threadIdx.x & 3) * DQ;
    float a[AB_R];
#pragma unroll
    for (int r = 0; r < AB_R; ++r) a[r] = 0.f;
    {
        const int kjc = min(kj, n - 1);   // keys past n: the own row again, masked below
        const bf16* kr = (kjc == n - 1 ? kn : K + (size_t)kjc * hdp) + qd;
#pragma unroll
        for (int dd = 0; dd < DQ; dd += 8) {
            const bf16x8 k8 = *(const bf16x8*)(kr + dd);
#pragma unroll
            for (int r = 0; r < AB_R; ++r) {
                const f32x4 qa = *(const f32x4*)&q_s[r][qd + dd], qb = *(const f32x4*)&q_s[r][qd + dd + 4];
#pragma unroll
                for (int e = 0; e < 4; ++e) a[r] += qa[e] * (float)k8[e];
#pragma unroll
                for (int e = 0; e < 4; ++e) a[r] += qb[e] * (float)k8[4 + e];
            }
        }
    }
#pragma unroll
    for (int r = 0; r < AB_R; ++r) {
        a[r] += __shfl_xor(a[r], 1, 64);
        a[r] += __shfl_xor(a[r], 2, 64);
        if ((threadIdx.x & 3) == 0) p_s[r][threadIdx.x >> 2] = kj < n ? a[r] * scale : -INFINITY;
    }
    __syncthreads();
    // softmax of the chunk, one wave per head (lane = key): wave w takes heads w, w + 4
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    for (int r = w; r < AB_R; r += NT / 64) {
        const float s = p_s[r][lane];
        const float m = wave_max(s);   // key j0 is valid, so m is finite
        const float pv = j0 + lane < n ? __expf(s - m) : 0.f;
        const float l = wave_sum(pv);
        p_s[r][lane] = pv;
        if (lane == 0) { m_s[r] = m; l_s[r] = l; }
    }
    __syncthreads();
    float acc[AB_R];
#pragma unroll
    for (int r = 0; r < AB_R; ++r) acc[r] = 0.f;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        const int jj = g + i * G;
#pragma unroll
        for (int r = 0; r < AB_R; ++r) acc[r] += p_s[r][jj] * vr[i];
    }
#pragma unroll
    for (int r = 0; r < AB_R; ++r) acc_s[r][threadIdx.x] = acc[r];
    __syncthreads();
    for (int i = threadIdx.x; i < Rg * HD; i += NT) {
        const int r = i / HD, dd = i - r * HD;
        float tsum = 0.f;
#pragma unroll
        for (int k = 0; k < G; ++k) tsum += acc_s[r][k * HD + dd];
        pp[r * hstride + 2 + dd] = tsum;
        if (dd == 0) { pp[r * hstride] = m_s[r]; pp[r * hstride + 1] = l_s[r]; }
    }
}

// Skinny linear layer y[nb, N] = epilogue(x[nb, K] W[N, K]^T), nb <= 16, on
// v_mfma_f32_16x16x32_bf16 with the batch as the M dimension: the A fragment of lane l is 8 k of
// batch row l & 15 (rows >= nb are zero and never stored), the B fragment 8 contiguous k of weight
// row n0 + (l & 15): one 16-B global load per lane straight from the row-major weight, every
// weight element read once per launch, no LDS round trip.  D[row m] depends on A[row m] only, so a
// batch row's result does not depend on its neighbours.
// Workgroup (blockIdx.x, blockIdx.y = K slice): the slice of x ([16, slice] bf16, the RMSNorm
// applied when norm_w is given, rounded to bf16 as stage_x rounds) is staged in LDS once;
//   wave_n = 0  one 16-row weight tile per workgroup, its 4 waves interleave the slice's 32-k
//               steps and their accumulators are summed through LDS in wave order;
//   wave_n = 1  one tile per wave (the lm_head: enough tiles to fill the chip on their own).
// With ksplit > 1 the fp32 slice sums go to `part` [ksplit, NACC, 16, N] and
// k_gemv_batch_reduce adds them in slice order and applies the epilogue (no atomics).
constexpr int GB_ROWS = 16;         // the MFMA's M
constexpr int GB_MAX_STEPS = 48;    // 32-k steps per K slice: 16 x (1536 + 8) bf16 = 48.25 KiB of LDS
constexpr int GB_PAD = 8;           // bf16 per LDS row: rows 16 B apart in the banks
constexpr int GB_PF = 8;            // weight fragments per wave loaded ahead of the x staging

// ---- the 16-row slab of x, shared by k_gemv_batch and k_gemv_slabs (kd_gemv_rows): a row's bits
// are the same in both because this code is the same ----

// 1/rms of each of the slab's nb rows, over the whole row, into rstd_s: 16 lanes per row, the same
// order in every slot.  Ends on a barrier.
__device__ __forceinline__ void gb_row_rstd(const bf16* __restrict__ x, int64_t ldx, int nb, int K, float eps,
                                            float* rstd_s) {
    const int b = threadIdx.x >> 4, sub = threadIdx.x & 15;
    float ss = 0.f;
    if (b < nb) {
        const bf16* xr = x + (size_t)b * ldx;
#pragma unroll 8
        for (int k = sub * 8; k < K; k += 128) {
            const bf16x8 v = *(const bf16x8*)(xr + k);
#pragma unroll
            for (int e = 0; e < 8; ++e) ss += (float)v[e] * (float)v[e];
        }
    }
#pragma unroll
    for (int o = 8; o > 0; o >>= 1) ss += __shfl_xor(ss, o, 64);
    if (sub == 0) rstd_s[b] = rsqrtf(ss / K + eps);
    __syncthreads();
}

// Columns [kb, kb + slice_steps * 32) of the slab into xs ([16][slice_steps * 32 + GB_PAD] bf16), with
// norm_w as the RMSNorm output rounded to bf16; rows >= nb and the K tail are zeros.  Ends on a barrier.
__device__ __forceinline__ void gb_stage_slab(const bf16* __restrict__ x, int64_t ldx, int nb, int K, int kb,
                                              int slice_steps, const bf16* __restrict__ norm_w, float eps,
                                              float* rstd_s, bf16* xs) {
    if (norm_w) gb_row_rstd(x, ldx, nb, K, eps, rstd_s);
    const int cpr = slice_steps * 4, XLD = slice_steps * 32 + GB_PAD;   // 16-B chunks per staged row
    const bf16x8 zero8 = {};
#pragma unroll 4
    for (int idx = threadIdx.x; idx < GB_ROWS * cpr; idx += NT) {
        const int b = idx / cpr, c = idx - b * cpr, k = kb + c * 8;
        const bool in = b < nb && k < K;
        const int bc = min(b, nb - 1), kc8 = min(k, K - 8);   // the loads stay unconditional, inside x
        bf16x8 v = *(const bf16x8*)(x + (size_t)bc * ldx + kc8);
        if (norm_w) {
            const bf16x8 nw = *(const bf16x8*)(norm_w + kc8);
            const float rstd = rstd_s[bc];
#pragma unroll
            for (int e = 0; e < 8; ++e) v[e] = (bf16)((float)v[e] * rstd * (float)nw[e]);
        }
        *(bf16x8*)(xs + b * XLD + c * 8) = in ? v : zero8;
    }
    __syncthreads();
}

// The 4 waves' K shares of a tile, summed in wave order through red_s: true on wave 0, which then
// holds the sums.  The barrier inside also ends every wave's reads of xs and rstd_s.
template <int NACC>
__device__ __forceinline__ bool gb_wave_order_sum(f32x4 (&red_s)[NACC][NT / 64][64], int w, int lane, f32x4& acc0,
                                                  f32x4& acc1) {
    red_s[0][w][lane] = acc0;
    if constexpr (NACC == 2) red_s[1][w][lane] = acc1;
    __syncthreads();
    if (w != 0) return false;
    acc0 = ((red_s[0][0][lane] + red_s[0][1][lane]) + red_s[0][2][lane]) + red_s[0][3][lane];
    if constexpr (NACC == 2) acc1 = ((red_s[1][0][lane] + red_s[1][1][lane]) + red_s[1][2][lane]) + red_s[1][3][lane];
    return true;
}

// One D fragment (column n = lane & 15, slab row (lane >> 4) * 4 + r, global row row0 + that):
// through the epilogue into y when K is not split, else as slice ks of the partials
// [ksplit, NACC, rows16, N].
template <int EPI>
__device__ __forceinline__ void gb_store(const f32x4& acc0, const f32x4& acc1, int lane, int nb, size_t row0,
                                         int rows16, int n, int N, int ks, int ksplit,
                                         const bf16* __restrict__ extra, bf16* __restrict__ y,
                                         float* __restrict__ part) {
    constexpr int NACC = EPI == 3 ? 2 : 1;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int b = (lane >> 4) * 4 + r;
        if (b >= nb) continue;
        const size_t gr = row0 + b;
        if (ksplit == 1) {
            float v = acc0[r];
            if constexpr (EPI == 1) v += (float)extra[n];
            if constexpr (EPI == 2) v += (float)extra[gr * N + n];
            if constexpr (EPI == 3) v = silu_fast(acc0[r]) * acc1[r];
            y[gr * N + n] = (bf16)v;
        } else {
            part[(((size_t)ks * NACC) * rows16 + gr) * N + n] = acc0[r];
            if constexpr (EPI == 3) part[(((size_t)ks * NACC + 1) * rows16 + gr) * N + n] = acc1[r];
        }
    }
}

template <int EPI>
__global__ void __launch_bounds__(NT) k_gemv_batch(const bf16* __restrict__ x, int64_t ldx, const bf16* __restrict__ W,
                                                   int64_t ldw, const bf16* __restrict__ extra, bf16* __restrict__ y,
                                                   float* __restrict__ part, int nb, int N, int K, int I,
                                                   const bf16* __restrict__ norm_w, float eps, int wave_n,
                                                   int slice_steps, int ksplit) {
    extern __shared__ __attribute__((aligned(16))) unsigned char gb_smem[];
    constexpr int NACC = EPI == 3 ? 2 : 1;
    __shared__ float rstd_s[GB_ROWS];
    __shared__ f32x4 red_s[NACC][NT / 64][64];
    bf16* xs = (bf16*)gb_smem;
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63, ks = blockIdx.y;
    const int ksteps = (K + 31) >> 5;
    const int s_beg = ks * slice_steps, s_end = min(ksteps, s_beg + slice_steps);
    const int kb = s_beg * 32, XLD = slice_steps * 32 + GB_PAD;
    const bf16x8 zero8 = {};
    const int tile = wave_n ? blockIdx.x * (NT / 64) + w : blockIdx.x;
    const int col = lane & 15, kq = (lane >> 4) * 8;
    const int n = tile * 16 + col, nc = min(n, N - 1);   // rows past N: a valid row is read, nothing stored
    const bf16* r0 = W + (size_t)nc * ldw;
    const bf16* r1 = W + (size_t)(I + nc) * ldw;
    const int s_first = s_beg + (wave_n ? 0 : w), sst = wave_n ? 1 : NT / 64;
    // the weights do not wait for x: the wave's first GB_PF fragments are in flight while the norm
    // and the staging of x run (a K = 896 layer's whole share); loads past the share or the K tail
    // stay unconditional, on the row's first chunk, and are replaced by zeros
    bf16x8 pf0[GB_PF], pf1[EPI == 3 ? GB_PF : 1];
#pragma unroll
    for (int i = 0; i < GB_PF; ++i) {
        const int k = (s_first + i * sst) * 32 + kq;
        const bool in = s_first + i * sst < s_end && k < K;
        pf0[i] = *(const bf16x8*)(r0 + (in ? k : 0));
        if constexpr (EPI == 3) pf1[i] = *(const bf16x8*)(r1 + (in ? k : 0));
    }
    gb_stage_slab(x, ldx, nb, K, kb, slice_steps, norm_w, eps, rstd_s, xs);
    const bf16* xr = xs + col * XLD + kq - kb;
    f32x4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int i = 0; i < GB_PF; ++i) {
        const int s = s_first + i * sst;
        if (s < s_end) {   // wave-uniform
            const bool in = s * 32 + kq < K;
            const bf16x8 a = *(const bf16x8*)(xr + s * 32);
            acc0 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, in ? pf0[i] : zero8, acc0, 0, 0, 0);
            if constexpr (EPI == 3) acc1 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, in ? pf1[i] : zero8, acc1, 0, 0, 0);
        }
    }
#pragma unroll 4
    for (int s = s_first + GB_PF * sst; s < s_end; s += sst) {
        const int k = s * 32 + kq;
        const bool in = k < K;   // K tail (K % 32 != 0): the load stays unconditional, on the row's first chunk
        const bf16x8 a = *(const bf16x8*)(xr + s * 32);
        const bf16x8 l0 = *(const bf16x8*)(r0 + (in ? k : 0));
        acc0 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, in ? l0 : zero8, acc0, 0, 0, 0);
        if constexpr (EPI == 3) {
            const bf16x8 l1 = *(const bf16x8*)(r1 + (in ? k : 0));
            acc1 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, in ? l1 : zero8, acc1, 0, 0, 0);
        }
    }
    if (!wave_n && !gb_wave_order_sum(red_s, w, lane, acc0, acc1)) return;
    if (n >= N) return;
    gb_store<EPI>(acc0, acc1, lane, nb, 0, GB_ROWS, n, N, ks, ksplit, extra, y, part);
}

// Sum of the K slices in slice order, then the epilogue, over `rows` rows of partials
// [ksplit, NACC, rows16, N] (k_gemv_batch: rows16 = 16).  Grid (ceil(N / 256), >= rows): rows past
// `rows` exit.
template <int EPI>
__global__ void __launch_bounds__(NT) k_gemv_batch_reduce(const float* __restrict__ part, const bf16* __restrict__ extra,
                                                          bf16* __restrict__ y, int rows, int rows16, int N,
                                                          int ksplit) {
    constexpr int NACC = EPI == 3 ? 2 : 1;
    const int b = blockIdx.y, n = blockIdx.x * NT + threadIdx.x;
    if (b >= rows || n >= N) return;
    float a0 = 0.f, a1 = 0.f;
    for (int ks = 0; ks < ksplit; ++ks) {
        a0 += part[(((size_t)ks * NACC) * rows16 + b) * N + n];
        if constexpr (EPI == 3) a1 += part[(((size_t)ks * NACC + 1) * rows16 + b) * N + n];
    }
    float v = a0;
    if constexpr (EPI == 1) v += (float)extra[n];
    if constexpr (EPI == 2) v += (float)extra[(size_t)b * N + n];
    if constexpr (EPI == 3) v = silu_fast(a0) * a1;
    y[(size_t)b * N + n] = (bf16)v;
}

// k_gen_select for row b = blockIdx.x: its own logits row, sequence and length (gen_row) and V
// bytes of flags.
__global__ void __launch_bounds__(1024) k_gen_select_batch(const bf16* __restrict__ logits_all, int64_t ldl, int V,
                                                           int64_t* __restrict__ seq_all, int smax,
                                                           int* __restrict__ cur_dev, float penalty, int ngram,
                                                           uint8_t* __restrict__ flags_all, int64_t* __restrict__ out) {
    const int b = blockIdx.x;
    const GenRow r = gen_row(seq_all, smax, cur_dev);
    const int bi = gen_select_row(logits_all + (size_t)b * ldl, V, r.seq, r.len, penalty, ngram,
                                  flags_all + (size_t)b * V);
    if (threadIdx.x == 0) gen_row_store(r, smax, cur_dev, out, bi);
}

// cos/sin row of position cur_dev[b] - 1 (kept inside the table) into row b of [nb, hh] buffers.
__global__ void k_rope_rows(const float* __restrict__ cos_t, const float* __restrict__ sin_t, int hh, int rows,
                            const int* __restrict__ cur_dev, float* __restrict__ cos_rows, float* __restrict__ sin_rows) {
    const int b = blockIdx.x, pos = min(max(cur_dev[b] - 1, 0), rows - 1);
    for (int i = threadIdx.x; i < hh; i += blockDim.x) {
        cos_rows[(size_t)b * hh + i] = cos_t[(size_t)pos * hh + i];
        sin_rows[(size_t)b * hh + i] = sin_t[(size_t)pos * hh + i];
    }
}

// The EOS ids of kd_gen_finish, passed by value: a captured step replays with fixed arguments.
struct GenEos {
    int64_t id[KD_GEN_EOS_MAX];
    int n;
};

// One wave, lane b < nb owns row b: fin[b] latches the row's length at its first EOS token
// (compared as int64), live[0] = rows still at 0 (ballot + popcount; no atomics).
__global__ void __launch_bounds__(64) k_gen_finish(const int64_t* __restrict__ tok, const int* __restrict__ cur_dev,
                                                   int nb, GenEos eos, int* __restrict__ fin, int* __restrict__ live) {
    const int b = threadIdx.x;
    bool open = false;
    if (b < nb) {
        int f = fin[b];
        if (f == 0) {
            const int64_t t = tok[b];
            bool hit = false;
#pragma unroll
            for (int e = 0; e < KD_GEN_EOS_MAX; ++e) hit |= e < eos.n && t == eos.id[e];
            if (hit) {
                f = cur_dev[b];
                fin[b] = f;
            }
        }
        open = f == 0;
    }
    const unsigned long long m = __ballot(open);
    if (b == 0) live[0] = __popcll(m);
}


// ------------------------------------------- grouped prefill: the suffix rows of a chunk ----
// k_gemv_batch for rows > 16 (kd_gemv_rows): the workgroup of a wave_n = 0 plan loads its wave's
// share of the weight tile once -- at most GB_MAX_STEPS / 4 fragments per wave, kept in VGPRs
// (compile-time indices, wave-uniform guards) -- and loops over its 16-row slabs of x, staging
// each slab (and its norm) as k_gemv_batch does.  Every slab runs k_gemv_batch's arithmetic in
// k_gemv_batch's order (32-k steps interleaved over the waves in ascending order, wave-order LDS
// sum, slice-order K reduce, 16 lanes per row for the norm), so a row's result is bit-identical
// to kd_gemv_batch on that row alone.  The partials of a split K are [ksplit, NACC, rows16, N].
constexpr int GS_FR = GB_MAX_STEPS / (NT / 64);   // weight fragments per wave and operand
constexpr int GS_SLAB_GROUPS = 4;                 // workgroups per weight tile, each with every 4th slab

template <int EPI>
__global__ void __launch_bounds__(NT) k_gemv_slabs(const bf16* __restrict__ x, int64_t ldx, const bf16* __restrict__ W,
                                                   int64_t ldw, const bf16* __restrict__ extra, bf16* __restrict__ y,
                                                   float* __restrict__ part, int rows, int N, int K, int I,
                                                   const bf16* __restrict__ norm_w, float eps, int slice_steps,
                                                   int ksplit) {
    extern __shared__ __attribute__((aligned(16))) unsigned char gb_smem[];
    constexpr int NACC = EPI == 3 ? 2 : 1;
    __shared__ float rstd_s[GB_ROWS];
    __shared__ f32x4 red_s[NACC][NT / 64][64];
    bf16* xs = (bf16*)gb_smem;
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63, ks = blockIdx.y;
    const int ksteps = (K + 31) >> 5;
    const int s_beg = ks * slice_steps, s_end = min(ksteps, s_beg + slice_steps);
    const int kb = s_beg * 32, XLD = slice_steps * 32 + GB_PAD;
    const bf16x8 zero8 = {};
    const int col = lane & 15, kq = (lane >> 4) * 8;
    const int n = blockIdx.x * 16 + col, nc = min(n, N - 1);   // rows past N: a valid row is read, nothing stored
    const bf16* r0 = W + (size_t)nc * ldw;
    const bf16* r1 = W + (size_t)(I + nc) * ldw;
    const int s_first = s_beg + w, sst = NT / 64;
    // the wave's whole share of the weight tile, once per launch; loads past the share or the K
    // tail stay unconditional, on the row's first chunk, and are replaced by zeros
    bf16x8 f0[GS_FR], f1[EPI == 3 ? GS_FR : 1];
#pragma unroll
    for (int i = 0; i < GS_FR; ++i) {
        const int k = (s_first + i * sst) * 32 + kq;
        const bool in = s_first + i * sst < s_end && k < K;
        const bf16x8 l0 = *(const bf16x8*)(r0 + (in ? k : 0));
        f0[i] = in ? l0 : zero8;
        if constexpr (EPI == 3) {
            const bf16x8 l1 = *(const bf16x8*)(r1 + (in ? k : 0));
            f1[i] = in ? l1 : zero8;
        }
    }
    const int rows16 = (rows + GB_ROWS - 1) / GB_ROWS * GB_ROWS;
    const bf16* xr = xs + col * XLD + kq - kb;
    // slabs blockIdx.z, blockIdx.z + gridDim.z, ...: a slab is a chain of dependent round trips (norm,
    // staging, MFMA, LDS sum), so up to GS_SLAB_GROUPS workgroups per tile share a CU and overlap them
    for (int row0 = blockIdx.z * GB_ROWS; row0 < rows; row0 += gridDim.z * GB_ROWS) {
        const int nb = min(GB_ROWS, rows - row0);
        gb_stage_slab(x + (size_t)row0 * ldx, ldx, nb, K, kb, slice_steps, norm_w, eps, rstd_s, xs);
        f32x4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int i = 0; i < GS_FR; ++i) {
            const int s = s_first + i * sst;
            if (s < s_end) {   // wave-uniform
                const bf16x8 a = *(const bf16x8*)(xr + s * 32);
                acc0 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, f0[i], acc0, 0, 0, 0);
                if constexpr (EPI == 3) acc1 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, f1[i], acc1, 0, 0, 0);
            }
        }
        // the sum's barrier: every wave is done with xs and rstd_s before the next slab overwrites them, and
        // wave 0 passes the next slab's barriers before red_s is rewritten
        if (!gb_wave_order_sum(red_s, w, lane, acc0, acc1) || n >= N) continue;
        gb_store<EPI>(acc0, acc1, lane, nb, row0, rows16, n, N, ks, ksplit, extra, y, part);
    }
}

// Extend attention (kd_attn_extend): the ragged suffix rows of nb questions, each against its own
// cache prefix [0, base) plus its own suffix rows up to itself.  Workgroup (kv head, 64-key chunk,
// question): the chunk's K ([key][d]) and V (transposed, [d][key]) are staged in LDS once for all
// S x R query-head rows of the question (row m = suffix row m / R, head m % R of the GQA group);
// positions >= base come from k_new / v_new, never from the cache rows this launch writes (the
// workgroup that owns a position stores it), positions past the suffix are zeros.  The waves take
// the rows in tiles of 16 on v_mfma_f32_16x16x32_bf16 (operand layout of k_gemv_batch): Q K^T
// (M = rows, N = 64 keys, K = HD), the chunk softmax in fp32 with key <= position, P (rounded to
// bf16 through LDS; the row sum is taken over the rounded values) times V.  Partials
// [rows * H, nch, HD + 2] for k_attn_decode_combine; chunk boundaries, tiles and order depend on
// the question's own (base, S) only.
constexpr int AE_PAD = 8;   // bf16 per LDS row: rows 16 B apart in the banks

template <int HD>
__global__ void __launch_bounds__(NT) k_attn_extend_part(const bf16* __restrict__ q, const bf16* __restrict__ k_new,
                                                         const bf16* __restrict__ v_new, bf16* __restrict__ kc,
                                                         bf16* __restrict__ vc, float* __restrict__ part, int H,
                                                         int HKV, int hdp, int smax, int rows,
                                                         const int* __restrict__ row_start,
                                                         const int* __restrict__ base_dev, float scale) {
    __shared__ __attribute__((aligned(16))) bf16 k_s[CH][HD + AE_PAD];
    __shared__ __attribute__((aligned(16))) bf16 vt_s[HD][CH + AE_PAD];
    __shared__ __attribute__((aligned(16))) bf16 p_s[NT / 64][16][CH + AE_PAD];
    const int kvh = blockIdx.x, c = blockIdx.y, b = blockIdx.z, nch = gridDim.y;
    const int R = H / HKV, j0 = c * CH;
    const int rs0 = row_start[b], rs1 = row_start[b + 1], S = rs1 - rs0, base = base_dev[b];
    if (rs0 < 0 || rs1 > rows || S < 1) return;   // the question owns no row
    const int M = S * R;
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63, col = lane & 15, quad = lane >> 4;
    if (base < 0 || base > smax - S || j0 >= base + S) {   // no key of this chunk for any row (or no room in the cache)
        for (int i = threadIdx.x; i < M * (HD + 2); i += NT) {
            const int m = i / (HD + 2), e = i - m * (HD + 2), j = m / R, r = m - j * R;
            part[(((size_t)(rs0 + j) * H + kvh * R + r) * nch + c) * (HD + 2) + e] = e == 0 ? -INFINITY : 0.f;
        }
        return;
    }
    bf16* K = kc + ((size_t)b * HKV + kvh) * smax * hdp;
    bf16* V = vc + ((size_t)b * HKV + kvh) * smax * hdp;
    const bf16* kn = k_new + ((size_t)kvh * rows + rs0) * hdp;
    const bf16* vn = v_new + ((size_t)kvh * rows + rs0) * hdp;
    constexpr int C8 = HD / 8;
    for (int idx = threadIdx.x; idx < CH * C8; idx += NT) {
        const int key = idx / C8, c8 = idx - key * C8, p = j0 + key;
        bf16x8 k8 = {}, v8 = {};
        if (p < base) {
            k8 = *(const bf16x8*)(K + (size_t)p * hdp + c8 * 8);
            v8 = *(const bf16x8*)(V + (size_t)p * hdp + c8 * 8);
        } else if (p < base + S) {
            k8 = *(const bf16x8*)(kn + (size_t)(p - base) * hdp + c8 * 8);
            v8 = *(const bf16x8*)(vn + (size_t)(p - base) * hdp + c8 * 8);
        }
        *(bf16x8*)&k_s[key][c8 * 8] = k8;
#pragma unroll
        for (int e = 0; e < 8; ++e) vt_s[c8 * 8 + e][key] = v8[e];
    }
    {   // the suffix rows that fall into this chunk go into the caches (read by later launches only)
        const int hc = hdp / 8;
        for (int idx = threadIdx.x; idx < CH * hc; idx += NT) {
            const int key = idx / hc, c8 = idx - key * hc, p = j0 + key;
            if (p >= base && p < base + S) {
                *(bf16x8*)(K + (size_t)p * hdp + c8 * 8) = *(const bf16x8*)(kn + (size_t)(p - base) * hdp + c8 * 8);
                *(bf16x8*)(V + (size_t)p * hdp + c8 * 8) = *(const bf16x8*)(vn + (size_t)(p - base) * hdp + c8 * 8);
            }
        }
    }
    __syncthreads();
    const int ntile = (M + 15) / 16;
    for (int t0 = 0; t0 < ntile; t0 += NT / 64) {   // workgroup-uniform trip count (the barrier below)
        const int t = t0 + w, m0 = t * 16;
        const bool have = t < ntile;
        // this lane's rows of D: m0 + quad * 4 + r
        bool rv[4];
        int pos[4];
        size_t poff[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int m = m0 + quad * 4 + r, mc = min(m, M - 1), j = mc / R, rr = mc - j * R;
            rv[r] = have && m < M;
            pos[r] = base + j;
            poff[r] = (((size_t)(rs0 + j) * H + kvh * R + rr) * nch + c) * (HD + 2);
        }
        // a tile whose last row sits before the chunk has no key here (wave-uniform)
        const bool act = have && j0 <= base + min(m0 + 15, M - 1) / R;
        float mx[4] = {-INFINITY, -INFINITY, -INFINITY, -INFINITY}, ls[4] = {0.f, 0.f, 0.f, 0.f};
        if (act) {
            const int ma = min(m0 + col, M - 1), ja = ma / R, ra = ma - ja * R;   // the A fragment's row
            const bf16* qr = q + ((size_t)(kvh * R + ra) * rows + rs0 + ja) * hdp + quad * 8;
            bf16x8 qa[HD / 32];
#pragma unroll
            for (int kk = 0; kk < HD / 32; ++kk) qa[kk] = *(const bf16x8*)(qr + kk * 32);
            f32x4 sc[CH / 16];
#pragma unroll
            for (int nk = 0; nk < CH / 16; ++nk) {
                sc[nk] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int kk = 0; kk < HD / 32; ++kk) {
                    const bf16x8 kf = *(const bf16x8*)&k_s[nk * 16 + col][kk * 32 + quad * 8];
                    sc[nk] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(qa[kk], kf, sc[nk], 0, 0, 0);
                }
            }
#pragma unroll
            for (int r = 0; r < 4; ++r) {   // D: key nk * 16 + col, row quad * 4 + r; 16 lanes share a row
                float m = -INFINITY;
#pragma unroll
                for (int nk = 0; nk < CH / 16; ++nk) {
                    const float s = rv[r] && j0 + nk * 16 + col <= pos[r] ? sc[nk][r] * scale : -INFINITY;
                    sc[nk][r] = s;
                    m = fmaxf(m, s);
                }
#pragma unroll
                for (int o = 8; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
                float l = 0.f;
#pragma unroll
                for (int nk = 0; nk < CH / 16; ++nk) {
                    const bf16 pb = (bf16)(m == -INFINITY ? 0.f : __expf(sc[nk][r] - m));
                    l += (float)pb;
                    p_s[w][quad * 4 + r][nk * 16 + col] = pb;
                }
#pragma unroll
                for (int o = 8; o > 0; o >>= 1) l += __shfl_xor(l, o, 64);
                mx[r] = m;
                ls[r] = l;
            }
        }
        __syncthreads();   // p_s[w]: written in the D layout, read back as A fragments
        if (!have) continue;
        f32x4 oacc[HD / 16];
#pragma unroll
        for (int nd = 0; nd < HD / 16; ++nd) oacc[nd] = f32x4{0.f, 0.f, 0.f, 0.f};
        if (act) {
#pragma unroll
            for (int kk = 0; kk < CH / 32; ++kk) {
                const bf16x8 pa = *(const bf16x8*)&p_s[w][col][kk * 32 + quad * 8];
#pragma unroll
                for (int nd = 0; nd < HD / 16; ++nd) {
                    const bf16x8 vf = *(const bf16x8*)&vt_s[nd * 16 + col][kk * 32 + quad * 8];
                    oacc[nd] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(pa, vf, oacc[nd], 0, 0, 0);
                }
            }
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            if (!rv[r]) continue;
            float* pp = part + poff[r];
#pragma unroll
            for (int nd = 0; nd < HD / 16; ++nd) pp[2 + nd * 16 + col] = oacc[nd][r];
            if (col == 0) { pp[0] = mx[r]; pp[1] = ls[r]; }
        }
    }
}

// ------------------------------------- constrained decoding: an allowed set of token ids ----
// With allowed_token_ids the step needs the logits of the A allowed ids only (ids: ascending,
// unique int32 on the device), so the lm_head reads A weight rows instead of V and the choice
// searches A scores.  The gathered GEMVs are kernels of their own, not an index pointer threaded
// through k_gemv / k_gemv_batch (see k_gemv: an edit there reschedules its loop).  They repeat the
// full kernels' arithmetic on a row: in k_gemv a logit is one wave's sum over its own weight row,
// in k_gemv_batch under the lm_head plan (wave_n = 1, ksplit = 1) one whole-K MFMA chain whose
// column n reads weight row n only, so y[., j] has the bits the full head gives at column ids[j].
// An id outside [0, N_full) reads no weight and scores -inf.

// k_gemv (EPI 0, no norm) over weight rows ids[0 .. A): its dot-product loop, a third copy.
__global__ void __launch_bounds__(NT) k_gemv_gather(const bf16* __restrict__ x, const bf16* __restrict__ W, int64_t ldw,
                                                    const int* __restrict__ ids, int A, bf16* __restrict__ y,
                                                    int N_full, int K) {
    extern __shared__ float xs[];
    __shared__ float red[8];
    stage_x(x, nullptr, 0.f, K, xs, red);
    const int j = blockIdx.x * (NT / 64) + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (j >= A) return;
    const int n = ids[j];
    if ((unsigned)n >= (unsigned)N_full) {
        if (lane == 0) y[j] = (bf16)(-INFINITY);
        return;
    }
    const bf16* r0 = W + (size_t)n * ldw;
    float a0 = 0.f;
    for (int k = lane * 8; k < K; k += 512) {
        const bf16x8 w0 = *(const bf16x8*)(r0 + k);
#pragma unroll
        for (int e = 0; e < 8; ++e) a0 += xs[k + e] * (float)w0[e];
    }
    a0 = wave_sum(a0);
    if (lane == 0) y[j] = (bf16)a0;
}

// k_gemv_batch's wave_n = 1, ksplit = 1 plan (EPI 0, no norm) over 16-row tiles of the gathered
// rows: tile t of wave (blockIdx.x, w) holds weight rows ids[16 t .. 16 t + 16), y is [nb, A].
// Same slab staging (gb_stage_slab), same ascending 32-k chain per wave, so batch invariant as
// k_gemv_batch is.
__global__ void __launch_bounds__(NT) k_gemv_batch_gather(const bf16* __restrict__ x, int64_t ldx,
                                                          const bf16* __restrict__ W, int64_t ldw,
                                                          const int* __restrict__ ids, int A, bf16* __restrict__ y,
                                                          int nb, int N_full, int K) {
    extern __shared__ __attribute__((aligned(16))) unsigned char gb_smem[];
    __shared__ float rstd_s[GB_ROWS];   // gb_stage_slab's norm scratch: not touched without norm_w
    bf16* xs = (bf16*)gb_smem;
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int ksteps = (K + 31) >> 5, XLD = ksteps * 32 + GB_PAD;
    const bf16x8 zero8 = {};
    const int tile = blockIdx.x * (NT / 64) + w;
    const int col = lane & 15, kq = (lane >> 4) * 8;
    const int j = tile * 16 + col, id = ids[min(j, A - 1)];   // entries past A: a valid entry is read, nothing stored
    const bool id_ok = (unsigned)id < (unsigned)N_full;
    const bf16* r0 = W + (size_t)(id_ok ? id : 0) * ldw;
    // k_gemv_batch's loop: the first GB_PF fragments in flight while x is staged, then the rest; loads
    // past the K tail stay unconditional, on the row's first chunk, and are replaced by zeros.  (All
    // ksteps fragments loaded up front, 236 VGPRs, measured the same 14 us per launch at A = 500.)
    bf16x8 pf0[GB_PF];
#pragma unroll
    for (int i = 0; i < GB_PF; ++i) {
        const int k = i * 32 + kq;
        const bool in = i < ksteps && k < K;
        pf0[i] = *(const bf16x8*)(r0 + (in ? k : 0));
    }
    gb_stage_slab(x, ldx, nb, K, 0, ksteps, nullptr, 0.f, rstd_s, xs);
    const bf16* xr = xs + col * XLD + kq;
    f32x4 acc0 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int i = 0; i < GB_PF; ++i) {
        if (i < ksteps) {   // uniform
            const bool in = i * 32 + kq < K;
            const bf16x8 a = *(const bf16x8*)(xr + i * 32);
            acc0 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, in ? pf0[i] : zero8, acc0, 0, 0, 0);
        }
    }
#pragma unroll 4
    for (int s = GB_PF; s < ksteps; ++s) {
        const int k = s * 32 + kq;
        const bool in = k < K;
        const bf16x8 a = *(const bf16x8*)(xr + s * 32);
        const bf16x8 l0 = *(const bf16x8*)(r0 + (in ? k : 0));
        acc0 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, in ? l0 : zero8, acc0, 0, 0, 0);
    }
    if (j >= A) return;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int b = (lane >> 4) * 4 + r;
        if (b < nb) y[(size_t)b * A + j] = id_ok ? (bf16)acc0[r] : (bf16)(-INFINITY);
    }
}

// Entry of the ascending ids[0 .. A) that equals t, or -1.  (Searching a copy of the ids in LDS
// took the kernel from 9.5 to 7.8 us at A = 500, 16 rows: not worth a second path.)
__device__ __forceinline__ int ids_find(const int* __restrict__ ids, int A, int64_t t) {
    int lo = 0, hi = A;   // the first entry >= t lies in [lo, hi]
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if ((int64_t)ids[mid] < t) lo = mid + 1;
        else hi = mid;
    }
    return lo < A && (int64_t)ids[lo] == t ? lo : -1;
}

// The flag pass of k_gen_select_ids over the A allowed entries (flags in LDS), shared with the
// sampling kernel (k_gen_sample): ends on a barrier.  (Its three-line penalty loop stays its own.)
__device__ __forceinline__ void gen_flags_ids(const int* __restrict__ ids, int A, const int64_t* __restrict__ seq,
                                              int len, float penalty, int ngram, uint8_t* flags) {
    for (int i = threadIdx.x; i < A; i += blockDim.x) flags[i] = 0;
    __syncthreads();
    if (penalty != 1.0f)
        for (int i = threadIdx.x; i < len; i += blockDim.x) {
            const int j = ids_find(ids, A, seq[i]);
            if (j >= 0) flags[j] = 1;
        }
    __syncthreads();   // the two processors set different bits of the same bytes
    gen_ngram_scan(seq, len, ngram, [&](int64_t t) {
        const int j = ids_find(ids, A, t);
        if (j >= 0) flags[j] |= 2;
    });
    __syncthreads();
}

// k_gen_select_batch over compact scores [nb, A] (column j: token ids[j]): row b = blockIdx.x.  The
// flags (bit 0 = seen, bit 1 = banned) are kept per allowed entry in LDS, and every id of the
// sequence is looked up in ids by binary search (a miss touches nothing), so the cost follows A
// and the row's length, never V.  Ascending ids: the lowest entry on a tie is the lowest id.  No
// finite allowed score: token 0, as the argmax of an all -inf row of V logits.
__global__ void __launch_bounds__(1024) k_gen_select_ids(const bf16* __restrict__ scores_all, int64_t lds,
                                                         const int* __restrict__ ids, int A,
                                                         int64_t* __restrict__ seq_all, int smax,
                                                         int* __restrict__ cur_dev, float penalty, int ngram,
                                                         int64_t* __restrict__ out) {
    __shared__ uint8_t flags[KD_GEN_ALLOWED_MAX];
    const GenRow r = gen_row(seq_all, smax, cur_dev);
    const bf16* scores = scores_all + (size_t)blockIdx.x * lds;
    gen_flags_ids(ids, A, r.seq, r.len, penalty, ngram, flags);
    float best = -INFINITY;
    int bj = 0x7fffffff;
    for (int j = threadIdx.x; j < A; j += blockDim.x) {
        const float s = gen_processed((float)scores[j], flags[j], penalty);
        if (s > best || (s == best && j < bj)) { best = s; bj = j; }   // NaN never wins
    }
    bj = gen_block_argmax(best, bj);
    // best == -inf: every allowed entry is banned, -inf or NaN (bj is then some entry or none at all)
    if (threadIdx.x == 0) gen_row_store(r, smax, cur_dev, out, best == -INFINITY ? 0 : (int64_t)ids[bj]);
}

// --------------------------------------------------------------- sampling (do_sample=True) ----
// k_gen_sample draws row b = blockIdx.x's token from the processed scores of the select kernels
// (their flag passes and gen_processed), then temperature, top-k, top-p and one Philox draw
// (include/kdstep.h states the semantics).  One workgroup of 1024 threads owns the row, so the
// grid is the batch and nothing a row computes can depend on nb or on its slot.  Every sum is an
// integer sum: a weight exp(t - max) becomes floor(w * 2^40) once (N <= 2^18 of them stay below
// 2^58), so Z, the top-p masses and the cumulative walk are exact in any order, and the 8-bit
// radix-select histograms are integer LDS atomics (GS_COPIES padded copies, chosen by the lane:
// logits crowd into a few exponent bins, and one copy would serialise the wave on them).
// Passes over the row, which stays in the workspace (t fp32, q = fixed-point weights, 256-id tile sums):
//   1  processed scores / T -> t, the row maximum, the top-k count histogram of the keys' top byte
//   2-4  (top-k)  the next three bytes of the k-th largest key, over the entries under its prefix
//   5  q for the entries top-k kept, Z, the top-p mass histogram of the top byte
//   6-8  (top-p)  the next three bytes of the cut's key (masses of the entries under its prefix)
//   9  tile sums of the kept q; the tile, then the id inside it, that the draw's target falls in
constexpr int GS_TILE = 256;     // ids per tile sum: 64 lanes x 4
constexpr int GS_COPIES = 16;    // histogram copies
constexpr int GS_HLD = 257;      // 64-bit words per copy: copy c of a bin sits c banks (of 8 B) further
typedef unsigned long long u64;
typedef __attribute__((ext_vector_type(2))) unsigned long long u64x2;

struct GsLayout {   // one row's workspace: every part 16-byte aligned
    size_t npad, tiles, q_off, tsum_off, t_off, flags_off, row_bytes;
};
__host__ __device__ inline GsLayout gs_layout(int N) {
    GsLayout l;
    l.npad = ((size_t)N + GS_TILE - 1) / GS_TILE * GS_TILE;
    l.tiles = l.npad / GS_TILE;
    l.q_off = 0;
    l.tsum_off = l.npad * 8;
    l.t_off = l.tsum_off + (l.tiles + 1) / 2 * 16;
    l.flags_off = l.t_off + l.npad * 4;
    l.row_bytes = (l.flags_off + l.npad + 255) / 256 * 256;
    return l;
}

// Order-preserving key of a float that is not NaN (-inf lowest).
__device__ __forceinline__ uint32_t gs_key(float t) {
    const uint32_t b = __float_as_uint(t);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}

// Word 0 of Philox4x32-10 at counter (c0, stream lo, stream hi, 0) under key (seed lo, seed hi).
__device__ __forceinline__ uint32_t gs_philox(uint64_t seed, uint32_t c0, uint64_t stream) {
    uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
    uint32_t c1 = (uint32_t)stream, c2 = (uint32_t)(stream >> 32), c3 = 0u;
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint32_t h0 = __umulhi(0xD2511F53u, c0), l0 = 0xD2511F53u * c0;
        const uint32_t h1 = __umulhi(0xCD9E8D57u, c2), l1 = 0xCD9E8D57u * c2;
        c0 = h1 ^ c1 ^ k0;
        c1 = l1;
        c2 = h0 ^ c3 ^ k1;
        c3 = l0;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    return c0;
}

__device__ __forceinline__ u64 gs_wave_sum(u64 v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ u64 gs_wave_scan(u64 v) {   // inclusive, ascending lanes
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const u64 n = __shfl_up(v, o, 64);
        if (lane >= o) v += n;
    }
    return v;
}
__device__ __forceinline__ void gs_hist_clear(u64* hist) {
    for (int i = threadIdx.x; i < GS_COPIES * GS_HLD; i += blockDim.x) hist[i] = 0;
    __syncthreads();
}
__device__ __forceinline__ void gs_hist_add(u64* hist, uint32_t digit, u64 v) {
    atomicAdd(&hist[(threadIdx.x & (GS_COPIES - 1)) * GS_HLD + digit], v);
}

// f(i4, t[4 * i4 .. 4 * i4 + 3]) over the row, four 16-byte loads per thread in flight: one workgroup
// reads the whole row, and with one load per thread a pass waits for 150 round trips in a row.
// The trip count is the workgroup's, and i4 < nvec is wave-uniform (nvec is a multiple of 64).
constexpr int GS_UNROLL = 4;
template <typename F>
__device__ __forceinline__ void gs_for_each4(const float* __restrict__ t, int npad, F f) {
    const int nvec = npad / 4, nt = blockDim.x;
    for (int base = threadIdx.x; base < nvec; base += GS_UNROLL * nt) {
        f32x4 tv[GS_UNROLL];
#pragma unroll
        for (int k = 0; k < GS_UNROLL; ++k) tv[k] = ((const f32x4*)t)[min(base + k * nt, nvec - 1)];
#pragma unroll
        for (int k = 0; k < GS_UNROLL; ++k)
            if (base + k * nt < nvec) f(base + k * nt, tv[k]);
    }
}

// Radix select, most significant byte first, over the keys of t [npad]: the largest key K such
// that the entries with a key >= K weigh at least `target` (an entry weighs 1, or its q with
// MASS); `kept` = what they weigh.  That is the k-th largest key (target = k), and with masses the
// smallest key whose strictly larger entries weigh less than target (the top-p cut).  The caller
// has filled hist with the first byte's histogram; the other three bytes take one pass each over
// the entries under the prefix found so far.  A target above the whole weight selects the lowest
// occupied key.  Every thread returns the same values.
template <bool MASS>
__device__ __forceinline__ uint32_t gs_radix_select(const float* __restrict__ t, const u64* __restrict__ q, int npad,
                                                    u64 target, u64* hist, u64* tot, u64* sel, u64& kept) {
    uint32_t prefix = 0;
    u64 above = 0;   // weight of the entries above the prefix
    for (int level = 0; level < 4; ++level) {
        const int shift = 24 - 8 * level;
        if (level > 0) {
            gs_hist_clear(hist);
            gs_for_each4(t, npad, [&](int i4, const f32x4& tv) {
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const uint32_t key = gs_key(tv[e]);
                    if ((key >> (shift + 8)) != prefix) continue;
                    const u64 v = MASS ? q[i4 * 4 + e] : 1ull;
                    if (v) gs_hist_add(hist, (key >> shift) & 255u, v);
                }
            });
        }
        __syncthreads();
        if (threadIdx.x < 256) {
            u64 s = 0;
#pragma unroll
            for (int c = 0; c < GS_COPIES; ++c) s += hist[c * GS_HLD + threadIdx.x];
            tot[threadIdx.x] = s;
        }
        __syncthreads();
        if (threadIdx.x < 64) {   // lane l: bins 255 - 4l ... 252 - 4l, the largest first
            const int lane = threadIdx.x;
            u64 v[4], ls = 0;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                v[e] = tot[255 - 4 * lane - e];
                ls += v[e];
            }
            const u64 incl = gs_wave_scan(ls), total = __shfl(incl, 63, 64);
            const u64 want = target < total ? target : total;
            u64 run = incl - ls;
            if (total == 0) {
                if (lane == 0) { sel[0] = 0; sel[1] = 1; sel[2] = above; sel[3] = 0; }
            } else if (run < want && incl >= want) {   // one lane: incl never decreases
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    if (run < want && run + v[e] >= want) {
                        sel[0] = 255 - 4 * lane - e;
                        sel[1] = want - run;
                        sel[2] = above + run;
                        sel[3] = v[e];
                    }
                    run += v[e];
                }
            }
        }
        __syncthreads();
        prefix = (prefix << 8) | (uint32_t)sel[0];
        target = sel[1];
        above = sel[2];
        kept = above + sel[3];
        __syncthreads();   // sel and hist are rewritten by the next level
    }
    return prefix;
}

template <bool IDS>
__global__ void __launch_bounds__(1024) k_gen_sample(const bf16* __restrict__ scores_all, int64_t lds, int N,
                                                     const int* __restrict__ ids, int64_t* __restrict__ seq_all,
                                                     int smax, int* __restrict__ cur_dev, float penalty, int ngram,
                                                     float temperature, int top_k, float top_p, uint64_t seed,
                                                     const int64_t* __restrict__ streams, unsigned char* __restrict__ ws,
                                                     int64_t* __restrict__ out, float* __restrict__ u_out) {
    __shared__ u64 hist[GS_COPIES * GS_HLD];
    __shared__ u64 tot[256];
    __shared__ u64 sel[4];
    __shared__ u64 wsum[16];
    __shared__ float red[16];
    __shared__ __attribute__((aligned(16))) uint8_t flags_s[IDS ? KD_GEN_ALLOWED_MAX : 16];
    const int b = blockIdx.x, lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const GsLayout lay = gs_layout(N);
    const int npad = (int)lay.npad;
    unsigned char* row = ws + (size_t)b * lay.row_bytes;
    u64* q = (u64*)(row + lay.q_off);
    u64* tsum = (u64*)(row + lay.tsum_off);
    float* t = (float*)(row + lay.t_off);
    uint8_t* flags = IDS ? flags_s : row + lay.flags_off;
    const GenRow r = gen_row(seq_all, smax, cur_dev);
    const int len = r.len;
    const bf16* scores = scores_all + (size_t)b * lds;
    if constexpr (IDS) gen_flags_ids(ids, N, r.seq, len, penalty, ngram, flags);
    else gen_flags_row(N, r.seq, len, penalty, ngram, flags);

    // ---- pass 1
    const bool use_k = top_k >= 1 && top_k < N;
    if (use_k) gs_hist_clear(hist);
    float mx = -INFINITY;
    auto first = [&](float s, uint32_t f) {
        float v = __fdiv_rn(gen_processed(s, f, penalty), temperature);
        if (!(v == v)) v = -INFINITY;   // NaN is never chosen
        if (v == 0.f) v = 0.f;          // -0 and +0 tie: one key
        mx = fmaxf(mx, v);
        if (use_k) gs_hist_add(hist, gs_key(v) >> 24, 1ull);
        return v;
    };
    const int v8 = (((uintptr_t)scores & 15) == 0 && ((uintptr_t)flags & 7) == 0) ? N >> 3 : 0;
    for (int base = threadIdx.x; base < v8; base += GS_UNROLL * blockDim.x) {
        bf16x8 lv[GS_UNROLL];
        u32x2 fv[GS_UNROLL];
#pragma unroll
        for (int k = 0; k < GS_UNROLL; ++k) {
            const int c = min(base + k * (int)blockDim.x, v8 - 1);
            lv[k] = ((const bf16x8*)scores)[c];
            fv[k] = ((const u32x2*)flags)[c];
        }
#pragma unroll
        for (int k = 0; k < GS_UNROLL; ++k) {
            const int c = base + k * (int)blockDim.x;
            if (c >= v8) continue;
            f32x4 lo, hi;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                lo[e] = first((float)lv[k][e], (fv[k].x >> (8 * e)) & 255u);
                hi[e] = first((float)lv[k][4 + e], (fv[k].y >> (8 * e)) & 255u);
            }
            ((f32x4*)t)[2 * c] = lo;
            ((f32x4*)t)[2 * c + 1] = hi;
        }
    }
    for (int i = (v8 << 3) + threadIdx.x; i < N; i += blockDim.x) t[i] = first((float)scores[i], flags[i]);
    for (int i = N + threadIdx.x; i < npad; i += blockDim.x) {   // the padding: -inf, weight 0
        t[i] = -INFINITY;
        if (use_k) gs_hist_add(hist, gs_key(-INFINITY) >> 24, 1ull);
    }
    mx = block_max<16>(mx, red);   // its barriers publish t and hist to the workgroup

    // u: Philox at the position the token is written to
    const uint32_t m24 = gs_philox(seed, (uint32_t)len, (uint64_t)streams[b]) >> 8;
    int64_t token = 0;
    if (mx > -INFINITY) {   // else no score above -inf: token 0, the greedy kernels' rule
        u64 kept = 0;
        uint32_t thr = 0;
        if (use_k) thr = gs_radix_select<false>(t, q, npad, (u64)top_k, hist, tot, sel, kept);

        // ---- pass 5: the fixed-point weights of what top-k kept
        const bool use_p = top_p < 1.0f;
        if (use_p) gs_hist_clear(hist);
        u64 z = 0;
        gs_for_each4(t, npad, [&](int i4, const f32x4& tv) {
            u64 qv[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const uint32_t key = gs_key(tv[e]);
                qv[e] = 0ull;
                if (key >= thr) {   // few entries behind a top-k: the exp is theirs alone
                    const float w = tv[e] == mx ? 1.0f : expf(tv[e] - mx);
                    qv[e] = (u64)(w * 1099511627776.0f);
                }
                z += qv[e];
                if (use_p && qv[e]) gs_hist_add(hist, key >> 24, qv[e]);
            }
            ((u64x2*)q)[2 * i4] = u64x2{qv[0], qv[1]};
            ((u64x2*)q)[2 * i4 + 1] = u64x2{qv[2], qv[3]};
        });
        z = gs_wave_sum(z);
        if (lane == 0) wsum[wv] = z;
        __syncthreads();   // also publishes q and hist
        z = 0;
#pragma unroll
        for (int i = 0; i < 16; ++i) z += wsum[i];
        if (use_p) {
            // keep j iff the mass strictly above it is < top_p * Z, i.e. < ceil(top_p * Z)
            const double pd = ceil((double)top_p * (double)z);
            u64 target = (u64)pd;
            target = target < 1 ? 1 : (target > z ? z : target);
            thr = gs_radix_select<true>(t, q, npad, target, hist, tot, sel, z);
        }
        __syncthreads();   // wsum is reused below

        // ---- pass 9: tile sums of the kept weights, then the tile and the id of the draw
        {
            const int nvec = npad / 4, nt = blockDim.x;
            for (int base = threadIdx.x; base < nvec; base += GS_UNROLL * nt) {
                f32x4 tv[GS_UNROLL];
                u64x2 qa[GS_UNROLL], qb[GS_UNROLL];
#pragma unroll
                for (int k = 0; k < GS_UNROLL; ++k) {
                    const int i4 = min(base + k * nt, nvec - 1);
                    tv[k] = ((const f32x4*)t)[i4];
                    qa[k] = ((const u64x2*)q)[2 * i4];
                    qb[k] = ((const u64x2*)q)[2 * i4 + 1];
                }
#pragma unroll
                for (int k = 0; k < GS_UNROLL; ++k) {
                    const int i4 = base + k * nt;
                    if (i4 >= nvec) continue;   // wave-uniform
                    u64 s = 0;
                    s += gs_key(tv[k][0]) >= thr ? qa[k].x : 0ull;
                    s += gs_key(tv[k][1]) >= thr ? qa[k].y : 0ull;
                    s += gs_key(tv[k][2]) >= thr ? qb[k].x : 0ull;
                    s += gs_key(tv[k][3]) >= thr ? qb[k].y : 0ull;
                    s = gs_wave_sum(s);
                    if (lane == 0) tsum[i4 >> 6] = s;
                }
            }
        }
        if (threadIdx.x == 0) sel[0] = sel[1] = sel[2] = 0;   // Z > 0 (the maximum is kept), so all three are set below
        __syncthreads();
        // smallest j with C_j > u * Z  <=>  C_j > floor(m24 * Z / 2^24); Z is the kept weight, C_last = Z
        const u64 target = (__umul64hi((u64)m24, z) << 40) | (((u64)m24 * z) >> 24);
        const int tiles = npad / GS_TILE;
        u64 base = 0;
        for (int c0 = 0; c0 < tiles; c0 += 1024) {
            const int ti = c0 + threadIdx.x;
            const u64 v = ti < tiles ? tsum[ti] : 0ull;
            const u64 incl = gs_wave_scan(v);
            if (lane == 63) wsum[wv] = incl;
            __syncthreads();
            u64 off = base, all = 0;
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                if (i < wv) off += wsum[i];
                all += wsum[i];
            }
            const u64 cj = off + incl;
            if (cj > target && cj - v <= target) {   // one thread of one chunk: cj never decreases
                sel[0] = (u64)ti;
                sel[1] = cj - v;
            }
            base += all;
            __syncthreads();
        }
        if (wv == 0) {
            const int i4 = (int)sel[0] * 64 + lane;
            const f32x4 tv = ((const f32x4*)t)[i4];
            const u64x2 qa = ((const u64x2*)q)[2 * i4], qb = ((const u64x2*)q)[2 * i4 + 1];
            u64 qv[4] = {qa.x, qa.y, qb.x, qb.y}, s = 0;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                if (gs_key(tv[e]) < thr) qv[e] = 0;
                s += qv[e];
            }
            const u64 incl = sel[1] + gs_wave_scan(s);
            if (incl > target && incl - s <= target) {
                u64 run = incl - s;
                int j = i4 * 4;
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    if (run <= target && run + qv[e] > target) j = i4 * 4 + e;
                    run += qv[e];
                }
                sel[2] = (u64)j;
            }
        }
        __syncthreads();
        const int j = (int)sel[2];
        token = IDS ? (int64_t)ids[j] : (int64_t)j;
    }
    if (threadIdx.x == 0) {
        gen_row_store(r, smax, cur_dev, out, token);
        if (u_out) u_out[b] = (float)m24 * 5.9604644775390625e-08f;
    }
}

// ------------------------------------------------------------ beam search (num_beams > 1) ----
// transformers' _beam_search (do_sample=False, early_stopping=False) as three launches per step
// (include/kdstep.h states the semantics): k_gen_beam_topk, one workgroup per beam row, leaves the
// row's M best accumulated log-probabilities; k_gen_beam_step, one workgroup per prompt, merges its
// K rows' lists and keeps the running and the finished hypotheses; k_kv_beam_reorder permutes the
// generated tail of the K/V cache by parent beam.  Rows are beams: slot p * K + j is beam j of
// prompt p, and nothing a prompt's workgroups compute depends on the other prompts of the call.
constexpr int BM_M_MAX = 72;   // candidates per row: max(2, 1 + KD_GEN_EOS_MAX) * KD_GEN_BEAMS_MAX
constexpr float BM_KILL = -1.0e9f;

struct BtLayout {   // one row's workspace of k_gen_beam_topk: the fp32 row of accumulated scores, then the flags
    size_t npad, flags_off, row_bytes;
};
__host__ __device__ inline BtLayout bt_layout(int V) {
    BtLayout l;
    l.npad = ((size_t)V + GS_TILE - 1) / GS_TILE * GS_TILE;
    l.flags_off = l.npad * 4;
    l.row_bytes = (l.flags_off + l.npad + 255) / 256 * 256;
    return l;
}

// f(i, logit i, flags i) over a row, 8 logits and 8 flags per load where both are aligned
// (k_gen_sample's first pass), GS_UNROLL loads in flight.  FLAGS = false: the flag bytes are not read
// (f gets 0): the maximum and the Z pass need the logits alone.
template <bool FLAGS, typename F>
__device__ __forceinline__ void bt_for_each(const bf16* __restrict__ scores, const uint8_t* __restrict__ flags, int N,
                                            F f) {
    const int nt = blockDim.x;
    const int v8 = (((uintptr_t)scores & 15) == 0 && ((uintptr_t)flags & 7) == 0) ? N >> 3 : 0;
    for (int base = threadIdx.x; base < v8; base += GS_UNROLL * nt) {
        bf16x8 lv[GS_UNROLL];
        u32x2 fv[GS_UNROLL];
#pragma unroll
        for (int k = 0; k < GS_UNROLL; ++k) {
            const int c = min(base + k * nt, v8 - 1);
            lv[k] = ((const bf16x8*)scores)[c];
            fv[k] = FLAGS ? ((const u32x2*)flags)[c] : u32x2{0u, 0u};
        }
#pragma unroll
        for (int k = 0; k < GS_UNROLL; ++k) {
            const int c = base + k * nt;
            if (c >= v8) continue;
#pragma unroll
            for (int e = 0; e < 8; ++e) f(c * 8 + e, (float)lv[k][e], ((e < 4 ? fv[k].x : fv[k].y) >> (8 * (e & 3))) & 255u);
        }
    }
    for (int i = (v8 << 3) + threadIdx.x; i < N; i += nt) f(i, (float)scores[i], FLAGS ? (uint32_t)flags[i] : 0u);
}

// A row's logsumexp over every logit that is not NaN, the one copy k_gen_beam_topk and k_score_rows
// share: mx = the largest such logit, Z = the integer sum of floor(exp(s - mx) * 2^40) (the maximum
// itself weighs 2^40), the same in every thread whatever order the waves ran in.  dead: nothing above
// -inf (lse is then 0 and means nothing).  1024 threads; red and wsum: 16 LDS words each.  flags only
// decides, with the row's own alignment, where bt_for_each takes its 16-byte loads.
struct BtLse {
    float mx, lse;
    bool dead;
};
__device__ __forceinline__ BtLse bt_row_lse(const bf16* __restrict__ logits, const uint8_t* __restrict__ flags, int V,
                                            float* red, u64* wsum) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    float mx = -INFINITY;
    bt_for_each<false>(logits, flags, V, [&](int, float s, uint32_t) { mx = fmaxf(mx, s); });   // fmaxf drops a NaN
    mx = block_max<16>(mx, red);
    const bool dead = !(mx > -INFINITY);
    u64 z = 0;
    if (!dead)
        bt_for_each<false>(logits, flags, V, [&](int, float s, uint32_t) {
            if (s == s) z += (u64)((s == mx ? 1.0f : expf(s - mx)) * 1099511627776.0f);
        });
    z = gs_wave_sum(z);
    if (lane == 0) wsum[wv] = z;
    __syncthreads();
    z = 0;
#pragma unroll
    for (int i = 0; i < 16; ++i) z += wsum[i];
    // Z >= 2^40 (the maximum weighs 1): log in double, one rounding to fp32, one more for the sum
    const float lse = dead ? 0.f : __fadd_rn(mx, (float)(log((double)z) - 40.0 * 0.69314718055994530942));
    return {mx, lse, dead};
}

// Row b = blockIdx.x: acc_i = processed(logit_i - lse) + run_score[b] over the full vocabulary, and
// its M largest (acc, token) pairs, descending, the lower token first among equals.  lse is order
// free: the row maximum, then the integer sum of floor(exp(s - max) * 2^40) (k_gen_sample's fixed
// point), so every thread holds the same Z whatever order the waves ran in.  flags: bit 0 / 1 of
// gen_flags_row, bit 2 = the id is allowed (with ids).  The M-th largest key comes from
// k_gen_sample's radix select; the entries above it are collected in any order, the entries equal
// to it in ascending token order until M are held, and a rank sort of the M pairs orders them.
// An entry at -inf (banned, not allowed, NaN, or a dead row) is reported as (-inf, 0).
__global__ void __launch_bounds__(1024) k_gen_beam_topk(const bf16* __restrict__ logits_all, int64_t ldl, int V,
                                                        const int* __restrict__ ids, int A,
                                                        int64_t* __restrict__ seq_all, int smax,
                                                        const int* __restrict__ cur_dev,
                                                        const float* __restrict__ run_score, float penalty, int ngram,
                                                        int M, unsigned char* __restrict__ ws,
                                                        float* __restrict__ cand_score, int* __restrict__ cand_tok) {
    __shared__ u64 hist[GS_COPIES * GS_HLD];
    __shared__ u64 tot[256];
    __shared__ u64 sel[4];
    __shared__ u64 wsum[16];
    __shared__ float red[16];
    __shared__ float top_s[BM_M_MAX];
    __shared__ int top_t[BM_M_MAX];
    __shared__ int wcnt[16];
    __shared__ int cnt;
    const int b = blockIdx.x, lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const BtLayout lay = bt_layout(V);
    const int npad = (int)lay.npad;
    unsigned char* row = ws + (size_t)b * lay.row_bytes;
    float* t = (float*)row;
    uint8_t* flags = row + lay.flags_off;
    const GenRow r = gen_row(seq_all, smax, cur_dev);
    const bf16* logits = logits_all + (size_t)b * ldl;
    gen_flags_row(V, r.seq, r.len, penalty, ngram, flags);
    if (ids) {
        for (int i = threadIdx.x; i < A; i += blockDim.x) {
            const int id = ids[i];
            if (id >= 0 && id < V) flags[id] |= 4;   // unique ids: one thread per byte
        }
        __syncthreads();
    }

    const BtLse rl = bt_row_lse(logits, flags, V, red, wsum);
    const bool dead = rl.dead;   // every entry is (-inf, 0)
    const float lse = rl.lse;

    // ---- acc into the workspace, and the histogram of the keys' top byte
    const float rs = run_score[b];
    gs_hist_clear(hist);
    bt_for_each<true>(logits, flags, V, [&](int i, float s, uint32_t f) {
        float v = gen_processed(__fsub_rn(s, lse), f, penalty);
        if (ids && !(f & 4)) v = -INFINITY;
        v = __fadd_rn(v, rs);
        if (dead || !(v == v)) v = -INFINITY;   // NaN never wins
        if (v == 0.f) v = 0.f;                  // -0 and +0 tie: one key
        t[i] = v;
        gs_hist_add(hist, gs_key(v) >> 24, 1ull);
    });
    for (int i = V + threadIdx.x; i < npad; i += blockDim.x) {   // the padding: -inf
        t[i] = -INFINITY;
        gs_hist_add(hist, gs_key(-INFINITY) >> 24, 1ull);
    }
    if (threadIdx.x == 0) cnt = 0;
    u64 kept = 0;
    // its first barrier publishes t, hist and cnt; npad >= 256 > M entries, so the M-th largest exists
    const uint32_t thr = gs_radix_select<false>(t, (const u64*)nullptr, npad, (u64)M, hist, tot, sel, kept);
    const int above = (int)sel[2];   // entries with a key above thr (< M): sel outlives the select until it is rewritten
    const bool inf_fill = thr == gs_key(-INFINITY);

    // ---- the entries above the cut, in any order (the rank sort below orders them)
    gs_for_each4(t, npad, [&](int i4, const f32x4& tv) {
#pragma unroll
        for (int e = 0; e < 4; ++e)
            if (gs_key(tv[e]) > thr) {
                const int s = atomicAdd(&cnt, 1);
                if (s < BM_M_MAX) {
                    top_s[s] = tv[e];
                    top_t[s] = i4 * 4 + e;
                }
            }
    });
    // ---- the entries at the cut, lowest tokens first, until M are held
    if (inf_fill) {
        for (int s = above + threadIdx.x; s < M; s += blockDim.x) {
            top_s[s] = -INFINITY;
            top_t[s] = 0;
        }
    } else {
        int filled = above;   // workgroup-uniform
        for (int c0 = 0; c0 < V && filled < M; c0 += blockDim.x) {
            const int i = c0 + threadIdx.x;
            const bool tie = i < V && gs_key(t[i]) == thr;
            const unsigned long long m = __ballot(tie);
            if (lane == 0) wcnt[wv] = __popcll(m);
            __syncthreads();
            int off = filled, all = 0;
#pragma unroll
            for (int w = 0; w < 16; ++w) {
                if (w < wv) off += wcnt[w];
                all += wcnt[w];
            }
            const int s = off + __popcll(m & ((1ull << lane) - 1ull));
            if (tie && s < M) {
                top_s[s] = t[i];
                top_t[s] = i;
            }
            filled += all;
            __syncthreads();
        }
    }
    __syncthreads();
    if ((int)threadIdx.x < M) {
        const int i = threadIdx.x;
        const float si = top_s[i];
        const int ti = top_t[i];
        int rank = 0;
        for (int j = 0; j < M; ++j) {
            const float sj = top_s[j];
            const int tj = top_t[j];
            rank += (sj > si || (sj == si && (tj < ti || (tj == ti && j < i)))) ? 1 : 0;
        }
        cand_score[(size_t)b * M + rank] = si;
        cand_tok[(size_t)b * M + rank] = ti;
    }
}

// Row r = blockIdx.x (include/kdstep.h, kd_score_rows): the log-probability of column t = target[r]
// under the row's softmax, k_gen_beam_topk's lse (bt_row_lse) without its M-best search.  With s' the
// score as fp32 and a NaN read as -inf: rank = the entries that the greedy select takes before t
// (s' larger, or equal at a lower column), top1 = the lowest column at the maximum.  Both are integer
// reductions (a count, a minimum), so nothing depends on the order the waves ran in.  They share the
// third pass over the row, which is skipped where neither is asked for.  lds = 0: every row reads the
// same N scores.
__global__ void __launch_bounds__(1024) k_score_rows(const bf16* __restrict__ scores_all, int64_t lds, int N,
                                                     const int* __restrict__ target, float* __restrict__ logprob,
                                                     int* __restrict__ rank, int* __restrict__ top1,
                                                     float* __restrict__ top1_logprob) {
    __shared__ u64 wsum[16];
    __shared__ float red[16];
    __shared__ int wcnt[16];
    __shared__ int wmin[16];
    const int r = blockIdx.x, lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const bf16* scores = scores_all + (size_t)r * lds;
    const int t = target[r];
    const bool inside = t >= 0 && t < N;
    const BtLse rl = bt_row_lse(scores, (const uint8_t*)nullptr, N, red, wsum);
    float st = inside ? (float)scores[t] : -INFINITY;
    if (!(st == st)) st = -INFINITY;
    if (threadIdx.x == 0) {
        logprob[r] = (rl.dead || !(st > -INFINITY)) ? -INFINITY : __fsub_rn(st, rl.lse);
        if (top1_logprob) top1_logprob[r] = rl.dead ? -INFINITY : __fsub_rn(rl.mx, rl.lse);
    }
    if (!rank && !top1) return;

    int cnt = 0, first = N;
    const float mx = rl.mx;
    bt_for_each<false>(scores, (const uint8_t*)nullptr, N, [&](int i, float s, uint32_t) {
        if (!(s == s)) s = -INFINITY;
        cnt += (s > st || (s == st && i < t)) ? 1 : 0;
        if (s == mx) first = min(first, i);
    });
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        cnt += __shfl_xor(cnt, o, 64);
        first = min(first, __shfl_xor(first, o, 64));
    }
    if (lane == 0) {
        wcnt[wv] = cnt;
        wmin[wv] = first;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        cnt = 0;
        first = N;
#pragma unroll
        for (int w = 0; w < 16; ++w) {
            cnt += wcnt[w];
            first = min(first, wmin[w]);
        }
        if (rank) rank[r] = inside ? cnt : N;
        if (top1) top1[r] = rl.dead ? 0 : first;
    }
}

// Prompt p = blockIdx.x, rows p * K .. p * K + K - 1: everything of a beam-search step behind the
// per-row lists (include/kdstep.h, kd_gen_beam_step).  Every selection is a rank sort in LDS over at
// most K * M <= 576 keys with a total order (score, then position), so the result does not depend on
// the thread schedule.  Only the generated window [L, L + max_new) of a sequence row moves: the
// prompt below it is the same in every beam.  The windows are staged in LDS (int32) before any row
// is rewritten, since beams and finished slots are permuted in place.  live[0] = prompts still open,
// written by the workgroup that arrives last at the counter live[1] (an integer ticket; the open
// flags cross workgroups through device-scope atomics).
__global__ void __launch_bounds__(256) k_gen_beam_step(const float* __restrict__ cand_score,
                                                       const int* __restrict__ cand_tok, int M, int K, int P,
                                                       int64_t* __restrict__ seq, int smax, int* __restrict__ cur_dev,
                                                       float* __restrict__ run_score, int64_t* __restrict__ out,
                                                       int* __restrict__ parent, int64_t* __restrict__ fin_seq,
                                                       float* __restrict__ fin_score, int* __restrict__ fin_len,
                                                       int* __restrict__ open, int* __restrict__ live,
                                                       const float* __restrict__ den, int max_new, GenEos eos,
                                                       const int* __restrict__ prompt_len) {
    extern __shared__ int bs_stage[];   // [K, max_new] running windows, then [K, max_new] finished windows
    __shared__ float cs[KD_GEN_BEAMS_MAX * BM_M_MAX];
    __shared__ int ct[KD_GEN_BEAMS_MAX * BM_M_MAX];
    __shared__ float ms[BM_M_MAX], mr[BM_M_MAX], fs[KD_GEN_BEAMS_MAX + BM_M_MAX];
    __shared__ int mj[BM_M_MAX], mt[BM_M_MAX], mhit[BM_M_MAX], flen[KD_GEN_BEAMS_MAX + BM_M_MAX];
    __shared__ int new_c[KD_GEN_BEAMS_MAX], new_f[KD_GEN_BEAMS_MAX];
    const int p = blockIdx.x, b0 = p * K, tid = threadIdx.x, nt = blockDim.x;
    int* st_run = bs_stage;
    int* st_fin = bs_stage + K * max_new;
    const int L = prompt_len[p], cur = cur_dev[b0], n_old = cur - L;
    bool run = __hip_atomic_load(&open[p], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0;
    if (run && (L < 0 || n_old < 0 || n_old >= max_new || (int64_t)L + max_new > smax)) {   // no room: close it
        run = false;
        if (tid == 0) __hip_atomic_store(&open[p], 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    if (run) {   // workgroup-uniform
        const int n = K * M;
        for (int i = tid; i < n; i += nt) {
            const float s = cand_score[(size_t)b0 * M + i];
            cs[i] = s == s ? s : -INFINITY;
            ct[i] = cand_tok[(size_t)b0 * M + i];
        }
        for (int k = tid; k < K; k += nt) {
            fs[k] = fin_score[b0 + k];
            flen[k] = fin_len[b0 + k];
        }
        for (int i = tid; i < K * n_old; i += nt) {
            const int j = i / n_old, x = i - j * n_old;
            st_run[j * max_new + x] = (int)seq[(size_t)(b0 + j) * smax + L + x];
        }
        for (int i = tid; i < K * max_new; i += nt) {
            const int k = i / max_new, x = i - k * max_new;
            st_fin[i] = (int)fin_seq[(size_t)(b0 + k) * smax + L + x];
        }
        __syncthreads();
        // ---- cand: the M largest of the K lists; ties: lower beam, then lower token = lower index
        const bool last = cur + 1 >= L + max_new;
        const float dn = den[n_old + 1];
        for (int i = tid; i < n; i += nt) {
            const float si = cs[i];
            int rank = 0;
            for (int j = 0; j < n; ++j) rank += (cs[j] > si || (cs[j] == si && j < i)) ? 1 : 0;
            if (rank < M) {
                const int tk = ct[i];
                bool hit = last;
#pragma unroll
                for (int e = 0; e < KD_GEN_EOS_MAX; ++e) hit |= e < eos.n && (int64_t)tk == eos.id[e];
                ms[rank] = si;
                mj[rank] = i / M;
                mt[rank] = tk;
                mhit[rank] = hit;
                mr[rank] = hit ? __fadd_rn(si, BM_KILL) : si;
                const bool just = hit && rank < K;
                // unsat holds on entry (a prompt whose heuristic turned false is closed): + 0
                fs[K + rank] = __fadd_rn(__fadd_rn(__fdiv_rn(si, dn), 0.f), just ? 0.f : BM_KILL);
                flen[K + rank] = just ? cur + 1 : 0;
            }
        }
        __syncthreads();
        // ---- running: the K largest r (ties: lower c); finished: the K largest of fin ++ cands
        for (int c = tid; c < M; c += nt) {
            int rank = 0;
            for (int j = 0; j < M; ++j) rank += (mr[j] > mr[c] || (mr[j] == mr[c] && j < c)) ? 1 : 0;
            if (rank < K) new_c[rank] = c;
        }
        for (int i = tid; i < K + M; i += nt) {
            int rank = 0;
            for (int j = 0; j < K + M; ++j) rank += (fs[j] > fs[i] || (fs[j] == fs[i] && j < i)) ? 1 : 0;
            if (rank < K) new_f[rank] = i;
        }
        __syncthreads();
        // ---- the rows, from the staged windows
        for (int i = tid; i < K * (n_old + 1); i += nt) {
            const int k = i / (n_old + 1), x = i - k * (n_old + 1), c = new_c[k];
            seq[(size_t)(b0 + k) * smax + L + x] = x < n_old ? (int64_t)st_run[mj[c] * max_new + x] : (int64_t)mt[c];
        }
        for (int i = tid; i < K * max_new; i += nt) {
            const int k = i / max_new, x = i - k * max_new, src = new_f[k];
            if (src == k) continue;   // the slot keeps its hypothesis
            int v;
            if (src < K) v = st_fin[src * max_new + x];
            else v = x < n_old ? st_run[mj[src - K] * max_new + x] : mt[src - K];   // past n_old: never read
            fin_seq[(size_t)(b0 + k) * smax + L + x] = v;
        }
        if (tid < K) {
            const int c = new_c[tid], src = new_f[tid];
            out[b0 + tid] = mt[c];
            parent[b0 + tid] = mj[c];
            run_score[b0 + tid] = mr[c];
            cur_dev[b0 + tid] = cur + 1;
            fin_score[b0 + tid] = fs[src];
            fin_len[b0 + tid] = flen[src];
        }
        if (tid == 0) {
            bool all_hit = true;
            for (int c = 0; c < M; ++c) all_hit &= mhit[c] != 0;
            const float best = __fdiv_rn(mr[new_c[0]], dn);   // den[cur + 1 - L] with the new cur
            float worst = INFINITY;
            for (int k = 0; k < K; ++k) worst = fminf(worst, fs[new_f[k]]);
            bool unsat = false;
            for (int k = 0; k < K; ++k) unsat |= best > (flen[new_f[k]] > 0 ? worst : BM_KILL);
            __hip_atomic_store(&open[p], unsat && !all_hit ? 1 : 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    } else if (tid < K) {
        parent[b0 + tid] = tid;   // a closed prompt: its rows stay where they are
    }
    __syncthreads();
    if (tid == 0) {
        __threadfence();
        if (atomicAdd(&live[1], 1) == P - 1) {   // the last workgroup to arrive counts
            __threadfence();
            int n_open = 0;
            for (int q = 0; q < P; ++q)
                n_open += __hip_atomic_load(&open[q], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0 ? 1 : 0;
            live[0] = n_open;
            live[1] = 0;
        }
    }
}

// Position L_p + blockIdx.x of prompt p = blockIdx.z, (layer, K or V, kv head) = blockIdx.y: beam row j
// receives the hd-vector of row parent[j].  Thread (j, 16-byte piece) reads before the barrier and
// writes behind it, so the in-place permutation never reads a vector already replaced.  Positions
// outside [L_p, cur - 1), an identity permutation and rows with parent[j] == j move nothing.
__global__ void __launch_bounds__(128) k_kv_beam_reorder(bf16* __restrict__ kc, bf16* __restrict__ vc, int layers,
                                                         int nb, int HKV, int smax, int hd, int K,
                                                         const int* __restrict__ parent,
                                                         const int* __restrict__ cur_dev,
                                                         const int* __restrict__ prompt_len) {
    const int p = blockIdx.z, b0 = p * K, L = prompt_len[p];
    const int pos = L + (int)blockIdx.x;
    if (L < 0 || pos >= min(cur_dev[b0] - 1, smax)) return;   // workgroup-uniform
    const int y = blockIdx.y, h = y % HKV, kv = (y / HKV) & 1, layer = y / (2 * HKV);
    const int pieces = hd >> 3, j = threadIdx.x / pieces, x = threadIdx.x - j * pieces;
    int src = j;
    if (j < K) {
        src = parent[b0 + j];
        if (src < 0 || src >= K) src = j;
    }
    const bool move = j < K && src != j;
    bf16* base = (kv ? vc : kc) + (((size_t)layer * nb + b0) * HKV + h) * (size_t)smax * hd + (size_t)pos * hd + x * 8;
    const size_t row = (size_t)HKV * smax * hd;
    bf16x8 v = {};
    if (move) v = *(const bf16x8*)(base + src * row);
    __syncthreads();
    if (move) *(bf16x8*)(base + j * row) = v;
}

}  // namespace

// Launch plan of k_gemv_batch: a function of (N, K) alone.  Never of nb.
struct GemvBatchPlan {
    int wg_n, wave_n, ksplit, slice_steps;
};
static GemvBatchPlan gemv_batch_plan(int N, int K) {
    const int tiles = (N + 15) / 16, ksteps = (K + 31) / 32;
    GemvBatchPlan p;
    p.wave_n = tiles >= 2048 ? 1 : 0;
    p.wg_n = p.wave_n ? (tiles + 3) / 4 : tiles;
    // K slices: about one workgroup per CU (256) while every wave keeps >= 2 steps; LDS bounds the slice
    int want = p.wave_n ? 1 : std::max(1, std::min((256 + p.wg_n - 1) / p.wg_n, ksteps / 8));
    want = std::max(want, (ksteps + GB_MAX_STEPS - 1) / GB_MAX_STEPS);
    p.slice_steps = (ksteps + want - 1) / want;
    p.ksplit = (ksteps + p.slice_steps - 1) / p.slice_steps;
    return p;
}

// f(std::integral_constant<int, E>) for the epilogue / head dim given at run time (both validated
// by the caller): one place that turns the value into a template instance.
template <typename F>
static void dispatch_epi(int epi, F&& f) {
    switch (epi) {
        case 0: f(std::integral_constant<int, 0>{}); break;
        case 1: f(std::integral_constant<int, 1>{}); break;
        case 2: f(std::integral_constant<int, 2>{}); break;
        default: f(std::integral_constant<int, 3>{});
    }
}
template <typename F>
static void dispatch_hd(int hd, F&& f) {
    if (hd == 64) f(std::integral_constant<int, 64>{});
    else f(std::integral_constant<int, 128>{});
}

// The argument checks of kd_gemv (rows_msg == nullptr: one row, read by scalar loads, no ldx) and
// of kd_gemv_batch / kd_gemv_rows (1 <= rows <= rows_max, else rows_msg), in the order the ABI
// tests pin; `who` names the entry in every message.
static int check_gemv_args(const char* who, const void* x, int64_t ldx, int rows, int rows_max, const char* rows_msg,
                           const void* W, int64_t ldw, const void* extra, const void* y, int N, int K, int epi, int I,
                           const void* norm_w) {
    auto msg = [who](const char* what) { return std::string(who) + ": " + what; };
    KD_CHECK_ARG(x && W && y, msg("null pointer"));
    KD_CHECK_ARG(epi >= 0 && epi <= 3 && (epi == 0 || epi == 3 || extra), msg("epilogue 0..3 (1, 2 need extra)"));
    const bool k_ok = N > 0 && K > 0 && K % 8 == 0 && K <= 16384 && ldw >= K && ldw % 8 == 0;
    if (!rows_msg) {
        KD_CHECK_SHAPE(k_ok, msg("K must be a multiple of 8 (<= 16384), ldw >= K and a multiple of 8"));
        KD_CHECK_ALIGN(W, 16, msg("W misaligned"));
        return KD_OK;
    }
    KD_CHECK_SHAPE(rows >= 1 && rows <= rows_max, msg(rows_msg));
    KD_CHECK_SHAPE(k_ok && ldx >= K && ldx % 8 == 0,
                   msg("K must be a multiple of 8 (<= 16384), ldw and ldx >= K and multiples of 8"));
    KD_CHECK_SHAPE(epi != 3 || I >= N, msg("SwiGLU needs inter >= N"));
    KD_CHECK_ALIGN(W, 16, msg("W misaligned"));
    KD_CHECK_ALIGN(x, 16, msg("x misaligned"));
    KD_CHECK_ALIGN(norm_w, 16, msg("norm_w misaligned"));
    return KD_OK;
}

// The argument checks of the three attention entries, in the order the ABI tests pin: ptrs_ok (every
// pointer the entry needs), rows_ok (its row-count rule, rows_msg), the head geometry, smax (with
// n_ok and its message for the entry that takes a host length), the alignment of the operands read
// 16 B at a time (vc and v_new only where the entry passes them) and the workspace.
static int check_attn_args(const char* who, bool ptrs_ok, bool rows_ok, const char* rows_msg, int H, int HKV, int hd,
                           int hdp, int smax, bool n_ok, const char* smax_msg, const void* q, const void* kc,
                           const void* vc, const void* k_new, const void* v_new, size_t ws_bytes, size_t ws_need) {
    auto msg = [who](const char* what) { return std::string(who) + ": " + what; };
    KD_CHECK_ARG(ptrs_ok, msg("null pointer"));
    KD_CHECK_SHAPE(rows_ok, msg(rows_msg));
    KD_CHECK_SHAPE(hd == 64 || hd == 128, msg("head dim must be 64 or 128"));
    KD_CHECK_SHAPE(hdp >= hd && hdp % 8 == 0, msg("hdp must be >= hd and a multiple of 8"));
    KD_CHECK_SHAPE(H > 0 && HKV > 0 && H % HKV == 0, msg("heads must be a multiple of kv heads"));
    KD_CHECK_SHAPE(smax > 0 && smax <= MAX_CH * CH && n_ok, msg(smax_msg));
    KD_CHECK_ALIGN(q, 16, msg("q misaligned"));
    KD_CHECK_ALIGN(kc, 16, msg("k cache misaligned"));
    KD_CHECK_ALIGN(vc, 16, msg("v cache misaligned"));
    KD_CHECK_ALIGN(k_new, 16, msg("k_new misaligned"));
    KD_CHECK_ALIGN(v_new, 16, msg("v_new misaligned"));
    if (ws_bytes < ws_need) return fail(KD_ERR_WORKSPACE, msg("workspace too small"));
    return KD_OK;
}

size_t gemv_batch_ws(int N, int K, int epi) {
    if (N <= 0 || K <= 0) return 0;
    const GemvBatchPlan p = gemv_batch_plan(N, K);
    return p.ksplit == 1 ? 0 : (size_t)p.ksplit * (epi == 3 ? 2 : 1) * GB_ROWS * N * sizeof(float);
}

int launch_gemv_batch(const void* x, int64_t ldx, int nb, const void* W, int64_t ldw, const void* extra, void* y, int N,
                      int K, int epi, int I, const void* norm_w, float eps, void* ws, size_t ws_bytes, void* stream) {
    if (int rc = check_gemv_args("gemv_batch", x, ldx, nb, GB_ROWS, "1 <= nb <= 16", W, ldw, extra, y, N, K, epi, I,
                                 norm_w))
        return rc;
    const GemvBatchPlan p = gemv_batch_plan(N, K);
    if (p.ksplit > 1 && (!ws || ws_bytes < gemv_batch_ws(N, K, epi)))
        return fail(KD_ERR_WORKSPACE, "gemv_batch: workspace too small (kd_gemv_batch_workspace_size)");
    const dim3 grid(p.wg_n, p.ksplit), rgrid((N + NT - 1) / NT, GB_ROWS);   // fixed by (N, K): rows >= nb exit
    const size_t lds = (size_t)GB_ROWS * (p.slice_steps * 32 + GB_PAD) * sizeof(bf16);
    hipStream_t s = as_stream(stream);
    const bf16 *xb = (const bf16*)x, *Wb = (const bf16*)W, *eb = (const bf16*)extra, *nw = (const bf16*)norm_w;
    dispatch_epi(epi, [&](auto e) {
        constexpr int E = decltype(e)::value;
        hipLaunchKernelGGL(k_gemv_batch<E>, grid, dim3(NT), lds, s, xb, ldx, Wb, ldw, eb, (bf16*)y, (float*)ws, nb, N, K,
                           I, nw, eps, p.wave_n, p.slice_steps, p.ksplit);
        if (p.ksplit > 1)
            hipLaunchKernelGGL(k_gemv_batch_reduce<E>, rgrid, dim3(NT), 0, s, (const float*)ws, eb, (bf16*)y, nb,
                               GB_ROWS, N, p.ksplit);
    });
    KD_LAUNCH_CHECK("k_gemv_batch");
    return KD_OK;
}

size_t attn_decode_ws(int H, int hd, int smax) {
    return (size_t)H * ((smax + CH - 1) / CH) * (hd + 2) * sizeof(float);
}

size_t attn_decode_batch_ws(int nb, int H, int hd, int smax) {
    return (size_t)std::max(nb, 0) * attn_decode_ws(H, hd, smax);
}

int launch_attn_decode_batch(const void* q, const void* k_new, const void* v_new, void* kc, void* vc, void* o, int nb,
                             int H, int HKV, int hd, int hdp, int smax, const int* cur_dev, void* ws, size_t ws_bytes,
                             void* stream) {
    if (int rc = check_attn_args("attn_decode_batch", q && k_new && v_new && kc && vc && o && cur_dev && ws,
                                 nb >= 1 && nb <= GB_ROWS, "1 <= nb <= 16", H, HKV, hd, hdp, smax, true,
                                 "need 0 < smax <= 32768", q, kc, nullptr, k_new, nullptr, ws_bytes,
                                 attn_decode_batch_ws(nb, H, hd, smax)))
        return rc;
    const int nch = (smax + CH - 1) / CH, ngrp = (H / HKV + AB_R - 1) / AB_R;   // head groups per kv head
    const float scale = 1.0f / sqrtf((float)hd);
    hipStream_t s = as_stream(stream);
    float* part = (float*)ws;
    dispatch_hd(hd, [&](auto d) {
        constexpr int HD = decltype(d)::value;
        hipLaunchKernelGGL(k_attn_decode_part_batch<HD>, dim3(HKV * ngrp, nch, nb), dim3(NT), 0, s, (const bf16*)q,
                           (const bf16*)k_new, (const bf16*)v_new, (bf16*)kc, (bf16*)vc, part, H, HKV, hdp, smax, nb,
                           cur_dev, scale);
        hipLaunchKernelGGL(k_attn_decode_combine<HD>, dim3(nb * H), dim3(NT), 0, s, part, nch, (bf16*)o);
    });
    KD_LAUNCH_CHECK("k_attn_decode_batch");
    return KD_OK;
}

size_t gemv_rows_ws(int rows, int N, int K, int epi) {
    if (rows < 1 || N <= 0 || K <= 0) return 0;
    const GemvBatchPlan p = gemv_batch_plan(N, K);
    if (p.ksplit == 1) return 0;
    const int rows16 = p.wave_n ? GB_ROWS : (rows + GB_ROWS - 1) / GB_ROWS * GB_ROWS;   // wave_n = 1: one slab at a time
    return (size_t)p.ksplit * (epi == 3 ? 2 : 1) * rows16 * N * sizeof(float);
}

int launch_gemv_rows(const void* x, int64_t ldx, int rows, const void* W, int64_t ldw, const void* extra, void* y, int N,
                     int K, int epi, int I, const void* norm_w, float eps, void* ws, size_t ws_bytes, void* stream) {
    if (int rc = check_gemv_args("gemv_rows", x, ldx, rows, KD_GEMV_ROWS_MAX, "1 <= rows <= KD_GEMV_ROWS_MAX", W, ldw,
                                 extra, y, N, K, epi, I, norm_w))
        return rc;
    const GemvBatchPlan p = gemv_batch_plan(N, K);
    if (p.ksplit > 1 && (!ws || ws_bytes < gemv_rows_ws(rows, N, K, epi)))
        return fail(KD_ERR_WORKSPACE, "gemv_rows: workspace too small (kd_gemv_rows_workspace_size)");
    const bf16 *xb = (const bf16*)x, *Wb = (const bf16*)W, *eb = (const bf16*)extra, *nw = (const bf16*)norm_w;
    if (p.wave_n) {
        // one tile per wave (the lm_head): a wave's share of the weights does not fit its registers,
        // so these plans make one kd_gemv_batch pass per slab (generation gives them <= 16 rows)
        for (int row0 = 0; row0 < rows; row0 += GB_ROWS) {
            const int rc = launch_gemv_batch(xb + (size_t)row0 * ldx, ldx, std::min(GB_ROWS, rows - row0), W, ldw,
                                             epi == 2 ? (const void*)(eb + (size_t)row0 * N) : extra,
                                             (bf16*)y + (size_t)row0 * N, N, K, epi, I, norm_w, eps, ws, ws_bytes, stream);
            if (rc != KD_OK) return rc;
        }
        return KD_OK;
    }
    const int rows16 = (rows + GB_ROWS - 1) / GB_ROWS * GB_ROWS;
    const dim3 grid(p.wg_n, p.ksplit, std::min(rows16 / GB_ROWS, GS_SLAB_GROUPS)), rgrid((N + NT - 1) / NT, rows);
    const size_t lds = (size_t)GB_ROWS * (p.slice_steps * 32 + GB_PAD) * sizeof(bf16);
    hipStream_t s = as_stream(stream);
    dispatch_epi(epi, [&](auto e) {
        constexpr int E = decltype(e)::value;
        hipLaunchKernelGGL(k_gemv_slabs<E>, grid, dim3(NT), lds, s, xb, ldx, Wb, ldw, eb, (bf16*)y, (float*)ws, rows, N, K,
                           I, nw, eps, p.slice_steps, p.ksplit);
        if (p.ksplit > 1)
            hipLaunchKernelGGL(k_gemv_batch_reduce<E>, rgrid, dim3(NT), 0, s, (const float*)ws, eb, (bf16*)y, rows,
                               rows16, N, p.ksplit);
    });
    KD_LAUNCH_CHECK("k_gemv_slabs");
    return KD_OK;
}

size_t attn_extend_ws(int rows, int H, int hd, int smax) {
    return (size_t)std::max(rows, 0) * attn_decode_ws(H, hd, smax);
}

int launch_attn_extend(const void* q, const void* k_new, const void* v_new, void* kc, void* vc, void* o, int nb,
                       int rows, int H, int HKV, int hd, int hdp, int smax, const int* row_start, const int* base,
                       void* ws, size_t ws_bytes, void* stream) {
    if (int rc = check_attn_args("attn_extend", q && k_new && v_new && kc && vc && o && row_start && base && ws,
                                 rows >= 1 && rows <= KD_GEMV_ROWS_MAX && nb >= 1 && nb <= rows,
                                 "1 <= nb <= rows <= KD_GEMV_ROWS_MAX", H, HKV, hd, hdp, smax, true,
                                 "need 0 < smax <= 32768", q, kc, vc, k_new, v_new, ws_bytes,
                                 attn_extend_ws(rows, H, hd, smax)))
        return rc;
    const int nch = (smax + CH - 1) / CH;
    const float scale = 1.0f / sqrtf((float)hd);
    hipStream_t s = as_stream(stream);
    float* part = (float*)ws;
    dispatch_hd(hd, [&](auto d) {
        constexpr int HD = decltype(d)::value;
        hipLaunchKernelGGL(k_attn_extend_part<HD>, dim3(HKV, nch, nb), dim3(NT), 0, s, (const bf16*)q,
                           (const bf16*)k_new, (const bf16*)v_new, (bf16*)kc, (bf16*)vc, part, H, HKV, hdp, smax, rows,
                           row_start, base, scale);
        hipLaunchKernelGGL(k_attn_decode_combine<HD>, dim3(rows * H), dim3(NT), 0, s, part, nch, (bf16*)o);
    });
    KD_LAUNCH_CHECK("k_attn_extend");
    return KD_OK;
}

// The checks the three batched choosers share: their pointers, a row of 1 <= N <= n_max scores (rule:
// the entry's words for it) at stride ld in a sequence row of smax, 1 <= nb <= 16 rows, the processors.
static int check_chooser_args(const char* who, bool pointers, int N, int n_max, const char* rule, int64_t ld, int smax,
                              int nb, float penalty, int ngram) {
    auto msg = [who](const std::string& what) { return std::string(who) + ": " + what; };
    KD_CHECK_ARG(pointers, msg("null pointer"));
    KD_CHECK_ARG(penalty > 0.f && ngram >= 0, msg("penalty must be > 0 and ngram >= 0"));
    KD_CHECK_SHAPE(N >= 1 && N <= n_max && smax > 0 && ld >= N && nb >= 1 && nb <= GB_ROWS,
                   msg(std::string(rule) + ", smax positive, ld >= its width, 1 <= nb <= 16"));
    return KD_OK;
}

int launch_gen_select_batch(const void* logits, int64_t ldl, int V, int64_t* seq, int smax, int nb, int* cur_dev,
                            float penalty, int ngram, void* flags_ws, size_t ws_bytes, int64_t* out, void* stream) {
    if (int rc = check_chooser_args("gen_select_batch", logits && seq && cur_dev && flags_ws, V, INT_MAX, "V positive",
                                    ldl, smax, nb, penalty, ngram))
        return rc;
    if (ws_bytes < (size_t)nb * V) return fail(KD_ERR_WORKSPACE, "gen_select_batch: workspace must hold nb * V bytes");
    hipLaunchKernelGGL(k_gen_select_batch, dim3(nb), dim3(1024), 0, as_stream(stream), (const bf16*)logits, ldl, V, seq,
                       smax, cur_dev, penalty, ngram, (uint8_t*)flags_ws, out);
    KD_LAUNCH_CHECK("k_gen_select_batch");
    return KD_OK;
}

int launch_rope_rows(const float* cos_t, const float* sin_t, int hh, int rows, int nb, const int* cur_dev,
                     float* cos_rows, float* sin_rows, void* stream) {
    KD_CHECK_ARG(cos_t && sin_t && cur_dev && cos_rows && sin_rows, "rope_rows: null pointer");
    KD_CHECK_SHAPE(hh > 0 && rows > 0 && nb >= 1 && nb <= KD_GEMV_ROWS_MAX,
                   "rope_rows: hh, rows positive, 1 <= nb <= KD_GEMV_ROWS_MAX");
    hipLaunchKernelGGL(k_rope_rows, dim3(nb), dim3(256), 0, as_stream(stream), cos_t, sin_t, hh, rows, cur_dev, cos_rows,
                       sin_rows);
    KD_LAUNCH_CHECK("k_rope_rows");
    return KD_OK;
}

int launch_gen_finish(const int64_t* tok, const int* cur_dev, int nb, const int64_t* eos_ids_host, int n_eos, int* fin,
                      int* live, void* stream) {
    KD_CHECK_ARG(tok && cur_dev && eos_ids_host && fin && live, "gen_finish: null pointer");
    KD_CHECK_SHAPE(nb >= 1 && nb <= 64, "gen_finish: 1 <= nb <= 64");
    KD_CHECK_SHAPE(n_eos >= 1 && n_eos <= KD_GEN_EOS_MAX, "gen_finish: 1 <= n_eos <= KD_GEN_EOS_MAX");
    GenEos eos;
    for (int e = 0; e < KD_GEN_EOS_MAX; ++e) eos.id[e] = e < n_eos ? eos_ids_host[e] : 0;
    eos.n = n_eos;
    hipLaunchKernelGGL(k_gen_finish, dim3(1), dim3(64), 0, as_stream(stream), tok, cur_dev, nb, eos, fin, live);
    KD_LAUNCH_CHECK("k_gen_finish");
    return KD_OK;
}

// One row of k_rope_rows; the table's length is not passed in, so only the lower clamp (a counter
// of 0 reads row 0) is in force.
int launch_rope_row(const float* cos_t, const float* sin_t, int hh, const int* cur_dev, float* cos_row, float* sin_row,
                    void* stream) {
    KD_CHECK_ARG(cos_t && sin_t && cur_dev && cos_row && sin_row, "rope_row: null pointer");
    KD_CHECK_SHAPE(hh > 0, "rope_row: hh must be positive");
    hipLaunchKernelGGL(k_rope_rows, dim3(1), dim3(256), 0, as_stream(stream), cos_t, sin_t, hh, INT_MAX, cur_dev, cos_row,
                       sin_row);
    KD_LAUNCH_CHECK("k_rope_rows");
    return KD_OK;
}

int launch_attn_decode(const void* q, const void* k_new, const void* v_new, void* kc, void* vc, void* o, int H,
                       int HKV, int hd, int hdp, int smax, int n, const int* cur_dev, void* ws, size_t ws_bytes,
                       void* stream) {
    if (int rc = check_attn_args("attn_decode", q && k_new && v_new && kc && vc && o && ws, true, "", H, HKV, hd, hdp,
                                 smax, cur_dev || (n > 0 && n <= smax), "need 0 < n <= smax <= 32768", q, kc, nullptr,
                                 k_new, nullptr, ws_bytes, attn_decode_ws(H, hd, smax)))
        return rc;
    const int nch = (smax + CH - 1) / CH;
    const float scale = 1.0f / sqrtf((float)hd);
    hipStream_t s = as_stream(stream);
    float* part = (float*)ws;
    dispatch_hd(hd, [&](auto d) {
        constexpr int HD = decltype(d)::value;
        hipLaunchKernelGGL(k_attn_decode_part<HD>, dim3(H, nch), dim3(NT), 0, s, (const bf16*)q, (const bf16*)k_new,
                           (const bf16*)v_new, (bf16*)kc, (bf16*)vc, part, H, HKV, hdp, smax, n, cur_dev, scale);
        hipLaunchKernelGGL(k_attn_decode_combine<HD>, dim3(H), dim3(NT), 0, s, part, nch, (bf16*)o);
    });
    KD_LAUNCH_CHECK("k_attn_decode");
    return KD_OK;
}

int launch_gemv(const void* x, const void* W, int64_t ldw, const void* extra, void* y, int N, int K, int epi, int I,
                const void* norm_w, float eps, void* stream) {
    if (int rc = check_gemv_args("gemv", x, 0, 1, 1, nullptr, W, ldw, extra, y, N, K, epi, I, norm_w)) return rc;
    const size_t lds = (size_t)K * sizeof(float);
    hipStream_t s = as_stream(stream);
    const bf16 *xb = (const bf16*)x, *Wb = (const bf16*)W, *eb = (const bf16*)extra, *nw = (const bf16*)norm_w;
    const bool wide = N < 4096 && K >= 512;   // few rows: one workgroup per row, K split over 256 threads
    dispatch_epi(epi, [&](auto e) {
        constexpr int E = decltype(e)::value;
        if (wide)
            hipLaunchKernelGGL(k_gemv_wide<E>, dim3(N), dim3(NT), lds, s, xb, Wb, ldw, eb, (bf16*)y, K, I, nw, eps);
        else
            hipLaunchKernelGGL(k_gemv<E>, dim3((N + NT / 64 - 1) / (NT / 64)), dim3(NT), lds, s, xb, Wb, ldw, eb,
                               (bf16*)y, N, K, I, nw, eps);
    });
    KD_LAUNCH_CHECK(wide ? "k_gemv_wide" : "k_gemv");
    return KD_OK;
}

int launch_gen_select(const void* logits, int V, int64_t* seq, int len, int* cur_dev, float penalty, int ngram,
                      void* flags_ws, size_t ws_bytes, int64_t* out, void* stream) {
    KD_CHECK_ARG(logits && seq && flags_ws, "gen_select: null pointer");
    KD_CHECK_SHAPE(V > 0 && (cur_dev || len > 0), "gen_select: V and len must be positive");
    KD_CHECK_ARG(penalty > 0.f && ngram >= 0, "gen_select: penalty must be > 0 and ngram >= 0");
    if (ws_bytes < (size_t)V) return fail(KD_ERR_WORKSPACE, "gen_select: workspace must hold V bytes");
    hipLaunchKernelGGL(k_gen_select, dim3(1), dim3(1024), 0, as_stream(stream), (const bf16*)logits, V, seq, len,
                       cur_dev, penalty, ngram, (uint8_t*)flags_ws, out);
    KD_LAUNCH_CHECK("k_gen_select");
    return KD_OK;
}

// Where a gathered logit has the full head's bits: the full-vocabulary routes whose per-row order
// does not depend on N.  kd_gemv: the wave-per-row k_gemv, not k_gemv_wide; kd_gemv_batch: one
// whole-K chain per tile (wave_n = 1, ksplit = 1).  The second implies the first (>= 2048 tiles),
// and both gathered entries take the one set.
bool gemv_gather_ok(int N_full, int K) {
    if (N_full <= 0 || K <= 0 || K % 8 != 0 || K > 16384) return false;
    const GemvBatchPlan p = gemv_batch_plan(N_full, K);
    const bool wide = N_full < 4096 && K >= 512;
    return !wide && p.wave_n == 1 && p.ksplit == 1;
}

// The checks the two gathered GEMVs share (x rows: check_gemv_args' rule for the entry).
static int check_gather_args(const char* who, const void* ids, int A, int N_full, int K) {
    auto msg = [who](const char* what) { return std::string(who) + ": " + what; };
    KD_CHECK_ARG(ids, msg("null pointer"));
    KD_CHECK_SHAPE(A >= 1 && A <= N_full, msg("1 <= A <= N_full"));
    KD_CHECK_SHAPE(gemv_gather_ok(N_full, K), msg("(N_full, K) outside kd_gemv_gather_supported"));
    return KD_OK;
}

int launch_gemv_gather(const void* x, const void* W, int64_t ldw, const int* ids, int A, void* y, int N_full, int K,
                       void* stream) {
    if (int rc = check_gemv_args("gemv_gather", x, 0, 1, 1, nullptr, W, ldw, nullptr, y, N_full, K, 0, 0, nullptr))
        return rc;
    if (int rc = check_gather_args("gemv_gather", ids, A, N_full, K)) return rc;
    hipLaunchKernelGGL(k_gemv_gather, dim3((A + NT / 64 - 1) / (NT / 64)), dim3(NT), (size_t)K * sizeof(float),
                       as_stream(stream), (const bf16*)x, (const bf16*)W, ldw, ids, A, (bf16*)y, N_full, K);
    KD_LAUNCH_CHECK("k_gemv_gather");
    return KD_OK;
}

int launch_gemv_batch_gather(const void* x, int64_t ldx, int nb, const void* W, int64_t ldw, const int* ids, int A,
                             void* y, int N_full, int K, void* stream) {
    if (int rc = check_gemv_args("gemv_batch_gather", x, ldx, nb, GB_ROWS, "1 <= nb <= 16", W, ldw, nullptr, y, N_full, K,
                                 0, 0, nullptr))
        return rc;
    if (int rc = check_gather_args("gemv_batch_gather", ids, A, N_full, K)) return rc;
    const int tiles = (A + 15) / 16, ksteps = (K + 31) / 32;   // ksteps <= GB_MAX_STEPS: ksplit = 1
    const size_t lds = (size_t)GB_ROWS * (ksteps * 32 + GB_PAD) * sizeof(bf16);
    hipLaunchKernelGGL(k_gemv_batch_gather, dim3((tiles + NT / 64 - 1) / (NT / 64)), dim3(NT), lds, as_stream(stream),
                       (const bf16*)x, ldx, (const bf16*)W, ldw, ids, A, (bf16*)y, nb, N_full, K);
    KD_LAUNCH_CHECK("k_gemv_batch_gather");
    return KD_OK;
}

int launch_gen_select_ids(const void* scores, int64_t lds, const int* ids, int A, int64_t* seq, int smax, int nb,
                          int* cur_dev, float penalty, int ngram, int64_t* out, void* stream) {
    if (int rc = check_chooser_args("gen_select_ids", scores && ids && seq && cur_dev, A, KD_GEN_ALLOWED_MAX,
                                    "1 <= A <= KD_GEN_ALLOWED_MAX", lds, smax, nb, penalty, ngram))
        return rc;
    hipLaunchKernelGGL(k_gen_select_ids, dim3(nb), dim3(1024), 0, as_stream(stream), (const bf16*)scores, lds, ids, A, seq,
                       smax, cur_dev, penalty, ngram, out);
    KD_LAUNCH_CHECK("k_gen_select_ids");
    return KD_OK;
}

constexpr int GS_N_MAX = 1 << 18;   // 2^18 weights of at most 2^40 each: every sum below 2^58

size_t gen_sample_ws(int nb, int N) {
    if (nb < 1 || N < 1 || N > GS_N_MAX) return 0;
    return (size_t)nb * gs_layout(N).row_bytes;
}

int launch_gen_sample(const void* scores, int64_t lds, int N, const int* ids, int64_t* seq, int smax, int nb,
                      int* cur_dev, float penalty, int ngram, float temperature, int top_k, float top_p, uint64_t seed,
                      const int64_t* streams, void* ws, size_t ws_bytes, int64_t* out, float* u_out, void* stream) {
    if (int rc = check_chooser_args("gen_sample", scores && seq && cur_dev && streams && ws && out, N,
                                    ids ? KD_GEN_ALLOWED_MAX : GS_N_MAX, "1 <= N <= 262144 (with ids: KD_GEN_ALLOWED_MAX)",
                                    lds, smax, nb, penalty, ngram))
        return rc;
    KD_CHECK_ARG(std::isfinite(temperature) && temperature > 0.f, "gen_sample: temperature must be finite and > 0");
    KD_CHECK_ARG(top_k >= 0, "gen_sample: top_k must be >= 0");
    KD_CHECK_ARG(top_p > 0.f && top_p <= 1.0f, "gen_sample: top_p must lie in (0, 1]");
    KD_CHECK_SHAPE(ws_bytes >= gen_sample_ws(nb, N), "gen_sample: workspace smaller than kd_gen_sample_workspace_size");
    KD_CHECK_SHAPE(((uintptr_t)ws & 15) == 0, "gen_sample: workspace must be 16-byte aligned");
    if (ids)
        hipLaunchKernelGGL(k_gen_sample<true>, dim3(nb), dim3(1024), 0, as_stream(stream), (const bf16*)scores, lds, N,
                           ids, seq, smax, cur_dev, penalty, ngram, temperature, top_k, top_p, seed, streams,
                           (unsigned char*)ws, out, u_out);
    else
        hipLaunchKernelGGL(k_gen_sample<false>, dim3(nb), dim3(1024), 0, as_stream(stream), (const bf16*)scores, lds, N,
                           (const int*)nullptr, seq, smax, cur_dev, penalty, ngram, temperature, top_k, top_p, seed,
                           streams, (unsigned char*)ws, out, u_out);
    KD_LAUNCH_CHECK("k_gen_sample");
    return KD_OK;
}

size_t gen_beam_topk_ws(int nb, int V) {
    if (nb < 1 || V < 1 || V > GS_N_MAX) return 0;
    return (size_t)nb * bt_layout(V).row_bytes;
}

int launch_gen_beam_topk(const void* logits, int64_t ldl, int V, const int* ids, int A, const int64_t* seq, int smax,
                         int nb, const int* cur_dev, const float* run_score, float penalty, int ngram, int M, void* ws,
                         size_t ws_bytes, float* cand_score, int* cand_tok, void* stream) {
    if (int rc = check_chooser_args("gen_beam_topk", logits && seq && cur_dev && run_score && ws && cand_score && cand_tok,
                                    V, GS_N_MAX, "1 <= V <= 262144", ldl, smax, nb, penalty, ngram))
        return rc;
    KD_CHECK_SHAPE(M >= 1 && M <= BM_M_MAX, "gen_beam_topk: 1 <= M <= 72");
    KD_CHECK_SHAPE(!ids || (A >= 1 && A <= V), "gen_beam_topk: with ids, 1 <= A <= V");
    if (ws_bytes < gen_beam_topk_ws(nb, V))
        return fail(KD_ERR_WORKSPACE, "gen_beam_topk: workspace smaller than kd_gen_beam_topk_workspace_size");
    KD_CHECK_ALIGN(ws, 16, "gen_beam_topk: workspace must be 16-byte aligned");
    hipLaunchKernelGGL(k_gen_beam_topk, dim3(nb), dim3(1024), 0, as_stream(stream), (const bf16*)logits, ldl, V, ids, A,
                       const_cast<int64_t*>(seq), smax, cur_dev, run_score, penalty, ngram, M, (unsigned char*)ws,
                       cand_score, cand_tok);
    KD_LAUNCH_CHECK("k_gen_beam_topk");
    return KD_OK;
}

int launch_score_rows(const void* scores, int64_t lds, int N, int rows, const int* target, float* logprob, int* rank,
                      int* top1, float* top1_logprob, void* stream) {
    KD_CHECK_ARG(scores && target && logprob, "score_rows: null pointer");
    KD_CHECK_SHAPE(N >= 1 && N <= GS_N_MAX && rows >= 1 && rows <= (1 << 20) && (lds == 0 || lds >= N),
                   "score_rows: 1 <= N <= 262144, 1 <= rows <= 2^20, ld_scores >= N or 0 (one shared row)");
    hipLaunchKernelGGL(k_score_rows, dim3(rows), dim3(1024), 0, as_stream(stream), (const bf16*)scores, lds, N, target,
                       logprob, rank, top1, top1_logprob);
    KD_LAUNCH_CHECK("k_score_rows");
    return KD_OK;
}

int launch_gen_beam_step(const float* cand_score, const int* cand_tok, int M, int K, int P, int64_t* seq, int smax,
                         int* cur_dev, float* run_score, int64_t* out, int* parent, int64_t* fin_seq, float* fin_score,
                         int* fin_len, int* open, int* live, const float* den, int max_new, const int64_t* eos_ids_host,
                         int n_eos, const int* prompt_len, void* stream) {
    KD_CHECK_ARG(cand_score && cand_tok && seq && cur_dev && run_score && out && parent && fin_seq && fin_score &&
                     fin_len && open && live && den && prompt_len && (eos_ids_host || n_eos == 0),
                 "gen_beam_step: null pointer");
    KD_CHECK_SHAPE(K >= 1 && K <= KD_GEN_BEAMS_MAX && M >= K && M <= BM_M_MAX,
                   "gen_beam_step: 1 <= K <= KD_GEN_BEAMS_MAX, K <= M <= 72");
    KD_CHECK_SHAPE(P >= 1 && P * K <= 64, "gen_beam_step: P >= 1 and P * K <= 64 rows");
    KD_CHECK_SHAPE(n_eos >= 0 && n_eos <= KD_GEN_EOS_MAX, "gen_beam_step: 0 <= n_eos <= KD_GEN_EOS_MAX");
    const size_t lds = (size_t)2 * K * (max_new > 0 ? max_new : 0) * sizeof(int);
    KD_CHECK_SHAPE(smax > 0 && max_new >= 1 && max_new <= smax && lds <= 32768,
                   "gen_beam_step: 1 <= max_new <= smax and K * max_new <= 4096 (the windows are staged in LDS)");
    GenEos eos;
    for (int e = 0; e < KD_GEN_EOS_MAX; ++e) eos.id[e] = e < n_eos ? eos_ids_host[e] : 0;
    eos.n = n_eos;
    hipLaunchKernelGGL(k_gen_beam_step, dim3(P), dim3(256), lds, as_stream(stream), cand_score, cand_tok, M, K, P, seq,
                       smax, cur_dev, run_score, out, parent, fin_seq, fin_score, fin_len, open, live, den, max_new, eos,
                       prompt_len);
    KD_LAUNCH_CHECK("k_gen_beam_step");
    return KD_OK;
}

int launch_kv_beam_reorder(void* kc, void* vc, int layers, int P, int K, int HKV, int smax, int hd, const int* parent,
                           const int* cur_dev, const int* prompt_len, int tail_max, void* stream) {
    KD_CHECK_ARG(kc && vc && parent && cur_dev && prompt_len, "kv_beam_reorder: null pointer");
    KD_CHECK_SHAPE(hd == 64 || hd == 128, "kv_beam_reorder: head dim 64 or 128");
    KD_CHECK_SHAPE(K >= 1 && K <= KD_GEN_BEAMS_MAX && P >= 1 && P * K <= 64,
                   "kv_beam_reorder: 1 <= K <= KD_GEN_BEAMS_MAX, P >= 1, P * K <= 64 rows");
    KD_CHECK_SHAPE(layers >= 1 && HKV >= 1 && (int64_t)layers * 2 * HKV <= 65535 && smax > 0 && tail_max >= 1 &&
                       tail_max <= smax,
                   "kv_beam_reorder: layers, HKV positive (layers * 2 * HKV <= 65535), 1 <= tail_max <= smax");
    hipLaunchKernelGGL(k_kv_beam_reorder, dim3(tail_max, layers * 2 * HKV, P), dim3(128), 0, as_stream(stream), (bf16*)kc,
                       (bf16*)vc, layers, P * K, HKV, smax, hd, K, parent, cur_dev, prompt_len);
    KD_LAUNCH_CHECK("k_kv_beam_reorder");
    return KD_OK;
}

}  // namespace kd
