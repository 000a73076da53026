// bert_any.hip -- the GENERAL BERT forward of librmu.so (gfx950): every post-LayerNorm, GELU(erf), absolute-position BERT whose heads are 64
// wide -- hidden = 64 * heads with 2 <= heads <= 16 (bert-tiny 128/2 ... bert-base 768/12, bert-large 1024/16), ffn a multiple of 64 up to
// 4096 -- with hidden, heads, ffn and layers as RUNTIME values.  The tuned 384/12/1536 encoder (bert.hip) is a different set of kernels and
// is not touched by anything here; bert.hip routes a model to this unit through the opaque context of bert_any.h.
//
// Numerics are the tuned path's: bf16 activations, fp32 accumulation, fp32 LayerNorm and softmax statistics.  Every buffer below is a
// rounding point (bf16): h, qkv, ctx, y, h1, mid -- and P, the softmax numerators, in front of the P V product.
//
// Token rows are PACKED: sequence b of a group at rows [cu[b] - cu[0], + len[b]), len = clip(lens, 0, max_len).  A call is walked in GROUPS
// of whole sequences, GROUP_TOKENS / max_len sequences each (so a group never holds more than GROUP_TOKENS = 16384 packed tokens): the
// workspace is bounded by the group, not by the call.  Every kernel computes a row (GEMM, LayerNorm) or a sequence (attention, heads) from
// that row or sequence alone, in one fixed order: what else is in the call, and where a group boundary falls, does not change a bit.
// One dispatch regime: the same kernels and tiles for 8 tokens and for a million.
#include <algorithm>
#include <cmath>
#include <new>
#include <vector>

#include "rmu_common.h"
#include "rmu_host.h"
#include "../../include/rmu.h"
#include "bert_any.h"

typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;
typedef __attribute__((ext_vector_type(4))) __bf16 bf16x4;
typedef __bf16 bf16;

namespace {

constexpr int GROUP_TOKENS = 16384;      // packed tokens of one group (>= 512: one sequence always fits)
constexpr int ROW_PAD = 128;             // workspace rows are a multiple of the GEMM's token tile: its M edge needs no guard
constexpr int MAX_UNITS = 2;             // a lane of a row-per-wave kernel holds 16-byte units `lane` and `lane + 64` of the row (hidden <= 1024)

__device__ __forceinline__ float bf2f(bf16 v) { return (float)v; }

// ------------------------------------------------------------------------------------------------------------
// create-time conversions
// ------------------------------------------------------------------------------------------------------------
__global__ void k_any_to_bf16(const float* __restrict__ src, bf16* __restrict__ dst, int64_t n, float scale) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) dst[i] = (bf16)(src[i] * scale);
}
__global__ void k_any_copy(const float* __restrict__ src, float* __restrict__ dst, int64_t n, float scale) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) dst[i] = src[i] * scale;
}

// cu[0] = 0, cu[b + 1] = cu[b] + clamp(lens[b], 0, max_len) over the WHOLE call; one block
__global__ __launch_bounds__(1024) void k_any_cu(const int* __restrict__ lens, int batch, int max_len, int* __restrict__ cu) {
    __shared__ int part[1024];
    const int tid = threadIdx.x, nt = blockDim.x;
    const int per = (batch + nt - 1) / nt;
    const int lo = min(batch, tid * per), hi = min(batch, lo + per);
    int s = 0;
    for (int i = lo; i < hi; ++i) s += min(max(lens[i], 0), max_len);
    part[tid] = s;
    __syncthreads();
    if (tid == 0) {
        int run = 0;
        for (int i = 0; i < nt; ++i) { const int v = part[i]; part[i] = run; run += v; }
        cu[0] = 0;
    }
    __syncthreads();
    int run = part[tid];
    for (int i = lo; i < hi; ++i) { run += min(max(lens[i], 0), max_len); cu[i + 1] = run; }
}

// ------------------------------------------------------------------------------------------------------------
// LayerNorm of one row held by one wave: lane l holds columns [8 l, +8) and [8 (l + 64), +8) where they exist; two-pass fp32 statistics
// ------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ void ln_row_any(float (&v)[MAX_UNITS][8], const bool (&act)[MAX_UNITS], int lane, int hidden, const float* __restrict__ g,
                                           const float* __restrict__ b, float eps) {
    float s = 0.f;
#pragma unroll
    for (int u = 0; u < MAX_UNITS; ++u)
#pragma unroll
        for (int i = 0; i < 8; ++i) s += act[u] ? v[u][i] : 0.f;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
    const float inv_h = 1.0f / (float)hidden;
    const float mu = s * inv_h;
    float q = 0.f;
#pragma unroll
    for (int u = 0; u < MAX_UNITS; ++u)
#pragma unroll
        for (int i = 0; i < 8; ++i) { const float d = act[u] ? v[u][i] - mu : 0.f; q = fmaf(d, d, q); }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) q += __shfl_xor(q, o);
    const float rs = rsqrtf(q * inv_h + eps);
#pragma unroll
    for (int u = 0; u < MAX_UNITS; ++u) {
        if (!act[u]) continue;
        const int c0 = (lane + 64 * u) * 8;
        const f32x4 g0 = *(const f32x4*)(g + c0), g1 = *(const f32x4*)(g + c0 + 4);
        const f32x4 b0 = *(const f32x4*)(b + c0), b1 = *(const f32x4*)(b + c0 + 4);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            v[u][i] = (v[u][i] - mu) * rs * g0[i] + b0[i];
            v[u][4 + i] = (v[u][4 + i] - mu) * rs * g1[i] + b1[i];
        }
    }
}

__device__ __forceinline__ void store_row_any(const float (&v)[MAX_UNITS][8], const bool (&act)[MAX_UNITS], int lane, bf16* __restrict__ row) {
#pragma unroll
    for (int u = 0; u < MAX_UNITS; ++u) {
        if (!act[u]) continue;
        bf16x8 o;
#pragma unroll
        for (int i = 0; i < 8; ++i) o[i] = (bf16)v[u][i];          // rounding point: the row leaves as bf16
        *(bf16x8*)(row + (lane + 64 * u) * 8) = o;
    }
}

// embeddings + LayerNorm: one wave per (sequence, position) slot of the group; packed output row cu[b] - cu[0] + pos.  type_ids == NULL: type 0.
__global__ __launch_bounds__(256) void k_any_embed_ln(const int* __restrict__ ids, const int* __restrict__ type_ids, const int* __restrict__ cu, int nseq,
                                                      int max_len, int hidden, const float* __restrict__ wemb, const float* __restrict__ pemb,
                                                      const float* __restrict__ temb, const float* __restrict__ g, const float* __restrict__ bta,
                                                      float eps, int vocab, int type_vocab, bf16* __restrict__ out) {
    const int lane = threadIdx.x & 63;
    const int64_t slot = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (slot >= (int64_t)nseq * max_len) return;
    const int b = (int)(slot / max_len), pos = (int)(slot % max_len);
    const int len = cu[b + 1] - cu[b];
    if (pos >= len) return;
    int id = ids[slot];
    id = min(max(id, 0), vocab - 1);
    int tt = type_ids ? type_ids[slot] : 0;
    tt = min(max(tt, 0), type_vocab - 1);
    float v[MAX_UNITS][8];
    bool act[MAX_UNITS];
#pragma unroll
    for (int u = 0; u < MAX_UNITS; ++u) {
        const int c0 = (lane + 64 * u) * 8;
        act[u] = c0 < hidden;
#pragma unroll
        for (int i = 0; i < 8; ++i) v[u][i] = 0.f;
        if (act[u]) {
            const float* we = wemb + (int64_t)id * hidden + c0;
            const float* pe = pemb + (int64_t)pos * hidden + c0;
            const float* te = temb + (int64_t)tt * hidden + c0;
#pragma unroll
            for (int hf = 0; hf < 2; ++hf) {
                const f32x4 a = *(const f32x4*)(we + 4 * hf), p = *(const f32x4*)(pe + 4 * hf), t = *(const f32x4*)(te + 4 * hf);
#pragma unroll
                for (int i = 0; i < 4; ++i) v[u][4 * hf + i] = a[i] + p[i] + t[i];
            }
        }
    }
    ln_row_any(v, act, lane, hidden, g, bta, eps);
    store_row_any(v, act, lane, out + ((int64_t)(cu[b] - cu[0]) + pos) * hidden);
}

// LayerNorm over the group's packed rows: one wave per row
__global__ __launch_bounds__(256) void k_any_layernorm(const bf16* __restrict__ y, const int* __restrict__ cu, int nseq, int hidden,
                                                       const float* __restrict__ g, const float* __restrict__ bta, float eps, bf16* __restrict__ out) {
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= (int64_t)(cu[nseq] - cu[0])) return;
    float v[MAX_UNITS][8];
    bool act[MAX_UNITS];
#pragma unroll
    for (int u = 0; u < MAX_UNITS; ++u) {
        const int c0 = (lane + 64 * u) * 8;
        act[u] = c0 < hidden;
        bf16x8 x = {};
        if (act[u]) x = *(const bf16x8*)(y + row * hidden + c0);
#pragma unroll
        for (int i = 0; i < 8; ++i) v[u][i] = bf2f(x[i]);
    }
    ln_row_any(v, act, lane, hidden, g, bta, eps);
    store_row_any(v, act, lane, out + row * hidden);
}

// ------------------------------------------------------------------------------------------------------------
// C[T, N] = A[T, K] W[N, K]^T + bias, bf16 in, fp32 accumulate, bf16 out.  Workgroup = 4 waves = a 128-token x 128-feature tile, wave
// (wr, wc) its 64 x 64 quarter as 4 x 4 fragments of v_mfma_f32_16x16x32_bf16 with the WEIGHTS as the A operand: D[feature][token], so a lane
// holds 4 consecutive features of one token (col = lane & 15 = token, row = 4 (lane >> 4) + reg = feature) and stores them as one 8-byte piece.
// Both operands are staged through LDS in 64-deep k tiles (rows of 64 bf16 + 8 of padding: 144-byte rows keep the 16-byte fragment reads of
// 16 consecutive rows off each other's banks); the next tile's global loads are in flight in registers while this one is multiplied.
// Weight layout: row-major [N, K] bf16 (converted once at create time) -- a B^T operand's fragment is 16 contiguous bytes of a weight row.
// Edges: N and K are multiples of 64; an N tile that hangs over (N = 192, 576, 704 ...) has its upper 64 features absent -- their weight rows
// are read from row N - 1 (in bounds) and the waves with wc = 1 neither multiply nor store.  T is arbitrary: the workspace rows are padded to
// a multiple of 128, tiles at or beyond T exit, and the last tile computes its padding rows into padding rows (a row depends on its own A
// row only, so whatever those hold reaches no real row).
// ------------------------------------------------------------------------------------------------------------
enum { EPI_BIAS = 0, EPI_GELU = 1, EPI_RESID = 2 };
constexpr int GBM = 128, GBN = 128, GBK = 64, GSTR = GBK + 8;

template <int EPI>
__global__ __launch_bounds__(256) void k_gemm_any(const bf16* __restrict__ A, const bf16* __restrict__ W, const float* __restrict__ bias,
                                                  const bf16* __restrict__ resid, bf16* __restrict__ out, const int* __restrict__ cu, int nseq, int N,
                                                  int K) {
    __shared__ __attribute__((aligned(16))) bf16 lds[2 * GBM * GSTR];
    bf16* sA = lds;
    bf16* sW = lds + GBM * GSTR;
    const int T = cu[nseq] - cu[0];
    const int m0 = blockIdx.y * GBM, n0 = blockIdx.x * GBN;
    if (m0 >= T) return;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int wr = w >> 1, wc = w & 1;
    const bool live = n0 + wc * 64 < N;                 // (wave-uniform) this wave's 64 features exist

    // staging: 128 rows x 8 units of 16 bytes per operand tile, four units per thread
    const bf16* ga[4];
    const bf16* gw[4];
    int so[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int u = tid + 256 * i, row = u >> 3, c = (u & 7) * 8;
        ga[i] = A + (int64_t)(m0 + row) * K + c;
        gw[i] = W + (int64_t)min(n0 + row, N - 1) * K + c;
        so[i] = row * GSTR + c;
    }
    bf16x8 ra[4], rw[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) { ra[i] = *(const bf16x8*)ga[i]; rw[i] = *(const bf16x8*)gw[i]; }

    f32x4 acc[4][4];
#pragma unroll
    for (int n = 0; n < 4; ++n)
#pragma unroll
        for (int m = 0; m < 4; ++m) acc[n][m] = f32x4{0.f, 0.f, 0.f, 0.f};

    const int fo = (lane & 15) * GSTR + (lane >> 4) * 8;       // a fragment: row lane & 15, k = 8 (lane >> 4) .. + 8
    for (int k0 = 0; k0 < K; k0 += GBK) {
        __syncthreads();                                       // the previous tile has been read
#pragma unroll
        for (int i = 0; i < 4; ++i) { *(bf16x8*)(sA + so[i]) = ra[i]; *(bf16x8*)(sW + so[i]) = rw[i]; }
        __syncthreads();
        if (k0 + GBK < K) {
#pragma unroll
            for (int i = 0; i < 4; ++i) { ra[i] = *(const bf16x8*)(ga[i] + k0 + GBK); rw[i] = *(const bf16x8*)(gw[i] + k0 + GBK); }
        }
        if (live) {
#pragma unroll
            for (int ks = 0; ks < 2; ++ks) {
                bf16x8 af[4], wf[4];
#pragma unroll
                for (int m = 0; m < 4; ++m) af[m] = *(const bf16x8*)(sA + (wr * 64 + m * 16) * GSTR + fo + ks * 32);
#pragma unroll
                for (int n = 0; n < 4; ++n) wf[n] = *(const bf16x8*)(sW + (wc * 64 + n * 16) * GSTR + fo + ks * 32);
#pragma unroll
                for (int n = 0; n < 4; ++n)
#pragma unroll
                    for (int m = 0; m < 4; ++m) acc[n][m] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf[n], af[m], acc[n][m], 0, 0, 0);
            }
        }
    }
    if (!live) return;
#pragma unroll
    for (int n = 0; n < 4; ++n) {
        const int col = n0 + wc * 64 + n * 16 + (lane >> 4) * 4;
        const f32x4 bv = *(const f32x4*)(bias + col);
#pragma unroll
        for (int m = 0; m < 4; ++m) {
            const int64_t row = m0 + wr * 64 + m * 16 + (lane & 15);
            f32x4 v = acc[n][m] + bv;
            if constexpr (EPI == EPI_GELU) {
#pragma unroll
                for (int r = 0; r < 4; ++r) v[r] = 0.5f * v[r] * (1.0f + erff(v[r] * 0.70710678118654752f));
            }
            if constexpr (EPI == EPI_RESID) {
                const bf16x4 rv = *(const bf16x4*)(resid + row * N + col);
#pragma unroll
                for (int r = 0; r < 4; ++r) v[r] += bf2f(rv[r]);
            }
            bf16x4 o;
#pragma unroll
            for (int r = 0; r < 4; ++r) o[r] = (bf16)v[r];         // rounding point: qkv / mid / y leave as bf16
            *(bf16x4*)(out + row * N + col) = o;
        }
    }
}

// ------------------------------------------------------------------------------------------------------------
// Attention, head width 64.  Workgroup = (sequence, head, block of 128 query rows), 4 waves of 32 query rows; keys and values of the
// sequence pass through LDS 64 at a time (K as [key][64 d], V transposed as [d][64 keys]).  Both products on v_mfma_f32_32x32x16_bf16:
//   S^T[key][q] = K Q^T  -- K the A operand, Q (in registers for the whole kernel) the B operand: a lane holds the scores of ONE query
//                 row, q = lane & 31, for keys (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5) of the 32-key tile; the other 16 in lane ^ 32.
//   O^T[d][q]  += V^T P^T -- P^T is that accumulator tile, converted to bf16 in place, as the B operand (registers 8 s .. 8 s + 7 are k-step
//                 s; element j is key 16 s + 8 (j >> 2) + 4 (lane >> 5) + (j & 3)), V^T fragments read from LDS in the same key order.
// Softmax is the online form over 32-key tiles with fp32 running maximum m and sum l per query row (one lane each: the rescale of O^T is a
// multiply of the lane's own registers); exp2 on the scores as they are, log2(e) / sqrt(64) having been folded into Wq and bq.  Keys at or
// beyond the sequence's length are masked to -inf; their K and V rows are staged as zeros.  Nothing S x S ever leaves the registers.
// ------------------------------------------------------------------------------------------------------------
constexpr int AKEYS = 64, ASTR = 64 + 8;

__global__ __launch_bounds__(256) void k_any_attn(const bf16* __restrict__ qkv, const int* __restrict__ cu, int hidden, bf16* __restrict__ ctx) {
    __shared__ __attribute__((aligned(16))) bf16 lds[2 * AKEYS * ASTR];
    bf16* sK = lds;                       // [key][d]
    bf16* sV = lds + AKEYS * ASTR;        // [d][key]
    const int b = blockIdx.z, head = blockIdx.y, q0 = blockIdx.x * 128;
    const int t0 = cu[b] - cu[0], L = cu[b + 1] - cu[b];
    if (q0 >= L) return;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int r = lane & 31, h = lane >> 5;
    const int64_t ld = 3 * (int64_t)hidden;
    const bf16* base = qkv + (int64_t)t0 * ld + head * 64;
    const int qw = q0 + w * 32;
    const bool wave_live = qw < L;        // (wave-uniform)
    const int q = qw + r;

    bf16x8 qf[4];
#pragma unroll
    for (int s = 0; s < 4; ++s) {
        qf[s] = bf16x8{};
        if (q < L) qf[s] = *(const bf16x8*)(base + (int64_t)q * ld + 16 * s + 8 * h);
    }
    f32x16 o0, o1;
#pragma unroll
    for (int i = 0; i < 16; ++i) { o0[i] = 0.f; o1[i] = 0.f; }
    float m = -INFINITY, l = 0.f;

    for (int c0 = 0; c0 < L; c0 += AKEYS) {
        __syncthreads();                  // the previous 64 keys have been read
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int u = tid + 256 * i, key = u >> 3, du = u & 7;
            bf16x8 kv = {}, vv = {};
            if (c0 + key < L) {
                const bf16* p = base + (int64_t)(c0 + key) * ld + du * 8;
                kv = *(const bf16x8*)(p + hidden);
                vv = *(const bf16x8*)(p + 2 * hidden);
            }
            *(bf16x8*)(sK + key * ASTR + du * 8) = kv;
#pragma unroll
            for (int e = 0; e < 8; ++e) sV[(du * 8 + e) * ASTR + key] = vv[e];
        }
        __syncthreads();
        if (!wave_live) continue;
#pragma unroll
        for (int kt = 0; kt < 2; ++kt) {
            const int kbase = c0 + kt * 32;
            if (kbase < L) {              // (uniform) a tile with no real key is skipped
                f32x16 sc;
#pragma unroll
                for (int i = 0; i < 16; ++i) sc[i] = 0.f;
#pragma unroll
                for (int s = 0; s < 4; ++s) {
                    const bf16x8 kf = *(const bf16x8*)(sK + (kt * 32 + r) * ASTR + 16 * s + 8 * h);
                    sc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kf, qf[s], sc, 0, 0, 0);
                }
                float tmax = -INFINITY;
#pragma unroll
                for (int i = 0; i < 16; ++i) {
                    const int key = kbase + (i & 3) + 8 * (i >> 2) + 4 * h;
                    sc[i] = key < L ? sc[i] : -INFINITY;
                    tmax = fmaxf(tmax, sc[i]);
                }
                tmax = fmaxf(tmax, __shfl_xor(tmax, 32));        // key kbase is real, so the tile's maximum is finite
                const float m_new = fmaxf(m, tmax);
                const float alpha = exp2f(m - m_new);            // (first tile: exp2(-inf) = 0 over o = 0, l = 0)
                m = m_new;
                float psum = 0.f;
#pragma unroll
                for (int i = 0; i < 16; ++i) { sc[i] = exp2f(sc[i] - m_new); psum += sc[i]; }
                l = fmaf(l, alpha, psum);
#pragma unroll
                for (int i = 0; i < 16; ++i) { o0[i] *= alpha; o1[i] *= alpha; }
#pragma unroll
                for (int s = 0; s < 2; ++s) {
                    bf16x8 pb;
#pragma unroll
                    for (int j = 0; j < 8; ++j) pb[j] = (bf16)sc[8 * s + j];      // rounding point: P enters the second product as bf16
                    const int ko = kt * 32 + 16 * s + 4 * h;
                    const bf16x4 a0 = *(const bf16x4*)(sV + r * ASTR + ko), a1 = *(const bf16x4*)(sV + r * ASTR + ko + 8);
                    const bf16x4 c0v = *(const bf16x4*)(sV + (r + 32) * ASTR + ko), c1v = *(const bf16x4*)(sV + (r + 32) * ASTR + ko + 8);
                    const bf16x8 va = {a0[0], a0[1], a0[2], a0[3], a1[0], a1[1], a1[2], a1[3]};
                    const bf16x8 vb = {c0v[0], c0v[1], c0v[2], c0v[3], c1v[0], c1v[1], c1v[2], c1v[3]};
                    o0 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(va, pb, o0, 0, 0, 0);
                    o1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(vb, pb, o1, 0, 0, 0);
                }
            }
        }
    }
    if (!wave_live) return;
    const float inv = 1.0f / (l + __shfl_xor(l, 32));
    if (q < L) {
        bf16* dst = ctx + (int64_t)(t0 + q) * hidden + head * 64;
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            bf16x4 a, c;
#pragma unroll
            for (int e = 0; e < 4; ++e) { a[e] = (bf16)(o0[4 * g + e] * inv); c[e] = (bf16)(o1[4 * g + e] * inv); }   // rounding point: ctx
            *(bf16x4*)(dst + 8 * g + 4 * h) = a;
            *(bf16x4*)(dst + 32 + 8 * g + 4 * h) = c;
        }
    }
}

// ------------------------------------------------------------------------------------------------------------
// heads, fp32 (semantics: include/rmu.h at RMU_BERT_POOL_MEAN ... RMU_BERT_NO_NORMALIZE)
// ------------------------------------------------------------------------------------------------------------
// Pooling + Normalize, one wave per sequence: masked mean (sum / max(len, 1e-9)) or the first token's state; x / max(|x|, 1e-12) unless told
// not to.  A sequence of length 0 gives the zero vector.
__global__ __launch_bounds__(64) void k_any_pool(const bf16* __restrict__ hs, const int* __restrict__ cu, int hidden, float* __restrict__ out,
                                                 int64_t out_stride, int pool_cls, int normalize) {
    const int b = blockIdx.x, lane = threadIdx.x;
    const int t0 = cu[b] - cu[0], Lr = cu[b + 1] - cu[b];
    const int L = pool_cls ? min(Lr, 1) : Lr;
    float s[MAX_UNITS][8];
    bool act[MAX_UNITS];
#pragma unroll
    for (int u = 0; u < MAX_UNITS; ++u) {
        act[u] = (lane + 64 * u) * 8 < hidden;
#pragma unroll
        for (int i = 0; i < 8; ++i) s[u][i] = 0.f;
    }
    for (int t = 0; t < L; ++t) {
#pragma unroll
        for (int u = 0; u < MAX_UNITS; ++u) {
            if (!act[u]) continue;
            const bf16x8 v = *(const bf16x8*)(hs + (int64_t)(t0 + t) * hidden + (lane + 64 * u) * 8);
#pragma unroll
            for (int i = 0; i < 8; ++i) s[u][i] += bf2f(v[i]);
        }
    }
    const float inv = pool_cls ? 1.0f : 1.0f / fmaxf((float)L, 1e-9f);
    float q = 0.f;
#pragma unroll
    for (int u = 0; u < MAX_UNITS; ++u)
#pragma unroll
        for (int i = 0; i < 8; ++i) { s[u][i] *= inv; q = fmaf(s[u][i], s[u][i], q); }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) q += __shfl_xor(q, o);
    const float rn = normalize ? 1.0f / fmaxf(sqrtf(q), 1e-12f) : 1.0f;
#pragma unroll
    for (int u = 0; u < MAX_UNITS; ++u) {
        if (!act[u]) continue;
        float* dst = out + (int64_t)b * out_stride + (lane + 64 * u) * 8;
#pragma unroll
        for (int i = 0; i < 8; ++i) dst[i] = s[u][i] * rn;
    }
}

// final hidden states of the group's real tokens as fp32 rows: local packed row i -> out row cu[0] + i (cu[0]: the packed tokens of the groups before)
__global__ __launch_bounds__(256) void k_any_tokens_out(const bf16* __restrict__ hs, const int* __restrict__ cu, int nseq, int hidden,
                                                        float* __restrict__ out, int64_t out_stride) {
    const int64_t M = cu[nseq] - cu[0];
    const int per = hidden / 8;
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;      // one thread per 8 features
    const int64_t row = i / per;
    const int c0 = (int)(i % per) * 8;
    if (row >= M) return;
    const bf16x8 v = *(const bf16x8*)(hs + row * hidden + c0);
    float* dst = out + (cu[0] + row) * out_stride + c0;
#pragma unroll
    for (int e = 0; e < 8; ++e) dst[e] = bf2f(v[e]);
}

// BertForSequenceClassification(num_labels = 1): logit = wc . tanh(Wp h_cls + bp) + bc; one workgroup of 4 waves per sequence, a wave per
// pooler row at a time (lanes along the row, shuffle reduction).  A sequence of length 0: the head over a zero hidden state.
__global__ __launch_bounds__(256) void k_any_cls_head(const bf16* __restrict__ hs, const int* __restrict__ cu, int hidden, const float* __restrict__ wp,
                                                      const float* __restrict__ bp, const float* __restrict__ wc, const float* __restrict__ bc,
                                                      float* __restrict__ out) {
    __shared__ float red[4];
    const int b = blockIdx.x, lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int t0 = cu[b] - cu[0], L = cu[b + 1] - cu[b];
    const int nj = hidden / 64;                        // 2 .. 16 columns per lane
    float hc[16];
#pragma unroll
    for (int j = 0; j < 16; ++j) hc[j] = (j < nj && L > 0) ? bf2f(hs[(int64_t)t0 * hidden + lane + 64 * j]) : 0.f;
    float part = 0.f;
    for (int o = w; o < hidden; o += 4) {
        const float* row = wp + (int64_t)o * hidden;
        float a = 0.f;
#pragma unroll
        for (int j = 0; j < 16; ++j)
            if (j < nj) a = fmaf(row[lane + 64 * j], hc[j], a);
#pragma unroll
        for (int sft = 32; sft > 0; sft >>= 1) a += __shfl_xor(a, sft);
        part = fmaf(wc[o], tanhf(a + bp[o]), part);
    }
    if (lane == 0) red[w] = part;
    __syncthreads();
    if (threadIdx.x == 0) out[b] = ((red[0] + red[1]) + (red[2] + red[3])) + bc[0];
}

}  // namespace

// ------------------------------------------------------------------------------------------------------------
// context
// ------------------------------------------------------------------------------------------------------------
struct AnyLayer {
    bf16 *wqkv, *wo, *w1, *w2;
    float *bqkv, *bo, *b1, *b2, *ln1g, *ln1b, *ln2g, *ln2b;
};
struct rmu_any_bert {
    rmu_bert_cfg cfg;
    float *wemb = nullptr, *pemb = nullptr, *temb = nullptr, *elng = nullptr, *elnb = nullptr;
    std::vector<AnyLayer> layers;
    float *wp = nullptr, *bp = nullptr, *wc = nullptr, *bc = nullptr;
    std::vector<void*> owned;             // the weights
    // workspace of ONE group (guarded by the model's mutex: one forward at a time)
    RmuDevBuf h, h1, y, qkv, ctx, mid, cu;
};

template <class T>
static int any_dev_alloc(rmu_any_bert* a, T** p, size_t count) {
    void* q = nullptr;
    if (hipMalloc(&q, count * sizeof(T)) != hipSuccess) return RMU_E_OOM;
    a->owned.push_back(q);
    *p = (T*)q;
    return RMU_OK;
}
static int any_f32(rmu_any_bert* a, float** dst, const void* src, size_t n, float scale, hipStream_t s) {
    if (any_dev_alloc(a, dst, n)) return RMU_E_OOM;
    hipLaunchKernelGGL(k_any_copy, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, (const float*)src, *dst, (int64_t)n, scale);
    return RMU_OK;
}
static void any_bf16(bf16* dst, const void* src, size_t n, float scale, hipStream_t s) {
    hipLaunchKernelGGL(k_any_to_bf16, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, (const float*)src, dst, (int64_t)n, scale);
}

bool rmu_any_geometry_(const rmu_bert_cfg* cfg) {
    if (cfg->hidden == 384 && cfg->heads == 12 && cfg->ffn == 1536) return false;       // the tuned kernels', always
    return cfg->heads >= 2 && cfg->heads <= 16 && cfg->hidden == 64 * cfg->heads && cfg->ffn >= 64 && cfg->ffn <= 4096 && cfg->ffn % 64 == 0;
}

void rmu_any_free_(rmu_any_bert* a) {
    if (!a) return;
    for (void* p : a->owned) (void)hipFree(p);
    delete a;                             // (the workspace buffers release themselves)
}

int rmu_any_create_(rmu_any_bert** out, const rmu_bert_cfg* cfg, const void* const* wptr, hipStream_t s) {
    auto* a = new (std::nothrow) rmu_any_bert();
    if (!a) return RMU_E_OOM;
    a->cfg = *cfg;
    const size_t H = (size_t)cfg->hidden, FF = (size_t)cfg->ffn;
    int rc = RMU_OK, wi = 0;
    rc |= any_f32(a, &a->wemb, wptr[wi++], (size_t)cfg->vocab_size * H, 1.f, s);
    rc |= any_f32(a, &a->pemb, wptr[wi++], (size_t)cfg->max_pos * H, 1.f, s);
    rc |= any_f32(a, &a->temb, wptr[wi++], (size_t)cfg->type_vocab * H, 1.f, s);
    rc |= any_f32(a, &a->elng, wptr[wi++], H, 1.f, s);
    rc |= any_f32(a, &a->elnb, wptr[wi++], H, 1.f, s);
    // softmax scale and log2(e) folded into the query projection (as the tuned path does): the attention kernel uses exp2 on the raw MFMA output
    const float qs = 1.4426950408889634f / sqrtf(64.0f);
    a->layers.resize(cfg->layers);
    for (int l = 0; l < cfg->layers && !rc; ++l) {
        AnyLayer& L = a->layers[l];
        const void *qw = wptr[wi++], *qb = wptr[wi++], *kw = wptr[wi++], *kb = wptr[wi++], *vw = wptr[wi++], *vb = wptr[wi++];
        rc |= any_dev_alloc(a, &L.wqkv, 3 * H * H);
        rc |= any_dev_alloc(a, &L.bqkv, 3 * H);
        if (rc) break;
        any_bf16(L.wqkv, qw, H * H, qs, s);
        any_bf16(L.wqkv + H * H, kw, H * H, 1.f, s);
        any_bf16(L.wqkv + 2 * H * H, vw, H * H, 1.f, s);
        const dim3 gb((unsigned)((H + 255) / 256));
        hipLaunchKernelGGL(k_any_copy, gb, dim3(256), 0, s, (const float*)qb, L.bqkv, (int64_t)H, qs);
        hipLaunchKernelGGL(k_any_copy, gb, dim3(256), 0, s, (const float*)kb, L.bqkv + H, (int64_t)H, 1.f);
        hipLaunchKernelGGL(k_any_copy, gb, dim3(256), 0, s, (const float*)vb, L.bqkv + 2 * H, (int64_t)H, 1.f);
        rc |= any_dev_alloc(a, &L.wo, H * H);
        if (!rc) any_bf16(L.wo, wptr[wi], H * H, 1.f, s);
        wi++;
        rc |= any_f32(a, &L.bo, wptr[wi++], H, 1.f, s);
        rc |= any_f32(a, &L.ln1g, wptr[wi++], H, 1.f, s);
        rc |= any_f32(a, &L.ln1b, wptr[wi++], H, 1.f, s);
        rc |= any_dev_alloc(a, &L.w1, FF * H);
        if (!rc) any_bf16(L.w1, wptr[wi], FF * H, 1.f, s);
        wi++;
        rc |= any_f32(a, &L.b1, wptr[wi++], FF, 1.f, s);
        rc |= any_dev_alloc(a, &L.w2, H * FF);
        if (!rc) any_bf16(L.w2, wptr[wi], H * FF, 1.f, s);
        wi++;
        rc |= any_f32(a, &L.b2, wptr[wi++], H, 1.f, s);
        rc |= any_f32(a, &L.ln2g, wptr[wi++], H, 1.f, s);
        rc |= any_f32(a, &L.ln2b, wptr[wi++], H, 1.f, s);
    }
    if (!rc && cfg->has_head) {
        rc |= any_f32(a, &a->wp, wptr[wi++], H * H, 1.f, s);
        rc |= any_f32(a, &a->bp, wptr[wi++], H, 1.f, s);
        rc |= any_f32(a, &a->wc, wptr[wi++], H, 1.f, s);
        rc |= any_f32(a, &a->bc, wptr[wi++], 1, 1.f, s);
    }
    if (rc) {
        (void)hipStreamSynchronize(s);    // (conversions already enqueued read and write what is about to be freed)
        rmu_any_free_(a);
        return rc;
    }
    *out = a;
    return RMU_OK;
}

// rows of the group workspace for a call of this shape: the largest group's padded capacity, up to the GEMM's token tile
static int64_t any_ws_rows(int batch, int max_len) {
    const int64_t spg = std::max(1, GROUP_TOKENS / max_len);
    const int64_t cap = std::min<int64_t>(batch, spg) * max_len;
    return (cap + ROW_PAD - 1) / ROW_PAD * ROW_PAD;
}
namespace {
struct WsNeed { RmuDevBuf rmu_any_bert::*buf; size_t bytes; };
}
static void any_ws_needs(const rmu_any_bert* a, int batch, int max_len, WsNeed (&need)[7]) {
    const size_t rows = (size_t)any_ws_rows(batch, max_len), H = (size_t)a->cfg.hidden, FF = (size_t)a->cfg.ffn;
    need[0] = {&rmu_any_bert::h, rows * H * 2};
    need[1] = {&rmu_any_bert::h1, rows * H * 2};
    need[2] = {&rmu_any_bert::y, rows * H * 2};
    need[3] = {&rmu_any_bert::qkv, rows * 3 * H * 2};
    need[4] = {&rmu_any_bert::ctx, rows * H * 2};
    need[5] = {&rmu_any_bert::mid, rows * FF * 2};
    need[6] = {&rmu_any_bert::cu, ((size_t)batch + 1) * sizeof(int)};
}
bool rmu_any_ws_grows_(const rmu_any_bert* a, int batch, int max_len) {
    WsNeed need[7];
    any_ws_needs(a, batch, max_len, need);
    for (const WsNeed& n : need)
        if ((a->*n.buf).p && n.bytes > (a->*n.buf).cap) return true;
    return false;
}
int rmu_any_ensure_ws_(rmu_any_bert* a, int batch, int max_len) {
    WsNeed need[7];
    any_ws_needs(a, batch, max_len, need);
    for (const WsNeed& n : need)
        if ((a->*n.buf).ensure(n.bytes) != hipSuccess) { (void)hipGetLastError(); return RMU_E_OOM; }
    return RMU_OK;
}

template <int EPI>
static void any_gemm(const bf16* A, const bf16* W, const float* bias, const bf16* resid, bf16* out, const int* cu, int nseq, int64_t cap, int N, int K,
                     hipStream_t s) {
    const dim3 grid((unsigned)((N + GBN - 1) / GBN), (unsigned)((cap + GBM - 1) / GBM));
    hipLaunchKernelGGL((k_gemm_any<EPI>), grid, dim3(256), 0, s, A, W, bias, resid, out, cu, nseq, N, K);
}

void rmu_any_enqueue_forward_(rmu_any_bert* a, const int32_t* ids, const int32_t* type_ids, const int32_t* lens, int batch, int max_len, int mode,
                              float* out_dev, int64_t out_stride, hipStream_t s) {
    const int kind = mode & 0xff;
    const bool normalize = !(mode & RMU_BERT_NO_NORMALIZE);
    const int H = a->cfg.hidden, FF = a->cfg.ffn, NH = a->cfg.heads;
    const float eps = a->cfg.ln_eps;
    bf16 *h = (bf16*)a->h.p, *h1 = (bf16*)a->h1.p, *y = (bf16*)a->y.p, *qkv = (bf16*)a->qkv.p, *ctx = (bf16*)a->ctx.p, *mid = (bf16*)a->mid.p;
    int* cu_all = (int*)a->cu.p;
    hipLaunchKernelGGL(k_any_cu, dim3(1), dim3(batch <= 64 ? 64 : batch <= 256 ? 256 : 1024), 0, s, (const int*)lens, batch, max_len, cu_all);
    const int spg = std::max(1, GROUP_TOKENS / max_len);
    for (int g0 = 0; g0 < batch; g0 += spg) {
        const int nb = std::min(spg, batch - g0);
        const int64_t cap = (int64_t)nb * max_len;                 // <= GROUP_TOKENS slots, at most that many packed rows
        const int* cu = cu_all + g0;
        const int32_t* gids = ids + (int64_t)g0 * max_len;
        const int32_t* gtt = type_ids ? type_ids + (int64_t)g0 * max_len : nullptr;
        const dim3 rows4((unsigned)((cap + 3) / 4));
        hipLaunchKernelGGL(k_any_embed_ln, rows4, dim3(256), 0, s, (const int*)gids, (const int*)gtt, cu, nb, max_len, H, a->wemb, a->pemb, a->temb,
                           a->elng, a->elnb, eps, a->cfg.vocab_size, a->cfg.type_vocab, h);
        for (const AnyLayer& L : a->layers) {
            any_gemm<EPI_BIAS>(h, L.wqkv, L.bqkv, nullptr, qkv, cu, nb, cap, 3 * H, H, s);
            hipLaunchKernelGGL(k_any_attn, dim3((unsigned)((max_len + 127) / 128), (unsigned)NH, (unsigned)nb), dim3(256), 0, s, (const bf16*)qkv, cu, H, ctx);
            any_gemm<EPI_RESID>(ctx, L.wo, L.bo, h, y, cu, nb, cap, H, H, s);
            hipLaunchKernelGGL(k_any_layernorm, rows4, dim3(256), 0, s, (const bf16*)y, cu, nb, H, L.ln1g, L.ln1b, eps, h1);
            any_gemm<EPI_GELU>(h1, L.w1, L.b1, nullptr, mid, cu, nb, cap, FF, H, s);
            any_gemm<EPI_RESID>(mid, L.w2, L.b2, h1, y, cu, nb, cap, H, FF, s);
            hipLaunchKernelGGL(k_any_layernorm, rows4, dim3(256), 0, s, (const bf16*)y, cu, nb, H, L.ln2g, L.ln2b, eps, h);
        }
        if (kind == RMU_BERT_POOL_MEAN || kind == RMU_BERT_POOL_CLS)
            hipLaunchKernelGGL(k_any_pool, dim3((unsigned)nb), dim3(64), 0, s, (const bf16*)h, cu, H, out_dev + (int64_t)g0 * out_stride, out_stride,
                               kind == RMU_BERT_POOL_CLS ? 1 : 0, normalize ? 1 : 0);
        else if (kind == RMU_BERT_TOKENS)
            hipLaunchKernelGGL(k_any_tokens_out, dim3((unsigned)((cap * (H / 8) + 255) / 256)), dim3(256), 0, s, (const bf16*)h, cu, nb, H, out_dev, out_stride);
        else
            hipLaunchKernelGGL(k_any_cls_head, dim3((unsigned)nb), dim3(256), 0, s, (const bf16*)h, cu, H, a->wp, a->bp, a->wc, a->bc, out_dev + g0);
    }
}
