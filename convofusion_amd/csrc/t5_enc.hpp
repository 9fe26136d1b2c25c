// The T5 v1.0 text encoder (transformers T5EncoderModel, feed_forward_proj "relu") and the reference's projection (t5.py:48-49, 57) in exact
// float32: token ids to the text memories in 5 launches per block + 1 (cfd_t5_encode, cfd_text.hip).
//
//   per block   t5_gemm  q | k | v = rs(x) (x g1) Wqkv^T        A gain g1 at the tile fill, row scale rs(x) = rsqrt(mean(x^2) + eps) in the epilogue;
//                                                               block 0 reads its rows straight from the embedding table (x = embed[ids])
//               t5_attn  ctx = softmax(q k^T + rel_bias[h][j - i + T - 1], keys of mask 0 left out) v      (no 1 / sqrt(d_kv))
//               t5_gemm  h = x + ctx Wo^T                       residual epilogue (block 0: the residual is gathered too)
//               t5_gemm  f = relu(rs(h) (h g2) Wi^T)            gain, row scale, ReLU
//               t5_gemm  x' = h + f Wo_ff^T                     residual epilogue
//   at the end  t5_gemm  out = rs(x) relu(x g_f) Wp^T + b       (relu(rs x g) = rs relu(x g): rs > 0), or t5_final_rows: out = rs(x) x g_f
//
// Arithmetic: v_mfma_f32_32x32x2_f32 -- float32 operands, float32 accumulation, each product an exact fmaf chain; no operand has a
// range limit (feed-forward intermediates of public T5 checkpoints leave fp16's range, so gemm_sp.hpp's split pairs are not used here).
// No atomics.  An output element's k order is fixed by the 32-deep k tile (tile step s multiplies k = s and k = 16 + s of the tile) and the
// 256-deep accumulation chunk alone, never by the number of rows or the block shape, and attention walks a query's unmasked keys in ascending order: a sequence's result is
// the same bits whatever else is in the batch, and whatever it is padded to.
//
// Packed weights (float32, built by convofusion_amd/text.py): embed [vocab][768] | per block: g1 [768] | Wqkv [2304][768] | Wo [768][768] |
// g2 [768] | Wi [3072][768] | Wo_ff [768][3072] | g_final [768].  Matrices as nn.Linear stores them ([out][in]), unscaled.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#define T5_D 768
#define T5_DKV 64
#define T5_H 12
#define T5_FF 3072
#define T5_MAX_LAYERS 12
#define T5_MAX_T 256
#define T5_BK 32          // k tile of the products
#define T5_CHUNK_TILES 8  // k tiles per accumulation chunk (256 k)
#define T5_LDK 36         // floats per LDS tile row (32 + 4: rows stay 16-byte aligned, 4-bank skew)

typedef __attribute__((ext_vector_type(16))) float t5_f32x16;
typedef __attribute__((ext_vector_type(4))) float t5_f32x4;

__host__ __device__ inline size_t t5_block_floats() { return (size_t)2 * T5_D + (size_t)4 * T5_D * T5_D + (size_t)2 * T5_FF * T5_D; }
__host__ __device__ inline size_t t5_pack_floats(int vocab, int nl) { return (size_t)vocab * T5_D + (size_t)nl * t5_block_floats() + T5_D; }
// the workspace of a call, floats per token row: x | h | q k v | ctx | f
__host__ __device__ inline size_t t5_ws_row_floats() { return (size_t)3 * T5_D + 3 * T5_D + T5_FF; }

enum { T5_ROWSCALE = 1, T5_RELU_OUT = 2, T5_RELU_A = 4 };

struct T5GemmArgs {
  const float* A;          // [M][K] rows of lda floats; with a_ids: the table whose row a_ids[m] is row m
  const int32_t* a_ids;
  long long lda;
  const float* gain;       // [K] or null: A is multiplied by it at the tile fill (the RMS norm's weight)
  const float* W;          // [N][K]
  const float* bias;       // [N] or null
  const float* R;          // residual [M][N] rows of ldr floats (or a table gathered through r_ids), or null
  const int32_t* r_ids;
  long long ldr;
  float* Y;                // [M][N] rows of ldy floats
  long long ldy;
  int M, N, K, flags;
  int id_max;              // ids are clamped to [0, id_max] (the host refuses ids outside the vocabulary; this keeps a stray one in bounds)
  float eps;
};

__device__ __forceinline__ long long t5_row_of(const int32_t* ids, int m, int id_max) {
  if (!ids) return m;
  const int v = ids[m];
  return v < 0 ? 0 : v > id_max ? id_max : v;
}

// Y = epilogue(A' W^T): a workgroup of 4 waves (2 x 2) owns a (64 TM) x (64 TN) block, a wave TM x TN MFMA tiles of 32 x 32.  A and W tiles
// of 32 k go global -> registers (one step ahead) -> LDS; lane (i = lane % 32, half = lane / 32) reads k = 16 half .. 16 half + 15 of its
// rows as four float4 and step s of the tile feeds v_mfma_f32_32x32x2_f32 the pair (k = s, k = 16 + s).  Rows past M read row M - 1 and
// are not written.  N % (64 TN) == 0 and K % 32 == 0 (checked by the caller).
template <int TM, int TN>
__global__ void __launch_bounds__(256) t5_gemm_kernel(const T5GemmArgs a) {
  constexpr int BM = 64 * TM, BN = 64 * TN;
  constexpr int NA = BM * (T5_BK / 4) / 256, NB = BN * (T5_BK / 4) / 256;   // float4 per thread and tile
  __shared__ __attribute__((aligned(16))) float As[BM * T5_LDK];
  __shared__ __attribute__((aligned(16))) float Ws[BN * T5_LDK];
  __shared__ float rs[BM];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;
  const int m0 = blockIdx.y * BM, n0 = blockIdx.x * BN;
  const int c4 = tid & 7;                      // the thread's float4 column of a tile row

  long long arow[NA], wrow[NB];                // the thread's tile rows, as element offsets into A and W
#pragma unroll
  for (int i = 0; i < NA; ++i) {
    int m = m0 + (tid >> 3) + 32 * i;
    m = m < a.M ? m : a.M - 1;
    arow[i] = t5_row_of(a.a_ids, m, a.id_max) * a.lda + 4 * c4;
  }
#pragma unroll
  for (int i = 0; i < NB; ++i) wrow[i] = (long long)(n0 + (tid >> 3) + 32 * i) * a.K + 4 * c4;

  // acc: the MFMA chain of the current 256-deep k chunk; tot: the sum of the finished chunks (two-level summation: the rounding error of a
  // 3072-deep product grows with sqrt(256) + sqrt(12), not sqrt(3072))
  t5_f32x16 acc[TM][TN], tot[TM][TN];
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[i][j][e] = tot[i][j][e] = 0.f;

  float ss[NA];
#pragma unroll
  for (int i = 0; i < NA; ++i) ss[i] = 0.f;
  t5_f32x4 ra[NA], rw[NB];
#pragma unroll
  for (int i = 0; i < NA; ++i) ra[i] = *reinterpret_cast<const t5_f32x4*>(a.A + arow[i]);
#pragma unroll
  for (int i = 0; i < NB; ++i) rw[i] = *reinterpret_cast<const t5_f32x4*>(a.W + wrow[i]);

  const int half = lane >> 5, li = lane & 31;
  for (int k0 = 0; k0 < a.K; k0 += T5_BK) {
    // registers -> LDS: the row's sum of squares from the raw values, then the gain and the ReLU of the operand
    t5_f32x4 g = {1.f, 1.f, 1.f, 1.f};
    if (a.gain) g = *reinterpret_cast<const t5_f32x4*>(a.gain + k0 + 4 * c4);
#pragma unroll
    for (int i = 0; i < NA; ++i) {
      t5_f32x4 v = ra[i];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        ss[i] = fmaf(v[e], v[e], ss[i]);
        v[e] *= g[e];
        if (a.flags & T5_RELU_A) v[e] = fmaxf(v[e], 0.f);
      }
      *reinterpret_cast<t5_f32x4*>(&As[((tid >> 3) + 32 * i) * T5_LDK + 4 * c4]) = v;
    }
#pragma unroll
    for (int i = 0; i < NB; ++i) *reinterpret_cast<t5_f32x4*>(&Ws[((tid >> 3) + 32 * i) * T5_LDK + 4 * c4]) = rw[i];
    __syncthreads();
    if (k0 + T5_BK < a.K) {                    // the next tile's loads fly under this tile's MFMAs
#pragma unroll
      for (int i = 0; i < NA; ++i) ra[i] = *reinterpret_cast<const t5_f32x4*>(a.A + arow[i] + k0 + T5_BK);
#pragma unroll
      for (int i = 0; i < NB; ++i) rw[i] = *reinterpret_cast<const t5_f32x4*>(a.W + wrow[i] + k0 + T5_BK);
    }
    t5_f32x4 fa[TM][4], fb[TN][4];
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
      for (int q = 0; q < 4; ++q) fa[i][q] = *reinterpret_cast<const t5_f32x4*>(&As[((wm * TM + i) * 32 + li) * T5_LDK + 16 * half + 4 * q]);
#pragma unroll
    for (int j = 0; j < TN; ++j)
#pragma unroll
      for (int q = 0; q < 4; ++q) fb[j][q] = *reinterpret_cast<const t5_f32x4*>(&Ws[((wn * TN + j) * 32 + li) * T5_LDK + 16 * half + 4 * q]);
#pragma unroll
    for (int q = 0; q < 4; ++q)
#pragma unroll
      for (int e = 0; e < 4; ++e)
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
          for (int j = 0; j < TN; ++j)
            acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[i][q][e], fb[j][q][e], acc[i][j], 0, 0, 0);
    if ((k0 / T5_BK) % T5_CHUNK_TILES == T5_CHUNK_TILES - 1 || k0 + T5_BK >= a.K) {
#pragma unroll
      for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j) {
          tot[i][j] += acc[i][j];
#pragma unroll
          for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;
        }
    }
    __syncthreads();
  }

  if (a.flags & T5_ROWSCALE) {                 // the 8 threads of a tile row hold its partial sums: one fixed order
#pragma unroll
    for (int i = 0; i < NA; ++i) {
      float s = ss[i];
      s += __shfl_xor(s, 1, 64);
      s += __shfl_xor(s, 2, 64);
      s += __shfl_xor(s, 4, 64);
      if (c4 == 0) rs[(tid >> 3) + 32 * i] = rsqrtf(s / (float)a.K + a.eps);
    }
    __syncthreads();
  }

  // C / D of the 32 x 32 MFMA: column lane % 32, row (reg % 4) + 8 (reg / 4) + 4 (lane / 32)
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j) {
      const int n = n0 + (wn * TN + j) * 32 + li;
      const float bn = a.bias ? a.bias[n] : 0.f;
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const int ml = (wm * TM + i) * 32 + (e & 3) + 8 * (e >> 2) + 4 * half;
        const int m = m0 + ml;
        if (m >= a.M) continue;
        float v = tot[i][j][e];
        if (a.flags & T5_ROWSCALE) v *= rs[ml];
        v += bn;
        if (a.flags & T5_RELU_OUT) v = fmaxf(v, 0.f);
        if (a.R) v += a.R[t5_row_of(a.r_ids, m, a.id_max) * a.ldr + n];
        a.Y[(long long)m * a.ldy + n] = v;
      }
    }
}

// ctx[s][i][h] = softmax_j(q_i . k_j + rel_bias[h][j - i + T - 1]) v_j over the keys j of mask 1, for 64 queries of one (sequence, head):
// grid (ceil(T / 64), 12, n_seq), one wave; a lane owns a query (q and the running value sum in registers) and walks the keys in
// ascending order, 64 at a time through LDS (K and V tiles, 32 KB), with a running maximum.  A masked key is skipped: probability
// exactly 0, and no trace of it in the sums.  Padded queries are computed like any other.  A sequence with no key at all gives NaN rows.
__global__ void __launch_bounds__(64) t5_attn_kernel(const float* __restrict__ qkv, const uint8_t* __restrict__ mask, const float* __restrict__ rel_bias,
                                                    float* __restrict__ ctx, int T) {
  __shared__ __attribute__((aligned(16))) float Ks[64 * T5_DKV];
  __shared__ __attribute__((aligned(16))) float Vs[64 * T5_DKV];
  __shared__ uint8_t Ms[64];
  const int lane = threadIdx.x, h = blockIdx.y, s = blockIdx.z;
  const int i = blockIdx.x * 64 + lane;
  const int iq = i < T ? i : T - 1;
  const float* base = qkv + (long long)s * T * (3 * T5_D) + h * T5_DKV;
  float q[T5_DKV], o[T5_DKV];
#pragma unroll
  for (int d = 0; d < T5_DKV; d += 4) {
    const float4 v = *reinterpret_cast<const float4*>(base + (long long)iq * (3 * T5_D) + d);
    q[d] = v.x; q[d + 1] = v.y; q[d + 2] = v.z; q[d + 3] = v.w;
    o[d] = o[d + 1] = o[d + 2] = o[d + 3] = 0.f;
  }
  const float* rb = rel_bias + (long long)h * (2 * T - 1) + (T - 1) - iq;
  float mx = -INFINITY, l = 0.f;
  for (int j0 = 0; j0 < T; j0 += 64) {
    const int nj = T - j0 < 64 ? T - j0 : 64;
    __syncthreads();
    for (int e = lane; e < nj * (T5_DKV / 4); e += 64) {
      const int j = e >> 4, d = (e & 15) * 4;
      const float* row = base + (long long)(j0 + j) * (3 * T5_D) + d;
      *reinterpret_cast<float4*>(&Ks[j * T5_DKV + d]) = *reinterpret_cast<const float4*>(row + T5_D);
      *reinterpret_cast<float4*>(&Vs[j * T5_DKV + d]) = *reinterpret_cast<const float4*>(row + 2 * T5_D);
    }
    if (lane < nj) Ms[lane] = mask[(long long)s * T + j0 + lane];
    __syncthreads();
    for (int j = 0; j < nj; ++j) {
      if (!Ms[j]) continue;                    // (wave-uniform)
      float sc = 0.f;
#pragma unroll
      for (int d = 0; d < T5_DKV; d += 4) {
        const float4 kv = *reinterpret_cast<const float4*>(&Ks[j * T5_DKV + d]);
        sc = fmaf(q[d], kv.x, sc); sc = fmaf(q[d + 1], kv.y, sc); sc = fmaf(q[d + 2], kv.z, sc); sc = fmaf(q[d + 3], kv.w, sc);
      }
      sc += rb[j0 + j];
      float p;
      if (sc > mx) {                           // a new maximum: what was summed so far shrinks by exp(old - new)
        const float c = expf(mx - sc);         // (0 for the first key: mx = -inf)
        l *= c;
#pragma unroll
        for (int d = 0; d < T5_DKV; ++d) o[d] *= c;
        mx = sc;
        p = 1.f;
      } else {
        p = expf(sc - mx);
      }
      l += p;
#pragma unroll
      for (int d = 0; d < T5_DKV; d += 4) {
        const float4 vv = *reinterpret_cast<const float4*>(&Vs[j * T5_DKV + d]);
        o[d] = fmaf(p, vv.x, o[d]); o[d + 1] = fmaf(p, vv.y, o[d + 1]); o[d + 2] = fmaf(p, vv.z, o[d + 2]); o[d + 3] = fmaf(p, vv.w, o[d + 3]);
      }
    }
  }
  if (i < T) {
    const float inv = 1.f / l;
    float* out = ctx + ((long long)s * T + i) * T5_D + h * T5_DKV;
#pragma unroll
    for (int d = 0; d < T5_DKV; d += 4) *reinterpret_cast<float4*>(out + d) = make_float4(o[d] * inv, o[d + 1] * inv, o[d + 2] * inv, o[d + 3] * inv);
  }
}

// The last hidden state when no projection is asked for: out = x rsqrt(mean(x^2) + eps) g, a wave per row (4 rows per workgroup).
__global__ void __launch_bounds__(256) t5_final_rows_kernel(const float* __restrict__ x, const float* __restrict__ g, float* __restrict__ out, int M,
                                                           float eps) {
  const int lane = threadIdx.x & 63;
  const int m = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (m >= M) return;
  const float* row = x + (long long)m * T5_D;
  float v[T5_D / 64], s = 0.f;
#pragma unroll
  for (int e = 0; e < T5_D / 64; ++e) { v[e] = row[lane + 64 * e]; s = fmaf(v[e], v[e], s); }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off, 64);
  const float r = rsqrtf(s / (float)T5_D + eps);
#pragma unroll
  for (int e = 0; e < T5_D / 64; ++e) out[(long long)m * T5_D + lane + 64 * e] = v[e] * r * g[lane + 64 * e];
}
