// ConvoFusionVae.encode in one launch: both SkipTransformerEncoders (body, hands) for every 16-frame chunk, from the raw motion
// features to the 2 global-motion tokens per chunk and stack (reference vae.py:162-266, SkipTransformerEncoder cross_attention.py:18-64,
// TransformerEncoderLayer.forward_pre :288-300; configs/modules/motion_vae.yaml: d_model 128, 2 heads, ff 1024, pre-norm, gelu).
//
// One workgroup (256 threads, 4 waves) = one stack x G chunk sequences of 18 tokens (2 global tokens + 16 frames), R = 16 * RT rows (RT
// a template parameter, 2 - 4), G = R / 18.  Row order inside the workgroup: the 2G global tokens first (row 2i + t = token t of sequence i), then the 16G frames
// (row 2G + 16i + f), then padding rows (zero input, never read as keys, never written out).  The global tokens thus fill the first
// 16-row tile, and the last layer -- whose result is kept for those rows only -- runs its queries, attention, out-projection, FFN and the
// final LayerNorm on that tile alone; its keys and values still cover every row.
//
// Activations stay in LDS: x, the (num_layers - 1) / 2 skip tensors of the input blocks, one work region (the per-head Q | K | V, the
// 128-column FFN hidden chunk, or the staged input features) and the per-row LayerNorm statistics.  Every product is exact float32:
// v_mfma_f32_16x16x4_f32 with the A fragment from LDS (the LayerNorm applied while it is read) and the B fragment streamed from the
// packed weights in global memory (one float4 per lane per 16-deep k-step, prefetched one step ahead).  The FFN hidden (1024) is produced
// and consumed in 128-column chunks that accumulate into registers.  Softmax and the value sum are per-row VALU work (4 lanes per row,
// 16 head dimensions each).
//
// Packed weights (float32; one block per stack, the hands block right after the body block; ve_stack_floats(num_layers) each), matrices
// W [N][K] (nn.Linear layout) in the MFMA-B order: float4 index ((n/16 * K/16 + k/16) * 64 + lane), lane = 16 * ((k % 16) / 4) + n % 16,
// element k % 4 -- built by convofusion_amd/vae.py (_pack_w):
//   skel_embedding.weight [128][128] (K zero-padded from 69 / 120), skel_embedding.bias [128], global_motion_token [2][128],
//   query_pos_encoder.pe[0:18] [18][128],
//   per layer (input_blocks..., middle_block, output_blocks...): norm1 w, b; self_attn.in_proj_weight [384][128]; in_proj_bias [384];
//     out_proj.weight [128][128]; out_proj.bias; norm2 w, b; linear1.weight [1024][128]; linear1.bias [1024]; linear2.weight [128][1024];
//     linear2.bias [128],
//   per linear block: weight [128][256], bias [128],
//   norm w, b.
#pragma once
#include <hip/hip_runtime.h>

#include "cfd_common.hpp"

#define VE_D 128
#define VE_FF 1024
#define VE_HD 64             // head dim (2 heads)
#define VE_T 18              // tokens per sequence: 2 global + 16 frames
#define VE_LDX (VE_D + 4)    // LDS row stride of x / skips / FFN hidden / staged input (floats)
#define VE_LDH (VE_HD + 4)   // LDS row stride of the per-head Q, K, V
#define VE_BODY 69
#define VE_HANDS 120
#define VE_NFEATS 189
#define VE_MAX_LAYERS 9

// float offsets inside one stack's block
#define VE_EMB_W 0
#define VE_EMB_B (VE_EMB_W + VE_D * VE_D)
#define VE_TOK (VE_EMB_B + VE_D)
#define VE_PE (VE_TOK + 2 * VE_D)
#define VE_LAYER0 (VE_PE + VE_T * VE_D)
// inside a layer
#define VL_LN1G 0
#define VL_LN1B (VL_LN1G + VE_D)
#define VL_WQKV (VL_LN1B + VE_D)
#define VL_BQKV (VL_WQKV + 3 * VE_D * VE_D)
#define VL_WO (VL_BQKV + 3 * VE_D)
#define VL_BO (VL_WO + VE_D * VE_D)
#define VL_LN2G (VL_BO + VE_D)
#define VL_LN2B (VL_LN2G + VE_D)
#define VL_W1 (VL_LN2B + VE_D)
#define VL_B1 (VL_W1 + VE_FF * VE_D)
#define VL_W2 (VL_B1 + VE_FF)
#define VL_B2 (VL_W2 + VE_D * VE_FF)
#define VL_SIZE (VL_B2 + VE_D)
#define VE_LIN_SIZE (2 * VE_D * VE_D + VE_D)

__host__ __device__ constexpr long long ve_stack_floats(int num_layers) {
  return (long long)VE_LAYER0 + (long long)num_layers * VL_SIZE + (long long)((num_layers - 1) / 2) * VE_LIN_SIZE + 2 * VE_D;
}
// LDS bytes of a workgroup of `rt` row tiles with `nb` skip tensors
__host__ __device__ constexpr int ve_lds_bytes(int rt, int nb) {
  return 4 * (16 * rt * (VE_LDX * (1 + nb) + 3 * VE_LDH + 2) + 16);
}

struct VaeEncArgs {
  const float* w;          // packed weights: body block, then hands block
  long long stack_floats;  // ve_stack_floats(num_layers)
  const float* feats;      // [bs * nframes] rows of >= 189 floats, row_stride apart
  long long row_stride;
  const int* lengths;      // [bs]
  float* mulv;             // [2 (mu, logvar)][2 (body, hands)][n_seq][128]
  float* feats_out;        // [bs * nframes][189], root-subtracted
  int nframes, n_chunks, n_seq, num_layers;
};

#define VE_MFMA __builtin_amdgcn_mfma_f32_16x16x4f32

// acc[r][c] += A[16r .. 16r+15][k-steps kk0 .. kk1) . W[16 cts[c] ..]^T for r < nrt.  afrag(r, kk) returns the lane's float4 of A: row
// 16r + lane % 16, columns 16kk + 4 (lane / 16) .. +3 (the k-order inside a step is permuted identically in the packed B).
template <int NRT, int NC, class AF>
__device__ __forceinline__ void ve_mm(f32x4 (&acc)[NRT][NC], const AF& afrag, const float* __restrict__ W, int KK, const int (&cts)[NC], int kk0,
                                      int kk1, int nrt, int lane) {
  const f32x4* Bp = reinterpret_cast<const f32x4*>(W);
  f32x4 b[NC], bn[NC];
#pragma unroll
  for (int c = 0; c < NC; ++c) b[c] = Bp[((long long)cts[c] * KK + kk0) * 64 + lane];
  for (int kk = kk0; kk < kk1; ++kk) {
    if (kk + 1 < kk1) {
#pragma unroll
      for (int c = 0; c < NC; ++c) bn[c] = Bp[((long long)cts[c] * KK + kk + 1) * 64 + lane];
    }
#pragma unroll
    for (int r = 0; r < NRT; ++r) {
      if (r < nrt) {
        const f32x4 a = afrag(r, kk);
#pragma unroll
        for (int c = 0; c < NC; ++c) {
          acc[r][c] = VE_MFMA(a[0], b[c][0], acc[r][c], 0, 0, 0);
          acc[r][c] = VE_MFMA(a[1], b[c][1], acc[r][c], 0, 0, 0);
          acc[r][c] = VE_MFMA(a[2], b[c][2], acc[r][c], 0, 0, 0);
          acc[r][c] = VE_MFMA(a[3], b[c][3], acc[r][c], 0, 0, 0);
        }
      }
    }
#pragma unroll
    for (int c = 0; c < NC; ++c) b[c] = bn[c];
  }
}

template <int NRT, int NC>
__device__ __forceinline__ void ve_zero(f32x4 (&acc)[NRT][NC]) {
#pragma unroll
  for (int r = 0; r < NRT; ++r)
#pragma unroll
    for (int c = 0; c < NC; ++c) acc[r][c] = f32x4{0.f, 0.f, 0.f, 0.f};
}

// LayerNorm statistics (two-pass, biased variance, eps 1e-5) of rows [0, rows) of x: 4 lanes per row
__device__ __forceinline__ void ve_ln_stats(const float* x, float* mean, float* rstd, int rows, int tid) {
  const int p = tid & 3;
  for (int r = tid >> 2; r < rows; r += 64) {
    const float* xr = x + r * VE_LDX + 32 * p;
    float s = 0.f;
#pragma unroll
    for (int j = 0; j < 32; j += 4) {
      const f32x4 v = *reinterpret_cast<const f32x4*>(xr + j);
      s += (v[0] + v[1]) + (v[2] + v[3]);
    }
    s += __shfl_xor(s, 1);
    s += __shfl_xor(s, 2);
    const float m = s * (1.0f / VE_D);
    float q = 0.f;
#pragma unroll
    for (int j = 0; j < 32; j += 4) {
      const f32x4 v = *reinterpret_cast<const f32x4*>(xr + j);
      const float d0 = v[0] - m, d1 = v[1] - m, d2 = v[2] - m, d3 = v[3] - m;
      q += (d0 * d0 + d1 * d1) + (d2 * d2 + d3 * d3);
    }
    q += __shfl_xor(q, 1);
    q += __shfl_xor(q, 2);
    if (p == 0) {
      mean[r] = m;
      rstd[r] = 1.0f / sqrtf(q * (1.0f / VE_D) + 1e-5f);
    }
  }
}

__device__ __forceinline__ float ve_gelu(float v) { return 0.5f * v * (1.0f + erff(v * 0.70710678118654752f)); }

// One pre-norm TransformerEncoderLayer (cross_attention.py:288-300) on rows [0, 16 * nrt_all) of x.  last: only the first tile's rows
// are kept afterwards -- queries and everything after the keys / values run on that tile alone.  skip_out: x is also copied there.
template <int RT>
__device__ void ve_layer(float* x, float* U, float* mean, float* rstd, const int* nvalid, const float* __restrict__ L, int G, bool last,
                         float* skip_out, int tid) {
  const int lane = tid & 63, w = tid >> 6, l15 = lane & 15, q4 = lane >> 4;
  const int nq = last ? 1 : RT;   // row tiles whose result is kept
  float* Qb = U;
  float* Kb = U + 16 * RT * VE_LDH;
  float* Vb = Kb + 16 * RT * VE_LDH;
  const float* g1 = L + VL_LN1G;
  const float* b1n = L + VL_LN1B;
  auto a_ln1 = [&](int r, int kk) __attribute__((always_inline)) {
    const int row = 16 * r + l15, k = 16 * kk + 4 * q4;
    const f32x4 v = *reinterpret_cast<const f32x4*>(x + row * VE_LDX + k);
    const f32x4 g = *reinterpret_cast<const f32x4*>(g1 + k), bb = *reinterpret_cast<const f32x4*>(b1n + k);
    const float m = mean[row], s = rstd[row];
    f32x4 o;
#pragma unroll
    for (int j = 0; j < 4; ++j) o[j] = (v[j] - m) * s * g[j] + bb[j];
    return o;
  };

  ve_ln_stats(x, mean, rstd, 16 * RT, tid);
  __syncthreads();
  f32x4 ao[RT][2];
  ve_zero(ao);
  const float* bqkv = L + VL_BQKV;
  for (int h = 0; h < 2; ++h) {
    // Q_h, K_h, V_h: column tiles 4h + w, 8 + 4h + w, 16 + 4h + w of in_proj
    auto put = [&](const f32x4 (&acc)[RT][1], float* dst, int nrt, int boff, float scale) __attribute__((always_inline)) {
      const float bias = bqkv[boff + 64 * h + 16 * w + l15];
#pragma unroll
      for (int r = 0; r < RT; ++r)
        if (r < nrt)
#pragma unroll
          for (int i = 0; i < 4; ++i) dst[(16 * r + 4 * q4 + i) * VE_LDH + 16 * w + l15] = (acc[r][0][i] + bias) * scale;
    };
    {
      f32x4 aq[RT][1];
      ve_zero(aq);
      const int cq[1] = {4 * h + w};
      ve_mm<RT, 1>(aq, a_ln1, L + VL_WQKV, 8, cq, 0, 8, nq, lane);
      put(aq, Qb, nq, 0, 0.125f);   // 1 / sqrt(head_dim)
    }
    {
      f32x4 akv[RT][2];
      ve_zero(akv);
      const int ckv[2] = {8 + 4 * h + w, 16 + 4 * h + w};
      ve_mm<RT, 2>(akv, a_ln1, L + VL_WQKV, 8, ckv, 0, 8, RT, lane);
      f32x4 t[RT][1];
#pragma unroll
      for (int r = 0; r < RT; ++r) t[r][0] = akv[r][0];
      put(t, Kb, RT, VE_D, 1.0f);
#pragma unroll
      for (int r = 0; r < RT; ++r) t[r][0] = akv[r][1];
      put(t, Vb, RT, 2 * VE_D, 1.0f);
    }
    __syncthreads();
    // attention of head h: 4 lanes per query row, 16 head dimensions each; the result replaces the row's Q
    {
      const int p = tid & 3;
      for (int r = tid >> 2; r < 16 * nq; r += 64) {
        int seq, krow0 = -1;
        if (r < 2 * G) seq = r >> 1;
        else if (r < VE_T * G) seq = (r - 2 * G) >> 4;
        else seq = -1;
        float* qr = Qb + r * VE_LDH + 16 * p;
        if (seq < 0) {
#pragma unroll
          for (int j = 0; j < 16; ++j) qr[j] = 0.f;
          continue;
        }
        krow0 = 2 * G + 16 * seq;
        const int nv = nvalid[seq];
        float qv[16];
#pragma unroll
        for (int j = 0; j < 16; j += 4) {
          const f32x4 v = *reinterpret_cast<const f32x4*>(qr + j);
          qv[j] = v[0]; qv[j + 1] = v[1]; qv[j + 2] = v[2]; qv[j + 3] = v[3];
        }
        float s[VE_T];
#pragma unroll
        for (int key = 0; key < VE_T; ++key) {
          const int kr = key < 2 ? 2 * seq + key : krow0 + key - 2;
          const float* kp = Kb + kr * VE_LDH + 16 * p;
          float d = 0.f;
#pragma unroll
          for (int j = 0; j < 16; j += 4) {
            const f32x4 v = *reinterpret_cast<const f32x4*>(kp + j);
            d += qv[j] * v[0] + qv[j + 1] * v[1] + qv[j + 2] * v[2] + qv[j + 3] * v[3];
          }
          d += __shfl_xor(d, 1);
          d += __shfl_xor(d, 2);
          s[key] = d;
        }
        float mx = fmaxf(s[0], s[1]);
#pragma unroll
        for (int key = 2; key < VE_T; ++key)
          if (key - 2 < nv) mx = fmaxf(mx, s[key]);
        float sum = 0.f;
#pragma unroll
        for (int key = 0; key < VE_T; ++key) {
          const float e = (key < 2 || key - 2 < nv) ? expf(s[key] - mx) : 0.f;
          s[key] = e;
          sum += e;
        }
        const float inv = 1.0f / sum;
        float o[16];
#pragma unroll
        for (int j = 0; j < 16; ++j) o[j] = 0.f;
#pragma unroll
        for (int key = 0; key < VE_T; ++key) {
          const int kr = key < 2 ? 2 * seq + key : krow0 + key - 2;
          const float* vp = Vb + kr * VE_LDH + 16 * p;
          const float pk = s[key] * inv;
#pragma unroll
          for (int j = 0; j < 16; j += 4) {
            const f32x4 v = *reinterpret_cast<const f32x4*>(vp + j);
            o[j] += pk * v[0]; o[j + 1] += pk * v[1]; o[j + 2] += pk * v[2]; o[j + 3] += pk * v[3];
          }
        }
#pragma unroll
        for (int j = 0; j < 16; j += 4) *reinterpret_cast<f32x4*>(qr + j) = f32x4{o[j], o[j + 1], o[j + 2], o[j + 3]};
      }
    }
    __syncthreads();
    // out-projection, head h's 64 input columns (k-steps 4h .. 4h+3 of out_proj.weight)
    {
      auto a_o = [&](int r, int kk) __attribute__((always_inline)) {
        return *reinterpret_cast<const f32x4*>(Qb + (16 * r + l15) * VE_LDH + 16 * (kk - 4 * h) + 4 * q4);
      };
      const int co[2] = {2 * w, 2 * w + 1};
      ve_mm<RT, 2>(ao, a_o, L + VL_WO, 8, co, 4 * h, 4 * h + 4, nq, lane);
    }
    __syncthreads();
  }
  // x += attention
#pragma unroll
  for (int r = 0; r < RT; ++r)
    if (r < nq)
#pragma unroll
      for (int c = 0; c < 2; ++c) {
        const int col = 16 * (2 * w + c) + l15;
        const float bias = L[VL_BO + col];
#pragma unroll
        for (int i = 0; i < 4; ++i) x[(16 * r + 4 * q4 + i) * VE_LDX + col] += ao[r][c][i] + bias;
      }
  __syncthreads();
  ve_ln_stats(x, mean, rstd, 16 * nq, tid);
  __syncthreads();
  // FFN in 128-column chunks of the hidden: H = gelu(LN2(x) W1c^T + b1c) in LDS, acc += H W2[:, c]^T
  const float* g2 = L + VL_LN2G;
  const float* b2n = L + VL_LN2B;
  auto a_ln2 = [&](int r, int kk) __attribute__((always_inline)) {
    const int row = 16 * r + l15, k = 16 * kk + 4 * q4;
    const f32x4 v = *reinterpret_cast<const f32x4*>(x + row * VE_LDX + k);
    const f32x4 g = *reinterpret_cast<const f32x4*>(g2 + k), bb = *reinterpret_cast<const f32x4*>(b2n + k);
    const float m = mean[row], s = rstd[row];
    f32x4 o;
#pragma unroll
    for (int j = 0; j < 4; ++j) o[j] = (v[j] - m) * s * g[j] + bb[j];
    return o;
  };
  float* Hb = U;
  f32x4 af[RT][2];
  ve_zero(af);
  for (int ch = 0; ch < VE_FF / VE_D; ++ch) {
    {
      f32x4 ah[RT][2];
      ve_zero(ah);
      const int c1[2] = {8 * ch + 2 * w, 8 * ch + 2 * w + 1};
      ve_mm<RT, 2>(ah, a_ln2, L + VL_W1, 8, c1, 0, 8, nq, lane);
#pragma unroll
      for (int r = 0; r < RT; ++r)
        if (r < nq)
#pragma unroll
          for (int c = 0; c < 2; ++c) {
            const int col = 16 * (2 * w + c) + l15;
            const float bias = L[VL_B1 + VE_D * ch + col];
#pragma unroll
            for (int i = 0; i < 4; ++i) Hb[(16 * r + 4 * q4 + i) * VE_LDX + col] = ve_gelu(ah[r][c][i] + bias);
          }
    }
    __syncthreads();
    auto a_h = [&](int r, int kk) __attribute__((always_inline)) {
      return *reinterpret_cast<const f32x4*>(Hb + (16 * r + l15) * VE_LDX + 16 * (kk - 8 * ch) + 4 * q4);
    };
    const int c2[2] = {2 * w, 2 * w + 1};
    ve_mm<RT, 2>(af, a_h, L + VL_W2, VE_FF / 16, c2, 8 * ch, 8 * ch + 8, nq, lane);
    __syncthreads();
  }
#pragma unroll
  for (int r = 0; r < RT; ++r)
    if (r < nq)
#pragma unroll
      for (int c = 0; c < 2; ++c) {
        const int col = 16 * (2 * w + c) + l15;
        const float bias = L[VL_B2 + col];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int row = 16 * r + 4 * q4 + i;
          const float v = x[row * VE_LDX + col] + (af[r][c][i] + bias);
          x[row * VE_LDX + col] = v;
          if (skip_out) skip_out[row * VE_LDX + col] = v;
        }
      }
  __syncthreads();
}

template <int RT>
__global__ void __launch_bounds__(256) vae_encode_kernel(const VaeEncArgs a) {
  extern __shared__ float ve_smem[];
  constexpr int R = 16 * RT;
  constexpr int G = R / VE_T;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, l15 = lane & 15, q4 = lane >> 4;
  const int stack = blockIdx.y;   // 0 body, 1 hands
  const int seq0 = blockIdx.x * G;
  const int nb = (a.num_layers - 1) / 2;
  float* x = ve_smem;
  float* skips = x + R * VE_LDX;
  float* U = skips + nb * R * VE_LDX;
  float* mean = U + 3 * R * VE_LDH;
  float* rstd = mean + R;
  int* nvalid = reinterpret_cast<int*>(rstd + R);
  const float* W = a.w + stack * a.stack_floats;

  if (tid < G) {   // valid frames per sequence of this group (vae.py:176,185: lengths_to_mask, chunked); absent sequences: none
    const int sq = seq0 + tid;
    int nv = 0;
    if (sq < a.n_seq) {
      const int b = sq / a.n_chunks, c = sq % a.n_chunks;
      nv = min(max(a.lengths[b] - 16 * c, 0), 16);
    }
    nvalid[tid] = nv;
  }
  // load stage: root subtraction (vae.py:184-187), the stack's feature columns zero-padded to 128 in U, the returned features
  const int c0 = stack ? VE_BODY : 0, nf = stack ? VE_HANDS : VE_BODY;
  for (int idx = tid; idx < R * VE_D; idx += 256) {
    const int row = idx >> 7, k = idx & (VE_D - 1);
    float v = 0.f;
    const int fr = row - 2 * G, i = fr >> 4, f = fr & 15;
    if (fr >= 0 && i < G && seq0 + i < a.n_seq && k < nf) {
      const int sq = seq0 + i, b = sq / a.n_chunks, c = sq % a.n_chunks;
      const long long frow = (long long)b * a.nframes + 16 * c + f;
      v = a.feats[frow * a.row_stride + c0 + k];
      if (!stack && k < 3) {
        const float root = a.feats[((long long)b * a.nframes + 16 * c) * a.row_stride + k];
        const float rxz = root * (k == 1 ? 0.0f : 1.0f);   // root_pos_init * [1, 0, 1]
        v = v - rxz;
      }
      a.feats_out[frow * VE_NFEATS + c0 + k] = v;
    }
    U[row * VE_LDX + k] = v;
  }
  __syncthreads();
  // skeleton embedding + global tokens + PE (vae.py:193-233)
  {
    f32x4 acc[RT][2];
    ve_zero(acc);
    auto a_in = [&](int r, int kk) __attribute__((always_inline)) {
      return *reinterpret_cast<const f32x4*>(U + (16 * r + l15) * VE_LDX + 16 * kk + 4 * q4);
    };
    const int ce[2] = {2 * w, 2 * w + 1};
    ve_mm<RT, 2>(acc, a_in, W + VE_EMB_W, 8, ce, 0, stack ? 8 : (VE_BODY + 15) / 16, RT, lane);
#pragma unroll
    for (int r = 0; r < RT; ++r)
#pragma unroll
      for (int c = 0; c < 2; ++c) {
        const int col = 16 * (2 * w + c) + l15;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int row = 16 * r + 4 * q4 + i;
          float v = 0.f;
          if (row < 2 * G) v = W[VE_TOK + (row & 1) * VE_D + col] + W[VE_PE + (row & 1) * VE_D + col];
          else if (row < VE_T * G) v = (acc[r][c][i] + W[VE_EMB_B + col]) + W[VE_PE + (2 + ((row - 2 * G) & 15)) * VE_D + col];
          x[row * VE_LDX + col] = v;
        }
      }
  }
  __syncthreads();
  // SkipTransformerEncoder (cross_attention.py:41-64)
  const int nl = a.num_layers;
  for (int l = 0; l < nl; ++l) {
    const float* L = W + VE_LAYER0 + (long long)l * VL_SIZE;
    if (l > nb) {   // output block l - nb - 1: x = linear(cat(x, skips.pop()))
      const int j = l - nb - 1;
      const float* sk = skips + (nb - 1 - j) * R * VE_LDX;
      const float* Wl = W + VE_LAYER0 + (long long)nl * VL_SIZE + (long long)j * VE_LIN_SIZE;
      f32x4 acc[RT][2];
      ve_zero(acc);
      auto a_cat = [&](int r, int kk) __attribute__((always_inline)) {
        const float* src = kk < 8 ? x + 16 * kk : sk + 16 * (kk - 8);
        return *reinterpret_cast<const f32x4*>(src + (16 * r + l15) * VE_LDX + 4 * q4);
      };
      const int cl[2] = {2 * w, 2 * w + 1};
      ve_mm<RT, 2>(acc, a_cat, Wl, 16, cl, 0, 16, RT, lane);
      __syncthreads();
#pragma unroll
      for (int r = 0; r < RT; ++r)
#pragma unroll
        for (int c = 0; c < 2; ++c) {
          const int col = 16 * (2 * w + c) + l15;
          const float bias = Wl[2 * VE_D * VE_D + col];
#pragma unroll
          for (int i = 0; i < 4; ++i) x[(16 * r + 4 * q4 + i) * VE_LDX + col] = acc[r][c][i] + bias;
        }
      __syncthreads();
    }
    ve_layer<RT>(x, U, mean, rstd, nvalid, L, G, l == nl - 1, l < nb ? skips + l * R * VE_LDX : nullptr, tid);
  }
  // final LayerNorm of the 2G global-token rows; token 0 -> mu, token 1 -> logvar (vae.py:240-254)
  ve_ln_stats(x, mean, rstd, 2 * G, tid);
  __syncthreads();
  const float* gn = W + a.stack_floats - 2 * VE_D;
  for (int idx = tid; idx < 2 * G * VE_D; idx += 256) {
    const int row = idx >> 7, col = idx & (VE_D - 1), sq = seq0 + (row >> 1);
    if (sq >= a.n_seq) continue;
    const float v = (x[row * VE_LDX + col] - mean[row]) * rstd[row] * gn[col] + gn[VE_D + col];
    a.mulv[(((long long)(row & 1) * 2 + stack) * a.n_seq + sq) * VE_D + col] = v;
  }
}
