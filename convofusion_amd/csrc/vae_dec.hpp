// ConvoFusionVae.decode with its vector-Jacobian product with respect to z (cfd_vae_decode_vjp): a forward of both SkipTransformerDecoders
// (reference vae.py:268-372, SkipTransformerDecoder cross_attention.py:66-125, TransformerDecoderLayer.forward_pre :361-382) that saves what
// the reverse sweep needs, and the sweep from a cotangent at the 189 output features back to the latents.  Exact float32 throughout
// (v_mfma_f32_16x16x4_f32 on the packed-weight order of vae_enc.hpp, VALU softmax and LayerNorm); no atomics: every sum has one fixed order.
//
// Unit of work: one 16-frame row tile of one (stack, sequence): grid (tiles, bs, 2), 256 threads.  Everything but the self-attention core
// is local to a row, so a layer costs two launches each way, and both stacks and all sequences share every grid:
//   forward   vd_mem_kernel                 K | V of the memory z[s] + mem_pos_decoder.pe for every layer (the only place z enters)
//             vd_fwd_rows_kernel(l), l = 0 .. nl: the rest of layer l - 1 behind its self-attention core (out-projection, cross-attention,
//                                           FFN), the skip linear in front of an output block, layer l's LN1 and q | k | v; at l = nl the
//                                           final norm, final_layer and the length mask instead
//             vd_self_fwd_kernel(l)         the self-attention core of the tile's 16 queries over the sequence's valid keys
//   sweep     vd_bwd_rows_kernel(l), l = nl - 1 .. 0: the head (final_layer, final norm) or layer l + 1's LN1 / q | k | v / skip linear
//                                           backward, then layer l from its output down to its self-attention core: FFN (pre-activation
//                                           recomputed in 128-column chunks), cross-attention (probabilities recomputed; dQ to the stream,
//                                           the tile's partial dK | dV of the memory to its own slot), the out-projection
//             vd_self_bwd_kernel(l), l >= 1: dQ of the tile's queries, then dK | dV of the tile's keys summed over the queries in order
//                                           (layer 0's queries are constants: its self-attention gets no backward)
//             vd_dz_kernel                  per (stack, sequence, layer): the partial dK | dV summed over the tiles in order, times W_k | W_v
//             vd_dz_sum_kernel              the layers' contributions added up in order: d_z
// Saved per row and layer: the stream at three points (layer input, behind self-attention, behind cross-attention), q | k | v, the
// self-attention output and log-sum-exp, the scaled cross-attention query.  Recomputed: LayerNorm statistics, both softmaxes, the FFN hidden.
// Frames at or beyond lengths[b] never act as keys and carry a zero cotangent; tiles that hold only such frames are skipped (they only write
// the zeros of their rows of feats and of the gradient tap g).
//
// The forward kernels carry a compile-time SAVE flag.  SAVE = true is the forward above, every layer's buffers resident for the sweep
// (cfd_vae_decode_vjp; cfd_vae_decode with a ticket, whose vd_mem launch also copies the lengths and -- for a sweep in a later call -- the
// stacks' weights into the workspace).  SAVE = false is the forward on its own (cfd_vae_decode without a ticket): the same arithmetic in the
// same order, storing only what a later forward launch reads -- the stream hand-off and the skip tensors (vd_xslot), q | k | v and o of
// the current layer (vd_lslot), the memory's K | V -- so its output has the saving forward's bits on (nb + 6) / 2 KB per row instead of 27.
//
// Packed weights (float32): one block per stack (body, then hands; vd_stack_floats(num_layers) each), then query_pos_decoder.pe[0:256]
// and mem_pos_decoder.pe[0:16].  A matrix W [N][K] (nn.Linear) is stored twice: in the MFMA-B order of vae_enc.hpp ("F": float4 index
// ((n/16 * K/16 + k/16) * 64 + lane), lane = 16 * ((k % 16) / 4) + n % 16, element k % 4) and as its transpose W^T [K][N] in the same
// order ("T": the B operand of dX = dY . W) -- built by convofusion_amd/vae.py (_decoder_pack):
//   per layer (input_blocks..., middle_block, output_blocks...): norm1 w, b; self_attn.in_proj_weight F, T; in_proj_bias [384];
//     self_attn.out_proj.weight F, T; bias; norm2 w, b; multihead_attn.in_proj_weight F, T; in_proj_bias; multihead_attn.out_proj.weight
//     F, T; bias; norm3 w, b; linear1.weight F, T; bias [1024]; linear2.weight F, T; bias,
//   per linear block: weight [128][256] F, T; bias,
//   norm w, b; final_layer.weight (rows zero-padded from 69 / 120 to 128) F, T; final_layer.bias (zero-padded to 128).
#pragma once
#include <hip/hip_runtime.h>

#include "vae_enc.hpp"

#define VD_MAX_FRAMES 256
#define VD_MAX_CHUNKS 16
#define VD_LD VE_LDX          // LDS row stride of a [16][128] tile
#define VD_LD3 (3 * VE_D + 4)  // ... of a [16][384] tile

// float offsets inside a layer
#define DL_LN1G 0
#define DL_LN1B (DL_LN1G + VE_D)
#define DL_SA_W (DL_LN1B + VE_D)
#define DL_SA_WT (DL_SA_W + 3 * VE_D * VE_D)
#define DL_SA_B (DL_SA_WT + 3 * VE_D * VE_D)
#define DL_SO_W (DL_SA_B + 3 * VE_D)
#define DL_SO_WT (DL_SO_W + VE_D * VE_D)
#define DL_SO_B (DL_SO_WT + VE_D * VE_D)
#define DL_LN2G (DL_SO_B + VE_D)
#define DL_LN2B (DL_LN2G + VE_D)
#define DL_CA_W (DL_LN2B + VE_D)
#define DL_CA_WT (DL_CA_W + 3 * VE_D * VE_D)
#define DL_CA_B (DL_CA_WT + 3 * VE_D * VE_D)
#define DL_CO_W (DL_CA_B + 3 * VE_D)
#define DL_CO_WT (DL_CO_W + VE_D * VE_D)
#define DL_CO_B (DL_CO_WT + VE_D * VE_D)
#define DL_LN3G (DL_CO_B + VE_D)
#define DL_LN3B (DL_LN3G + VE_D)
#define DL_W1 (DL_LN3B + VE_D)
#define DL_W1T (DL_W1 + VE_FF * VE_D)
#define DL_B1 (DL_W1T + VE_FF * VE_D)
#define DL_W2 (DL_B1 + VE_FF)
#define DL_W2T (DL_W2 + VE_FF * VE_D)
#define DL_B2 (DL_W2T + VE_FF * VE_D)
#define DL_SIZE (DL_B2 + VE_D)
// a linear block
#define DLIN_W 0
#define DLIN_WT (2 * VE_D * VE_D)
#define DLIN_B (4 * VE_D * VE_D)
#define DLIN_SIZE (4 * VE_D * VE_D + VE_D)
// the tail of a stack's block
#define DT_NG 0
#define DT_NB VE_D
#define DT_FW (2 * VE_D)
#define DT_FWT (DT_FW + VE_D * VE_D)
#define DT_FB (DT_FWT + VE_D * VE_D)
#define DT_SIZE (DT_FB + VE_D)

__host__ __device__ constexpr long long vd_stack_floats(int nl) {
  return (long long)nl * DL_SIZE + (long long)((nl - 1) / 2) * DLIN_SIZE + DT_SIZE;
}
__host__ __device__ constexpr long long vd_pack_floats(int nl) {
  return 2 * vd_stack_floats(nl) + (long long)(VD_MAX_FRAMES + VD_MAX_CHUNKS) * VE_D;
}

struct VaeDecArgs {
  const float* w;            // the pack
  long long stack_floats;
  const float* qpe;          // query_pos_decoder.pe rows (inside the pack)
  const float* mpe;          // mem_pos_decoder.pe rows
  const float* z;            // [2][bs][n_chunks][128]
  const int* lengths;        // [bs]
  const float* d_feats;      // [bs][nframes][189]
  float* feats;              // [bs][nframes][189] or null
  float* d_z;                // [2][bs][n_chunks][128]
  int bs, nframes, fp, nt, n_chunks, nl, nb;
  long long rows;            // 2 * bs * fp; row ((s * bs + b) * fp + f)
  // workspace: per layer l (stride `rows` rows) unless noted
  float* x0;     // [nl + 1][rows][128]  layer l's input (behind the skip linear); [nl]: the last layer's output
  float* x1;     // [nl][rows][128]      behind the self-attention
  float* x2;     // [nl][rows][128]      behind the cross-attention
  float* qkv;    // [nl][rows][384]      q (scaled by 1/8) | k | v of the self-attention
  float* o;      // [nl][rows][128]      the self-attention core's output
  float* lse;    // [nl][rows][2]        its log-sum-exp per head
  float* qc;     // [nl][rows][128]      the cross-attention's scaled query
  float* mkv;    // [nl][2 * bs][16][256]   K | V of the memory
  float* g;      // [nl][rows][128]      the running gradient at layer l's output (tap "vae.g.l")
  float* g1;     // [rows][128]          ... behind layer l's self-attention, handed to the next launch of the sweep
  float* d_o;    // [rows][128]          at the self-attention core's output
  float* dd;     // [rows][2]            sum_j P_ij dP_ij = dO_i . O_i per head
  float* dqkv;   // [rows][384]
  float* gskip;  // [nb][rows][128]      the skip tensors' gradient from the linear blocks
  float* pkv;    // [nl][2 * bs][nt][16][256]  per-tile partial dK | dV of the memory
  float* dzl;    // [nl][2][bs][16][128] layer l's contribution to d_z (tap "vae.dz.l")
  // what a kept forward (SAVE) copies out of the caller's memory for a sweep that runs in a later call: vd_mem_kernel's extra blocks
  float* keep_w;     // [2 * stack_floats]  the two stacks' blocks of the pack
  int* keep_len;     // [bs]                the lengths
};

// Where layer l's buffers live.  SAVE: every layer keeps its own (the sweep reads them).  Forward-only: what a later forward launch still
// reads and no more -- q | k | v and o of the current layer in slot 0; the stream in nb + 2 slots: the inputs of layers 1 .. nb, which
// are the skip tensors of the output blocks, in slots 1 .. nb, every other layer's input alternating between slots 0 and nb + 1, so a
// launch never writes the slot it reads.
template <bool SAVE>
__device__ __forceinline__ int vd_xslot(int l, int nb) {
  if (SAVE || (l >= 1 && l <= nb)) return l;
  return (l > nb && ((l - nb) & 1)) ? nb + 1 : 0;
}
template <bool SAVE>
__device__ __forceinline__ int vd_lslot(int l) { return SAVE ? l : 0; }

// A fragment of a [16][*] LDS tile: k-step kk reads columns 16 (kk - k0) ..
struct VdTile {
  const float* p;
  int ld, k0, l15, q4;
  __device__ __forceinline__ f32x4 operator()(int, int kk) const { return *reinterpret_cast<const f32x4*>(p + l15 * ld + 16 * (kk - k0) + 4 * q4); }
};
// ... with a LayerNorm applied while it is read
struct VdTileLn {
  const float* x;
  const float *mean, *rstd, *g, *b;
  int l15, q4;
  __device__ __forceinline__ f32x4 operator()(int, int kk) const {
    const int k = 16 * kk + 4 * q4;
    const f32x4 v = *reinterpret_cast<const f32x4*>(x + l15 * VD_LD + k);
    const f32x4 gg = *reinterpret_cast<const f32x4*>(g + k), bb = *reinterpret_cast<const f32x4*>(b + k);
    const float m = mean[l15], s = rstd[l15];
    f32x4 o;
#pragma unroll
    for (int j = 0; j < 4; ++j) o[j] = (v[j] - m) * s * gg[j] + bb[j];
    return o;
  }
};
// ... of cat([x, skip]) (256 columns)
struct VdTileCat {
  const float *x, *sk;
  int l15, q4;
  __device__ __forceinline__ f32x4 operator()(int, int kk) const {
    const float* src = kk < 8 ? x + 16 * kk : sk + 16 * (kk - 8);
    return *reinterpret_cast<const f32x4*>(src + l15 * VD_LD + 4 * q4);
  }
};

// acc = A . W^T for the 128 output columns whose first column tile is ct0: wave w owns column tiles ct0 + 2w, ct0 + 2w + 1; W has KK k-steps
// per column tile, of which [kk0, kk1) are summed.  acc[c][i] is row 4 (lane / 16) + i, column 16 (2w + c) + lane % 16 of the chunk.
// ve_mm's product and order of sums, with the weights fetched VD_PF k-steps ahead: at 16 rows per workgroup a k-step is 8 MFMAs, far
// shorter than a fetch from L2.
#define VD_PF 4
template <class AF>
__device__ __forceinline__ void vd_mm(f32x4 (&acc)[1][2], const AF& a, const float* __restrict__ W, int KK, int ct0, int kk0, int kk1, int w, int lane) {
  const f32x4* B0 = reinterpret_cast<const f32x4*>(W) + (long long)(ct0 + 2 * w) * KK * 64 + lane;
  const f32x4* B1 = B0 + (long long)KK * 64;
  f32x4 b0[VD_PF], b1[VD_PF];
#pragma unroll
  for (int i = 0; i < VD_PF; ++i)
    if (kk0 + i < kk1) {
      b0[i] = B0[(kk0 + i) * 64];
      b1[i] = B1[(kk0 + i) * 64];
    }
  for (int kk = kk0; kk < kk1; kk += VD_PF) {
#pragma unroll
    for (int i = 0; i < VD_PF; ++i) {
      if (kk + i < kk1) {
        const f32x4 av = a(0, kk + i);
        const f32x4 x0 = b0[i], x1 = b1[i];
        if (kk + i + VD_PF < kk1) {
          b0[i] = B0[(kk + i + VD_PF) * 64];
          b1[i] = B1[(kk + i + VD_PF) * 64];
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          acc[0][0] = VE_MFMA(av[j], x0[j], acc[0][0], 0, 0, 0);
          acc[0][1] = VE_MFMA(av[j], x1[j], acc[0][1], 0, 0, 0);
        }
      }
    }
  }
}

// f(row, col, value) for every accumulator element of the wave
template <class F>
__device__ __forceinline__ void vd_each(const f32x4 (&acc)[1][2], int w, int lane, F&& f) {
  const int l15 = lane & 15, q4 = lane >> 4;
#pragma unroll
  for (int c = 0; c < 2; ++c)
#pragma unroll
    for (int i = 0; i < 4; ++i) f(4 * q4 + i, 16 * (2 * w + c) + l15, acc[0][c][i]);
}

__device__ __forceinline__ void vd_load_tile(float* dst, const float* __restrict__ src, int tid) {   // [16][128] global rows -> LDS
  for (int idx = tid; idx < 16 * 32; idx += 256) {
    const int r = idx >> 5, c = (idx & 31) * 4;
    *reinterpret_cast<f32x4*>(dst + r * VD_LD + c) = *reinterpret_cast<const f32x4*>(src + r * VE_D + c);
  }
}
__device__ __forceinline__ void vd_store_tile(float* __restrict__ dst, const float* src, int tid) {   // LDS -> [16][128] global rows
  for (int idx = tid; idx < 16 * 32; idx += 256) {
    const int r = idx >> 5, c = (idx & 31) * 4;
    *reinterpret_cast<f32x4*>(dst + r * VE_D + c) = *reinterpret_cast<const f32x4*>(src + r * VD_LD + c);
  }
}

__device__ __forceinline__ float vd_sum8(float v) {
  v += __shfl_xor(v, 1);
  v += __shfl_xor(v, 2);
  v += __shfl_xor(v, 4);
  return v;
}
__device__ __forceinline__ float vd_sum16(float v) {
  v = vd_sum8(v);
  v += __shfl_xor(v, 8);
  return v;
}

__device__ __forceinline__ float vd_gelu_grad(float v) {
  return 0.5f * (1.0f + erff(v * 0.70710678118654752f)) + v * expf(-0.5f * v * v) * 0.39894228040143268f;
}

// gb (+)= LayerNorm backward of the tile: x the LayerNorm's input (statistics in mean / rstd), dy the gradient at its output.  16 lanes per
// row, 8 columns each.  base: null (gb += ...) or the [16][128] global rows gb is set from (gb = base + ...).
__device__ __forceinline__ void vd_ln_bwd(float* gb, const float* x, const float* mean, const float* rstd, const float* __restrict__ gamma,
                                          const float* dy, const float* __restrict__ base, int tid) {
  const int r = tid >> 4, c0 = (tid & 15) * 8;
  const float m = mean[r], s = rstd[r];
  float xh[8], dh[8], a = 0.f, b = 0.f;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    xh[j] = (x[r * VD_LD + c0 + j] - m) * s;
    dh[j] = dy[r * VD_LD + c0 + j] * gamma[c0 + j];
    a += dh[j];
    b += dh[j] * xh[j];
  }
  a = vd_sum16(a) * (1.0f / VE_D);
  b = vd_sum16(b) * (1.0f / VE_D);
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const float v = s * (dh[j] - a - xh[j] * b);
    const float old = base ? base[r * VE_D + c0 + j] : gb[r * VD_LD + c0 + j];
    gb[r * VD_LD + c0 + j] = old + v;
  }
}

// ---- forward ------------------------------------------------------------------------------------------------------------------------------
// K | V of the memory for layer blockIdx.x, sequence blockIdx.y, stack blockIdx.z.  SAVE: block (0, b, 0) copies lengths[b] to keep_len, and
// the blocks with blockIdx.x >= nl -- a launch that keeps the weights for a later call has some -- share the copy of the stacks' weights to
// keep_w (float4 cb * 256 + tid of block cb, then every (blocks * 256)-th).
template <bool SAVE>
__global__ void __launch_bounds__(256) vd_mem_kernel(const VaeDecArgs a) {
  __shared__ float A[16 * VD_LD];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, l15 = lane & 15, q4 = lane >> 4;
  const int l = blockIdx.x, b = blockIdx.y, s = blockIdx.z;
  if (SAVE) {
    if (l >= a.nl) {
      const long long n4 = a.stack_floats / 2, blocks = (long long)(gridDim.x - a.nl) * gridDim.y * 2;
      const long long cb = ((long long)(l - a.nl) * gridDim.y + b) * 2 + s;
      const f32x4* __restrict__ src = reinterpret_cast<const f32x4*>(a.w);
      f32x4* __restrict__ dst = reinterpret_cast<f32x4*>(a.keep_w);
      for (long long i = cb * 256 + tid; i < n4; i += blocks * 256) dst[i] = src[i];
      return;
    }
    if (l == 0 && s == 0 && tid == 0) a.keep_len[b] = a.lengths[b];
  }
  const float* L = a.w + s * a.stack_floats + (long long)l * DL_SIZE;
  for (int idx = tid; idx < 16 * VE_D; idx += 256) {
    const int j = idx >> 7, c = idx & 127;
    A[j * VD_LD + c] = j < a.n_chunks ? a.z[(((long long)s * a.bs + b) * a.n_chunks + j) * VE_D + c] + a.mpe[j * VE_D + c] : 0.f;
  }
  __syncthreads();
  float* out = a.mkv + (((long long)l * 2 * a.bs) + (long long)s * a.bs + b) * 16 * 256;
  const VdTile at{A, VD_LD, 0, l15, q4};
  for (int kv = 0; kv < 2; ++kv) {
    f32x4 acc[1][2];
    ve_zero(acc);
    vd_mm(acc, at, L + DL_CA_W, 8, 8 + 8 * kv, 0, 8, w, lane);
    vd_each(acc, w, lane, [&](int r, int c, float v) { out[r * 256 + 128 * kv + c] = v + L[DL_CA_B + VE_D * (1 + kv) + c]; });
  }
}

// The cross-attention of the tile's rows against the <= 16 memory rows: thread = (row tid / 16, head (tid / 8) % 2, 8 of the head's 64
// dimensions).  q (scaled) is read from `q`; with d_o null the attention output replaces it (forward).  With d_o: the sweep -- the gradient
// at the scaled query's projection output (times 1/8) goes to dq, the probabilities and dS to ps / ds [16][2][16].
__device__ __forceinline__ void vd_cross(float* q, const float* d_o, float* dq, float* ps, float* ds, const float* __restrict__ mkv, int nc, int tid) {
  const int r = tid >> 4, h = (tid >> 3) & 1, p = tid & 7, c0 = 64 * h + 8 * p;
  float qv[8], sc[VD_MAX_CHUNKS];
#pragma unroll
  for (int j = 0; j < 8; ++j) qv[j] = q[r * VD_LD + c0 + j];
  float mx = -INFINITY;
#pragma unroll
  for (int k = 0; k < VD_MAX_CHUNKS; ++k) {
    float d = 0.f;
    if (k < nc) {
      const float* kp = mkv + k * 256 + c0;
#pragma unroll
      for (int j = 0; j < 8; ++j) d += qv[j] * kp[j];
    }
    d = vd_sum8(d);
    sc[k] = d;
    if (k < nc) mx = fmaxf(mx, d);
  }
  float sum = 0.f;
#pragma unroll
  for (int k = 0; k < VD_MAX_CHUNKS; ++k) {
    sc[k] = k < nc ? expf(sc[k] - mx) : 0.f;
    sum += sc[k];
  }
  const float inv = 1.0f / sum;
  if (!d_o) {
    float o[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) o[j] = 0.f;
#pragma unroll
    for (int k = 0; k < VD_MAX_CHUNKS; ++k)
      if (k < nc) {
        const float* vp = mkv + k * 256 + 128 + c0;
        const float pk = sc[k] * inv;
#pragma unroll
        for (int j = 0; j < 8; ++j) o[j] += pk * vp[j];
      }
#pragma unroll
    for (int j = 0; j < 8; ++j) q[r * VD_LD + c0 + j] = o[j];
    return;
  }
  float dov[8], dp[VD_MAX_CHUNKS], dsum = 0.f;
#pragma unroll
  for (int j = 0; j < 8; ++j) dov[j] = d_o[r * VD_LD + c0 + j];
#pragma unroll
  for (int k = 0; k < VD_MAX_CHUNKS; ++k) {
    float d = 0.f;
    if (k < nc) {
      const float* vp = mkv + k * 256 + 128 + c0;
#pragma unroll
      for (int j = 0; j < 8; ++j) d += dov[j] * vp[j];
    }
    d = vd_sum8(d);
    sc[k] *= inv;
    dp[k] = d;
    dsum += sc[k] * d;
  }
  float g[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) g[j] = 0.f;
#pragma unroll
  for (int k = 0; k < VD_MAX_CHUNKS; ++k) {
    const float dsk = sc[k] * (dp[k] - dsum);
    if (k < nc) {
      const float* kp = mkv + k * 256 + c0;
#pragma unroll
      for (int j = 0; j < 8; ++j) g[j] += dsk * kp[j];
    }
    if (p == 0) {
      ps[(r * 2 + h) * 16 + k] = sc[k];
      ds[(r * 2 + h) * 16 + k] = dsk;
    }
  }
#pragma unroll
  for (int j = 0; j < 8; ++j) dq[r * VD_LD + c0 + j] = 0.125f * g[j];
}

// Launch l of the forward's row-local part (see the head of the file).  SAVE = false: the same arithmetic in the same order on the
// forward-only slots (vd_xslot, vd_lslot), without the stores only the sweep reads (x1, qc, x2, the last layer's output).
template <bool SAVE>
__global__ void __launch_bounds__(256) vd_fwd_rows_kernel(const VaeDecArgs a, int l) {
  __shared__ float X[16 * VD_LD], A[16 * VD_LD], Hb[16 * VD_LD], mean[16], rstd[16];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, l15 = lane & 15, q4 = lane >> 4;
  const int t = blockIdx.x, b = blockIdx.y, s = blockIdx.z;
  const int len = min(a.lengths[b], a.nframes);
  if (16 * t >= len) {   // a tile wholly beyond the length: nothing to compute; its rows of feats are the zeros of the length mask
    if (l == a.nl && a.feats) {
      const int c0 = s ? VE_BODY : 0, nf = s ? VE_HANDS : VE_BODY;
      for (int idx = tid; idx < 16 * nf; idx += 256) {
        const int f = 16 * t + idx / nf;
        if (f < a.nframes) a.feats[((long long)b * a.nframes + f) * VE_NFEATS + c0 + idx % nf] = 0.f;
      }
    }
    return;
  }
  const float* W = a.w + s * a.stack_floats;
  const long long sb = (long long)s * a.bs + b, row0 = sb * a.fp + 16 * t;
  const VdTile atA{A, VD_LD, 0, l15, q4};
  if (l == 0) {
    vd_load_tile(X, a.qpe + (long long)16 * t * VE_D, tid);
    __syncthreads();
  } else {
    const int lp = l - 1;
    const float* L = W + (long long)lp * DL_SIZE;
    const long long off = ((long long)lp * a.rows + row0) * VE_D;
    vd_load_tile(X, a.x0 + ((long long)vd_xslot<SAVE>(lp, a.nb) * a.rows + row0) * VE_D, tid);
    vd_load_tile(A, a.o + ((long long)vd_lslot<SAVE>(lp) * a.rows + row0) * VE_D, tid);
    __syncthreads();
    {   // self-attention out-projection and residual
      f32x4 acc[1][2];
      ve_zero(acc);
      vd_mm(acc, atA, L + DL_SO_W, 8, 0, 0, 8, w, lane);
      vd_each(acc, w, lane, [&](int r, int c, float v) { X[r * VD_LD + c] += v + L[DL_SO_B + c]; });
    }
    __syncthreads();
    if (SAVE) vd_store_tile(a.x1 + off, X, tid);
    ve_ln_stats(X, mean, rstd, 16, tid);
    __syncthreads();
    {   // cross-attention: scaled query, attention over the memory rows, out-projection and residual
      f32x4 acc[1][2];
      ve_zero(acc);
      const VdTileLn an{X, mean, rstd, L + DL_LN2G, L + DL_LN2B, l15, q4};
      vd_mm(acc, an, L + DL_CA_W, 8, 0, 0, 8, w, lane);
      vd_each(acc, w, lane, [&](int r, int c, float v) { A[r * VD_LD + c] = (v + L[DL_CA_B + c]) * 0.125f; });
    }
    __syncthreads();
    if (SAVE) vd_store_tile(a.qc + off, A, tid);
    __syncthreads();   // (vd_cross replaces the query in A with the attention output, under another thread-to-element map)
    vd_cross(A, nullptr, nullptr, nullptr, nullptr, a.mkv + ((long long)lp * 2 * a.bs + sb) * 16 * 256, a.n_chunks, tid);
    __syncthreads();
    {
      f32x4 acc[1][2];
      ve_zero(acc);
      vd_mm(acc, atA, L + DL_CO_W, 8, 0, 0, 8, w, lane);
      vd_each(acc, w, lane, [&](int r, int c, float v) { X[r * VD_LD + c] += v + L[DL_CO_B + c]; });
    }
    __syncthreads();
    if (SAVE) vd_store_tile(a.x2 + off, X, tid);
    ve_ln_stats(X, mean, rstd, 16, tid);
    __syncthreads();
    {   // FFN in 128-column chunks of the hidden
      f32x4 af[1][2];
      ve_zero(af);
      const VdTileLn an{X, mean, rstd, L + DL_LN3G, L + DL_LN3B, l15, q4};
      for (int ch = 0; ch < VE_FF / VE_D; ++ch) {
        f32x4 ah[1][2];
        ve_zero(ah);
        vd_mm(ah, an, L + DL_W1, 8, 8 * ch, 0, 8, w, lane);
        vd_each(ah, w, lane, [&](int r, int c, float v) { Hb[r * VD_LD + c] = ve_gelu(v + L[DL_B1 + VE_D * ch + c]); });
        __syncthreads();
        const VdTile ahb{Hb, VD_LD, 8 * ch, l15, q4};
        vd_mm(af, ahb, L + DL_W2, VE_FF / 16, 0, 8 * ch, 8 * ch + 8, w, lane);
        __syncthreads();
      }
      vd_each(af, w, lane, [&](int r, int c, float v) { X[r * VD_LD + c] += v + L[DL_B2 + c]; });
    }
    __syncthreads();
    if (l > a.nb && l < a.nl) {   // x = linear_blocks[j](cat(x, xs.pop())): the skip is the output of input block nb - 1 - j = layer nb - j's input
      const int j = l - a.nb - 1;
      const float* Wl = W + (long long)a.nl * DL_SIZE + (long long)j * DLIN_SIZE;
      vd_load_tile(A, a.x0 + ((long long)(a.nb - j) * a.rows + row0) * VE_D, tid);
      __syncthreads();
      f32x4 acc[1][2];
      ve_zero(acc);
      const VdTileCat ac{X, A, l15, q4};
      vd_mm(acc, ac, Wl + DLIN_W, 16, 0, 0, 16, w, lane);
      __syncthreads();
      vd_each(acc, w, lane, [&](int r, int c, float v) { X[r * VD_LD + c] = v + Wl[DLIN_B + c]; });
      __syncthreads();
    }
  }
  if (SAVE || l < a.nl) vd_store_tile(a.x0 + ((long long)vd_xslot<SAVE>(l, a.nb) * a.rows + row0) * VE_D, X, tid);
  ve_ln_stats(X, mean, rstd, 16, tid);
  __syncthreads();
  if (l < a.nl) {   // LN1 and q | k | v of layer l
    const float* L = W + (long long)l * DL_SIZE;
    const VdTileLn an{X, mean, rstd, L + DL_LN1G, L + DL_LN1B, l15, q4};
    float* out = a.qkv + ((long long)vd_lslot<SAVE>(l) * a.rows + row0) * 3 * VE_D;
    for (int ch = 0; ch < 3; ++ch) {
      f32x4 acc[1][2];
      ve_zero(acc);
      vd_mm(acc, an, L + DL_SA_W, 8, 8 * ch, 0, 8, w, lane);
      const float scale = ch == 0 ? 0.125f : 1.0f;
      vd_each(acc, w, lane, [&](int r, int c, float v) { out[r * 3 * VE_D + VE_D * ch + c] = (v + L[DL_SA_B + VE_D * ch + c]) * scale; });
    }
  } else if (a.feats) {   // final norm, final_layer, zero beyond the length (vae.py:359-368)
    const float* T = W + a.stack_floats - DT_SIZE;
    const VdTileLn an{X, mean, rstd, T + DT_NG, T + DT_NB, l15, q4};
    f32x4 acc[1][2];
    ve_zero(acc);
    vd_mm(acc, an, T + DT_FW, 8, 0, 0, 8, w, lane);
    const int c0 = s ? VE_BODY : 0, nf = s ? VE_HANDS : VE_BODY;
    vd_each(acc, w, lane, [&](int r, int c, float v) {
      const int f = 16 * t + r;
      if (c < nf && f < a.nframes) a.feats[((long long)b * a.nframes + f) * VE_NFEATS + c0 + c] = f < len ? v + T[DT_FB + c] : 0.f;
    });
  }
}

// Self-attention core of layer l for the tile's 16 queries: thread = (head tid / 128, row (tid / 8) % 16, 8 of the head's 64 dimensions);
// two passes over the valid keys (maximum and sum, then the value sum).  SAVE = false: slot 0 of qkv / o, no log-sum-exp stored.
template <bool SAVE>
__global__ void __launch_bounds__(256) vd_self_fwd_kernel(const VaeDecArgs a, int l) {
  const int tid = threadIdx.x, h = tid >> 7, r = (tid >> 3) & 15, p = tid & 7, c0 = 64 * h + 8 * p;
  const int t = blockIdx.x, b = blockIdx.y, s = blockIdx.z;
  const int len = min(a.lengths[b], a.nframes);
  if (16 * t >= len) return;
  const long long seq0 = ((long long)s * a.bs + b) * a.fp, row = seq0 + 16 * t + r;
  const float* __restrict__ qkv = a.qkv + (long long)vd_lslot<SAVE>(l) * a.rows * 3 * VE_D;
  float qv[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) qv[j] = qkv[row * 3 * VE_D + c0 + j];
  float mx = -INFINITY, sum = 0.f;
#pragma unroll 4
  for (int k = 0; k < len; ++k) {   // (unrolled: the keys' loads of several iterations are in flight together)
    const float* kp = qkv + (seq0 + k) * 3 * VE_D + VE_D + c0;
    float d = 0.f;
#pragma unroll
    for (int j = 0; j < 8; ++j) d += qv[j] * kp[j];
    d = vd_sum8(d);
    const float m2 = fmaxf(mx, d);
    sum = sum * expf(mx - m2) + expf(d - m2);
    mx = m2;
  }
  const float lse = mx + logf(sum);
  float o[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) o[j] = 0.f;
#pragma unroll 4
  for (int k = 0; k < len; ++k) {   // (unrolled: the keys' loads of several iterations are in flight together)
    const float* kp = qkv + (seq0 + k) * 3 * VE_D + VE_D + c0;
    float d = 0.f;
#pragma unroll
    for (int j = 0; j < 8; ++j) d += qv[j] * kp[j];
    d = vd_sum8(d);
    const float pk = expf(d - lse);
#pragma unroll
    for (int j = 0; j < 8; ++j) o[j] += pk * kp[VE_D + j];
  }
  float* out = a.o + ((long long)vd_lslot<SAVE>(l) * a.rows + row) * VE_D + c0;
#pragma unroll
  for (int j = 0; j < 8; ++j) out[j] = o[j];
  if (SAVE && p == 0) a.lse[((long long)l * a.rows + row) * 2 + h] = lse;
}

// ---- reverse sweep ------------------------------------------------------------------------------------------------------------------------
// Launch l of the sweep's row-local part (see the head of the file).
__global__ void __launch_bounds__(256) vd_bwd_rows_kernel(const VaeDecArgs a, int l) {
  __shared__ float X[16 * VD_LD], Gb[16 * VD_LD], A[16 * VD_LD3], Hb[16 * VD_LD], Tb[16 * VD_LD], mean[16], rstd[16], ps[16 * 2 * 16], ds[16 * 2 * 16];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, l15 = lane & 15, q4 = lane >> 4;
  const int t = blockIdx.x, b = blockIdx.y, s = blockIdx.z;
  const int len = min(a.lengths[b], a.nframes);
  if (16 * t >= len) {   // a tile wholly beyond the length carries no gradient: the tap reads zeros
    float* gz = a.g + ((long long)l * a.rows + ((long long)s * a.bs + b) * a.fp + 16 * t) * VE_D;
    for (int idx = tid; idx < 16 * VE_D; idx += 256) gz[idx] = 0.f;
    return;
  }
  const float* W = a.w + s * a.stack_floats;
  const long long sb = (long long)s * a.bs + b, row0 = sb * a.fp + 16 * t;
  const VdTile atG{Gb, VD_LD, 0, l15, q4};
  if (l == a.nl - 1) {   // the head: d_feats . final_layer.weight, the final norm
    const float* T = W + a.stack_floats - DT_SIZE;
    const int c0 = s ? VE_BODY : 0, nf = s ? VE_HANDS : VE_BODY;
    for (int idx = tid; idx < 16 * VE_D; idx += 256) {
      const int r = idx >> 7, c = idx & 127, f = 16 * t + r;
      A[r * VD_LD + c] = (c < nf && f < len) ? a.d_feats[((long long)b * a.nframes + f) * VE_NFEATS + c0 + c] : 0.f;
    }
    vd_load_tile(X, a.x0 + ((long long)a.nl * a.rows + row0) * VE_D, tid);
    for (int idx = tid; idx < 16 * VE_D; idx += 256) Gb[(idx >> 7) * VD_LD + (idx & 127)] = 0.f;
    __syncthreads();
    f32x4 acc[1][2];
    ve_zero(acc);
    const VdTile at{A, VD_LD, 0, l15, q4};
    vd_mm(acc, at, T + DT_FWT, 8, 0, 0, 8, w, lane);
    vd_each(acc, w, lane, [&](int r, int c, float v) { Tb[r * VD_LD + c] = v; });
    ve_ln_stats(X, mean, rstd, 16, tid);
    __syncthreads();
    vd_ln_bwd(Gb, X, mean, rstd, T + DT_NG, Tb, nullptr, tid);
    __syncthreads();
  } else {   // layer l + 1 below its self-attention core: q | k | v projection, LN1, the skip linear in front of an output block
    const int lu = l + 1;
    const float* L = W + (long long)lu * DL_SIZE;
    for (int idx = tid; idx < 16 * 96; idx += 256) {
      const int r = idx / 96, c = (idx % 96) * 4;
      *reinterpret_cast<f32x4*>(A + r * VD_LD3 + c) = *reinterpret_cast<const f32x4*>(a.dqkv + (row0 + r) * 3 * VE_D + c);
    }
    vd_load_tile(X, a.x0 + ((long long)lu * a.rows + row0) * VE_D, tid);
    __syncthreads();
    f32x4 acc[1][2];
    ve_zero(acc);
    const VdTile at{A, VD_LD3, 0, l15, q4};
    vd_mm(acc, at, L + DL_SA_WT, 24, 0, 0, 24, w, lane);
    vd_each(acc, w, lane, [&](int r, int c, float v) { Tb[r * VD_LD + c] = v; });
    ve_ln_stats(X, mean, rstd, 16, tid);
    __syncthreads();
    vd_ln_bwd(Gb, X, mean, rstd, L + DL_LN1G, Tb, a.g1 + row0 * VE_D, tid);
    __syncthreads();
    if (lu > a.nb) {   // d cat([x, skip]) = g . linear_blocks[j].weight: the first half goes on, the second is the skip tensor's gradient
      const int j = lu - a.nb - 1;
      const float* Wl = W + (long long)a.nl * DL_SIZE + (long long)j * DLIN_SIZE;
      f32x4 a0[1][2], a1[1][2];
      ve_zero(a0);
      ve_zero(a1);
      vd_mm(a0, atG, Wl + DLIN_WT, 8, 0, 0, 8, w, lane);
      vd_mm(a1, atG, Wl + DLIN_WT, 8, 8, 0, 8, w, lane);
      __syncthreads();
      float* gs = a.gskip + ((long long)(a.nb - 1 - j) * a.rows + row0) * VE_D;
      vd_each(a0, w, lane, [&](int r, int c, float v) { Gb[r * VD_LD + c] = v; });
      vd_each(a1, w, lane, [&](int r, int c, float v) { gs[r * VE_D + c] = v; });
      __syncthreads();
    }
  }
  if (l < a.nb) {   // layer l's output is also a skip tensor
    const float* gs = a.gskip + ((long long)l * a.rows + row0) * VE_D;
    for (int idx = tid; idx < 16 * VE_D; idx += 256) Gb[(idx >> 7) * VD_LD + (idx & 127)] += gs[idx];
    __syncthreads();
  }
  const float* L = W + (long long)l * DL_SIZE;
  const long long off = ((long long)l * a.rows + row0) * VE_D;
  vd_store_tile(a.g + off, Gb, tid);
  // FFN: the pre-activation recomputed chunk by chunk
  vd_load_tile(X, a.x2 + off, tid);
  __syncthreads();
  ve_ln_stats(X, mean, rstd, 16, tid);
  __syncthreads();
  {
    f32x4 af[1][2];
    ve_zero(af);
    const VdTileLn an{X, mean, rstd, L + DL_LN3G, L + DL_LN3B, l15, q4};
    for (int ch = 0; ch < VE_FF / VE_D; ++ch) {
      f32x4 ah[1][2], dh[1][2];
      ve_zero(ah);
      ve_zero(dh);
      vd_mm(ah, an, L + DL_W1, 8, 8 * ch, 0, 8, w, lane);
      vd_mm(dh, atG, L + DL_W2T, 8, 8 * ch, 0, 8, w, lane);
#pragma unroll
      for (int c = 0; c < 2; ++c) {
        const int col = 16 * (2 * w + c) + l15;
        const float bias = L[DL_B1 + VE_D * ch + col];
#pragma unroll
        for (int i = 0; i < 4; ++i) Hb[(4 * q4 + i) * VD_LD + col] = dh[0][c][i] * vd_gelu_grad(ah[0][c][i] + bias);
      }
      __syncthreads();
      const VdTile ahb{Hb, VD_LD, 8 * ch, l15, q4};
      vd_mm(af, ahb, L + DL_W1T, VE_FF / 16, 0, 8 * ch, 8 * ch + 8, w, lane);
      __syncthreads();
    }
    vd_each(af, w, lane, [&](int r, int c, float v) { Tb[r * VD_LD + c] = v; });
  }
  __syncthreads();
  vd_ln_bwd(Gb, X, mean, rstd, L + DL_LN3G, Tb, nullptr, tid);
  __syncthreads();
  // cross-attention
  {
    f32x4 acc[1][2];
    ve_zero(acc);
    vd_mm(acc, atG, L + DL_CO_WT, 8, 0, 0, 8, w, lane);
    vd_each(acc, w, lane, [&](int r, int c, float v) { Tb[r * VD_LD + c] = v; });   // dO of the cross-attention
  }
  vd_load_tile(A, a.qc + off, tid);   // (row stride VD_LD inside the wider buffer)
  vd_load_tile(X, a.x1 + off, tid);
  __syncthreads();
  vd_cross(A, Tb, Hb, ps, ds, a.mkv + ((long long)l * 2 * a.bs + sb) * 16 * 256, a.n_chunks, tid);
  ve_ln_stats(X, mean, rstd, 16, tid);
  __syncthreads();
  {   // the tile's partial dK | dV of the memory: thread = (K or V, column), the 16 rows summed in order
    const int kv = tid >> 7, c = tid & 127, h = c >> 6;
    const float* wgt = kv ? ps : ds;
    const float* val = kv ? Tb : A;
    float* out = a.pkv + ((((long long)l * 2 * a.bs + sb) * a.nt + t) * 16) * 256 + 128 * kv + c;
    for (int k = 0; k < 16; ++k) {
      float acc = 0.f;
      for (int r = 0; r < 16; ++r) acc += wgt[(r * 2 + h) * 16 + k] * val[r * VD_LD + c];
      out[k * 256] = acc;
    }
  }
  __syncthreads();
  {
    f32x4 acc[1][2];
    ve_zero(acc);
    const VdTile at{Hb, VD_LD, 0, l15, q4};
    vd_mm(acc, at, L + DL_CA_WT, 24, 0, 0, 8, w, lane);
    vd_each(acc, w, lane, [&](int r, int c, float v) { Tb[r * VD_LD + c] = v; });
  }
  __syncthreads();
  vd_ln_bwd(Gb, X, mean, rstd, L + DL_LN2G, Tb, nullptr, tid);
  __syncthreads();
  if (l == 0) return;   // layer 0's self-attention sees constants only
  // the self-attention's out-projection: dO, D = dO . O per head, the stream's gradient for the next launch
  {
    f32x4 acc[1][2];
    ve_zero(acc);
    vd_mm(acc, atG, L + DL_SO_WT, 8, 0, 0, 8, w, lane);
    vd_each(acc, w, lane, [&](int r, int c, float v) { Tb[r * VD_LD + c] = v; });
  }
  vd_store_tile(a.g1 + row0 * VE_D, Gb, tid);
  __syncthreads();
  vd_store_tile(a.d_o + row0 * VE_D, Tb, tid);
  {
    const int r = tid >> 4, h = (tid >> 3) & 1, p = tid & 7, c0 = 64 * h + 8 * p;
    const float* op = a.o + off + r * VE_D + c0;
    float d = 0.f;
#pragma unroll
    for (int j = 0; j < 8; ++j) d += Tb[r * VD_LD + c0 + j] * op[j];
    d = vd_sum8(d);
    if (p == 0) a.dd[(row0 + r) * 2 + h] = d;
  }
}

// Self-attention core of layer l backwards: dq of the tile's rows as queries, then dk | dv of the tile's rows as keys.  Thread as in
// vd_self_fwd_kernel; both loops run over the sequence's valid rows in order.
__global__ void __launch_bounds__(256) vd_self_bwd_kernel(const VaeDecArgs a, int l) {
  const int tid = threadIdx.x, h = tid >> 7, r = (tid >> 3) & 15, p = tid & 7, c0 = 64 * h + 8 * p;
  const int t = blockIdx.x, b = blockIdx.y, s = blockIdx.z;
  const int len = min(a.lengths[b], a.nframes);
  if (16 * t >= len) return;
  const long long seq0 = ((long long)s * a.bs + b) * a.fp, row = seq0 + 16 * t + r;
  const float* __restrict__ qkv = a.qkv + (long long)l * a.rows * 3 * VE_D;
  const float* __restrict__ lse = a.lse + (long long)l * a.rows * 2;
  float* out = a.dqkv + row * 3 * VE_D + c0;
  {
    float qv[8], dov[8], g[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      qv[j] = qkv[row * 3 * VE_D + c0 + j];
      dov[j] = a.d_o[row * VE_D + c0 + j];
      g[j] = 0.f;
    }
    const float ls = lse[row * 2 + h], dsum = a.dd[row * 2 + h];
#pragma unroll 4
    for (int k = 0; k < len; ++k) {
      const float* kp = qkv + (seq0 + k) * 3 * VE_D + VE_D + c0;
      float d = 0.f, e = 0.f;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        d += qv[j] * kp[j];
        e += dov[j] * kp[VE_D + j];
      }
      d = vd_sum8(d);
      e = vd_sum8(e);
      const float dsk = expf(d - ls) * (e - dsum);
#pragma unroll
      for (int j = 0; j < 8; ++j) g[j] += dsk * kp[j];
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) out[j] = 0.125f * g[j];
  }
  float gk[8], gv[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) gk[j] = gv[j] = 0.f;
  if (16 * t + r < len) {
    float kv[8], vv[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      kv[j] = qkv[row * 3 * VE_D + VE_D + c0 + j];
      vv[j] = qkv[row * 3 * VE_D + 2 * VE_D + c0 + j];
    }
#pragma unroll 4
    for (int i = 0; i < len; ++i) {
      const float* qp = qkv + (seq0 + i) * 3 * VE_D + c0;
      const float* dp = a.d_o + (seq0 + i) * VE_D + c0;
      float d = 0.f, e = 0.f;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        d += qp[j] * kv[j];
        e += dp[j] * vv[j];
      }
      d = vd_sum8(d);
      e = vd_sum8(e);
      const float pk = expf(d - lse[(seq0 + i) * 2 + h]);
      const float dsk = pk * (e - a.dd[(seq0 + i) * 2 + h]);
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        gk[j] += dsk * qp[j];
        gv[j] += pk * dp[j];
      }
    }
  }
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    out[VE_D + j] = gk[j];
    out[2 * VE_D + j] = gv[j];
  }
}

// Layer blockIdx.z's contribution to d_z of sequence blockIdx.x, stack blockIdx.y: the partial dK | dV summed over the sequence's tiles in
// order, times W_k | W_v (k-steps 8 .. 23 of the transposed in-projection).
__global__ void __launch_bounds__(256) vd_dz_kernel(const VaeDecArgs a) {
  __shared__ float A[16 * (256 + 4)];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, l15 = lane & 15, q4 = lane >> 4;
  const int b = blockIdx.x, s = blockIdx.y, l = blockIdx.z;
  const int ntl = (min(a.lengths[b], a.nframes) + 15) / 16;
  const float* W = a.w + s * a.stack_floats;
  const long long sb = (long long)s * a.bs + b;
  const float* pk = a.pkv + (((long long)l * 2 * a.bs + sb) * a.nt) * 16 * 256;
  for (int idx = tid; idx < 16 * 256; idx += 256) {
    float v = 0.f;
#pragma unroll 4
    for (int t = 0; t < ntl; ++t) v += pk[(long long)t * 16 * 256 + idx];
    A[(idx >> 8) * 260 + (idx & 255)] = v;
  }
  __syncthreads();
  f32x4 acc[1][2];
  ve_zero(acc);
  const VdTile at{A, 260, 8, l15, q4};
  vd_mm(acc, at, W + (long long)l * DL_SIZE + DL_CA_WT, 24, 0, 8, 24, w, lane);
  float* out = a.dzl + (((long long)l * 2 * a.bs) + sb) * 16 * VE_D;
  vd_each(acc, w, lane, [&](int r, int c, float v) { out[r * VE_D + c] = v; });
}

// d_z = the layers' contributions summed in order
__global__ void __launch_bounds__(256) vd_dz_sum_kernel(const VaeDecArgs a) {
  const long long sb = (long long)blockIdx.y * a.bs + blockIdx.x;
  for (int idx = threadIdx.x; idx < a.n_chunks * VE_D; idx += 256) {
    float v = 0.f;
    for (int l = 0; l < a.nl; ++l) v += a.dzl[(((long long)l * 2 * a.bs) + sb) * 16 * VE_D + idx];
    a.d_z[sb * a.n_chunks * VE_D + idx] = v;
  }
}
