// libcfdenoise: the backward pass of AudioConvEncoder (cfd_audio_encoder_vjp, cfd_audio.hip) -- Linear, LeakyReLU(0.1), Linear,
// LeakyReLU(0.1), Linear over a few thousand Mel rows.  Exact float32: every sum is one FMA chain in ascending order of its reduction
// index, owned by one thread, so the bits depend on the inputs and the row count alone -- not on what else the call asks for, not on
// the workspace, no atomics.
//   aeb_dgrad_kernel   out[r][n] = (sum_k g[r][k] W[k][n]) * leaky'(h[r][n])          dz2, dz1 and d_x (h null: no slope)
//   aeb_wgrad_kernel   dW[n][k] = sum_r g[r][n] a[r][k], db[n] = sum_r g[r][n]        all three layers in one launch, rows in segments
//   aeb_close_kernel   out[i] = sum_s plane[s][i], s ascending                          only where the rows were split
// The rows are the reduction dimension of the weight gradients: a 64 x 64 tile of one dW and one segment of rows belong to one
// workgroup, which stages the rows 32 at a time through LDS.  The segmentation is a function of n_rows alone (aeb_seg_rows).
#pragma once
#include <hip/hip_runtime.h>

constexpr int AEB_THREADS = 256;
constexpr int AEB_CHUNK = 32;          // rows per LDS stage
constexpr int AEB_TILE = 64;           // a weight-gradient tile is 64 outputs x 64 inputs
constexpr int AEB_SEG_ROWS = 512;      // the shortest segment
constexpr int AEB_MAX_SEGS = 16;
constexpr int AEB_MAX_WIDTH = 1024;

// Rows per segment: 512, or as many (a multiple of the 32-row chunk) as keep the segments at 16 or fewer
static inline long long aeb_seg_rows(long long n_rows) {
  const long long per = (n_rows + AEB_MAX_SEGS - 1) / AEB_MAX_SEGS;
  const long long r = (per + AEB_CHUNK - 1) / AEB_CHUNK * AEB_CHUNK;
  return r > AEB_SEG_ROWS ? r : AEB_SEG_ROWS;
}

// leaky'(z) from h = leaky(z): h and z have the same sign, and h == 0 (either zero) only where z is not positive
__device__ __forceinline__ float aeb_slope(float h) { return h > 0.f ? 1.f : 0.1f; }

// ------------------------------------------------------------------------------------------------
// out[r][n] = (sum_k g[r][k] W[k][n]) * leaky'(h[r][n]): the gradient at a layer's input from the gradient at its output, W as nn.Linear
// stores it ([K = out features][N = in features], row pitch N).  32 rows x 64 columns per block, k in chunks of 32, ascending.
// ------------------------------------------------------------------------------------------------
template <int = 0>
__global__ void __launch_bounds__(AEB_THREADS) aeb_dgrad_kernel(const float* __restrict__ g, long long n_rows, int K, const float* __restrict__ W, int N,
                                                                const float* __restrict__ h, float* __restrict__ out) {
  __shared__ float gs[32][33];
  __shared__ float ws[32][AEB_TILE];
  const int tid = threadIdx.x;
  const int tx = tid & 15, ty = tid >> 4;               // 4 output columns, 2 rows per thread
  const long long r0 = (long long)blockIdx.y * 32;
  const int n0 = blockIdx.x * AEB_TILE;
  float acc[2][4] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
  for (int k0 = 0; k0 < K; k0 += 32) {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int e = tid + 256 * q, rr = e >> 5, kk = e & 31;
      const long long r = r0 + rr;
      gs[rr][kk] = (r < n_rows && k0 + kk < K) ? g[r * K + k0 + kk] : 0.f;
    }
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      const int e = tid + 256 * q, kk = e >> 6, nn = e & 63;
      ws[kk][nn] = (k0 + kk < K && n0 + nn < N) ? W[(long long)(k0 + kk) * N + n0 + nn] : 0.f;
    }
    __syncthreads();
#pragma unroll
    for (int kk = 0; kk < 32; ++kk) {
      const float x0 = gs[ty * 2][kk], x1 = gs[ty * 2 + 1][kk];
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const float w = ws[kk][tx * 4 + c];
        acc[0][c] = fmaf(x0, w, acc[0][c]);
        acc[1][c] = fmaf(x1, w, acc[1][c]);
      }
    }
    __syncthreads();
  }
#pragma unroll
  for (int rr = 0; rr < 2; ++rr) {
    const long long r = r0 + ty * 2 + rr;
    if (r >= n_rows) continue;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const int n = n0 + tx * 4 + c;
      if (n >= N) continue;
      float v = acc[rr][c];
      if (h) v = v * aeb_slope(h[r * N + n]);
      out[r * N + n] = v;
    }
  }
}

// One layer's parameter gradients as the weight-gradient launch sees them: dW [N][K] = g^T a with g [rows][N] the gradient at the
// layer's output and a [rows][K] its input; db [N] the column sums of g.  w_dst / b_dst: the caller's outputs where the rows are one
// segment, else this layer's blocks in segment 0's plane (segment s writes seg_stride floats further on).  A null destination is not
// written; without w_dst only the tiles of k-tile 0 exist (they own the bias).
struct AebLayer {
  const float *g, *a;
  int N, K;
  float *w_dst, *b_dst;
  int nkt;        // k-tiles per n-tile in this launch: ceil(K / 64), or 1 where only the bias is wanted
  int ntiles;     // ceil(N / 64) * nkt, or 0: nothing of this layer is wanted
};
struct AebWgradArgs {
  AebLayer layer[3];
  long long n_rows, seg_rows, seg_stride;
};

// Workgroup (x, y): tile x of the wanted layers' tiles in layer order, segment y of the rows.  Thread (tn, tk) owns outputs
// n0 + 4 tn .. + 3 by inputs k0 + 4 tk .. + 3 and walks its segment's rows in ascending order; the threads of tk == 0 in a k-tile 0
// workgroup also own the bias sums of their four outputs, over the same rows in the same order.
template <int = 0>
__global__ void __launch_bounds__(AEB_THREADS) aeb_wgrad_kernel(const AebWgradArgs p) {
  __shared__ __attribute__((aligned(16))) float gs[AEB_CHUNK][AEB_TILE];
  __shared__ __attribute__((aligned(16))) float as[AEB_CHUNK][AEB_TILE];
  int idx = blockIdx.x, m = 0;
  while (m < 2 && idx >= p.layer[m].ntiles) { idx -= p.layer[m].ntiles; ++m; }
  const AebLayer& y = p.layer[m];
  if (idx >= y.ntiles) return;                          // (uniform: the grid is the sum of ntiles)
  const int n0 = (idx / y.nkt) * AEB_TILE, k0 = (idx % y.nkt) * AEB_TILE;
  const long long seg = blockIdx.y, row_lo = seg * p.seg_rows;
  const long long row_hi = row_lo + p.seg_rows < p.n_rows ? row_lo + p.seg_rows : p.n_rows;
  const int tid = threadIdx.x, tn = tid >> 4, tk = tid & 15;
  const int N = y.N, K = y.K;
  const bool bias = y.b_dst && k0 == 0 && tk == 0;
  float acc[4][4], bsum[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = 0.f;
  for (long long r0 = row_lo; r0 < row_hi; r0 += AEB_CHUNK) {
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      const int e = tid + AEB_THREADS * q, rr = e >> 6, cc = e & 63;
      const long long r = r0 + rr;
      const bool live = r < row_hi;
      gs[rr][cc] = (live && n0 + cc < N) ? y.g[r * N + n0 + cc] : 0.f;
      as[rr][cc] = (live && k0 + cc < K) ? y.a[r * K + k0 + cc] : 0.f;
    }
    __syncthreads();
#pragma unroll 8
    for (int rr = 0; rr < AEB_CHUNK; ++rr) {
      const float4 g4 = *reinterpret_cast<const float4*>(&gs[rr][tn * 4]);
      const float4 a4 = *reinterpret_cast<const float4*>(&as[rr][tk * 4]);
      const float gv[4] = {g4.x, g4.y, g4.z, g4.w}, av[4] = {a4.x, a4.y, a4.z, a4.w};
#pragma unroll
      for (int i = 0; i < 4; ++i) {
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = fmaf(gv[i], av[j], acc[i][j]);
        if (bias) bsum[i] = bsum[i] + gv[i];
      }
    }
    __syncthreads();
  }
  const long long so = seg * p.seg_stride;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int n = n0 + tn * 4 + i;
    if (n >= N) continue;
    if (y.w_dst) {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int k = k0 + tk * 4 + j;
        if (k < K) y.w_dst[so + (long long)n * K + k] = acc[i][j];
      }
    }
    if (bias) y.b_dst[so + n] = bsum[i];
  }
}

// The closing pass of a call whose rows were split: the plane of a segment holds the six blocks w0 b0 w1 b1 w2 b2 back to back (end[b]:
// one past block b's last float); every wanted block's element is the sum of the segments' in ascending segment order.
struct AebCloseArgs {
  const float* planes;
  long long stride;       // floats per plane
  int n_seg;
  long long end[6];
  float* dst[6];          // null: not wanted (and not written by the launch before)
};
template <int = 0>
__global__ void aeb_close_kernel(const AebCloseArgs p) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= p.end[5]) return;
  int b = 0;
  while (b < 5 && i >= p.end[b]) ++b;
  if (!p.dst[b]) return;
  float s = p.planes[i];
  for (int k = 1; k < p.n_seg; ++k) s = s + p.planes[(long long)k * p.stride + i];
  p.dst[b][i - (b ? p.end[b - 1] : 0)] = s;
}
