// Motion evaluation (cfd_motion_eval / cfd_motion_diversity, cfd_metrics.hip): what the reference's quant_eval/ scripts compute on the
// host, one motion at a time, from the tensor ConvoFusionVae.decode returns.
//   stage A   me_stage_a_kernel   one workgroup per sequence, the sequence [T][189] staged in LDS: the L1div partial (metric_eval.py:342-356),
//                                 the SRGR partial and count (:317-339), the jitter sum (jitter_metric.py), the motion beats of joints
//                                 5 6 7 9 10 11 (:124-165, scipy's argrelextrema(np.less, order, mode="clip")), the beat alignment against the
//                                 caller's onset times (:262-293) and process_motion (:376-421)
//   stage B   me_gemm_kernel      HalfEmbeddingNet's pose encoder (motion_autoencoder.py:39-78) on the processed motion: four convolutions as
//                                 products over frame-major rows whose A rows overlap (row stride C or 2 C, K = 3 C or 4 C), then out_net and
//                                 fc_mu folded into one affine map at load (their LeakyReLU(True) has slope 1.0); v_mfma_f32_32x32x2_f32, exact
//                                 float32, every edge (M, N, K) masked at the tile fill
//   stage C   me_stats_kernel     n, sum e, sum e e^T of the embeddings in float64, added to the caller's state in one fixed order
//             me_div_*            the mean pairwise Euclidean distance (:303-314) from differences, accumulated in float64
// Reductions run in float64 in one fixed order (no atomics), so a sequence's outputs are the same bits on every call and in every batch.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#define ME_FEAT 189
#define ME_JOINTS 63
#define ME_T_MIN 24
#define ME_T_MAX 128
#define ME_THREADS 256
#define ME_TRACKS 6
#define ME_EMB_FRAMES 128   // the embedding net's Linear(59 F, ...) fixes the sequence length
#define ME_BK 32            // k tile of the products
#define ME_CHUNK_TILES 8    // k tiles per accumulation chunk (256 k)
#define ME_LDK 33           // floats per LDS tile row (32 + 1: a wave's 32 rows fall on 32 banks)
#define ME_DIV_TILE 16
#define ME_DIV_KC 64
#define ME_DIV_MAX_N 8192

typedef __attribute__((ext_vector_type(16))) float me_f32x16;

// The folded pack of the embedding net, floats: per convolution W [N][K] then b [N] (K = kernel x C_in, index kk * C_in + c), then the
// folded affine map W [F][59 F] (column t * F + c) and b [F]
__host__ __device__ inline size_t me_pack_floats(int F) {
  const size_t f = (size_t)F;
  return f * (3 * ME_FEAT) + f + 2 * f * (3 * f) + 2 * f + 2 * f * (8 * f) + 2 * f + f * (6 * f) + f + f * (59 * f) + f;
}
// per sequence, floats of the four activations [126][F] [124][2F] [61][2F] [59][F]
__host__ __device__ inline size_t me_act_floats(int F) { return (size_t)F * (126 + 2 * 124 + 2 * 61 + 59); }

struct MeStageAArgs {
  const float* pred;        // [B][T] rows of `stride` floats
  const float* target;      // same layout, or null
  const float* semantic;    // [B][T] or null
  long long stride;
  int T, order, n_onsets;
  double fps, sigma, threshold;
  const int32_t* onset_off; // [B + 1] or null
  const double* onset_t;    // [n_onsets]
  double *l1div, *srgr, *jitter, *align;   // [B] each, or null
  int32_t* srgr_count;      // [B] or null
  uint8_t* beats;           // [B][6][T - 1] or null
  float* processed;         // [B][T][189] or null
};

// the sum of one value per thread, in one fixed order (ascending pairs); every thread gets it
__device__ __forceinline__ double me_block_sum(double v, double* red) {
  const int tid = threadIdx.x;
  red[tid] = v;
  __syncthreads();
  for (int s = ME_THREADS / 2; s > 0; s >>= 1) {
    if (tid < s) red[tid] += red[tid + s];
    __syncthreads();
  }
  const double r = red[0];
  __syncthreads();
  return r;
}

__device__ __forceinline__ void me_cross(const double a[3], const double b[3], double o[3]) {
  o[0] = a[1] * b[2] - a[2] * b[1];
  o[1] = a[2] * b[0] - a[0] * b[2];
  o[2] = a[0] * b[1] - a[1] * b[0];
}

// joint j of frame t on the floor, its XZ at the first frame's root, turned by q (w, x, y, z): qrot's v + 2 (w (u x v) + u x (u x v))
__device__ __forceinline__ void me_placed(const float* x, int t, int j, double floor_y, double rx, double rz, const double q[4], double o[3]) {
  const float* p = x + t * ME_FEAT + 3 * j;
  const double v[3] = {(double)p[0] - rx, (double)p[1] - floor_y, (double)p[2] - rz};
  double uv[3], uuv[3];
  me_cross(q + 1, v, uv);
  me_cross(q + 1, uv, uuv);
#pragma unroll
  for (int c = 0; c < 3; ++c) o[c] = v[c] + 2.0 * (q[0] * uv[c] + uuv[c]);
}

__global__ void __launch_bounds__(ME_THREADS) me_stage_a_kernel(const MeStageAArgs a) {
  extern __shared__ float x[];                       // the sequence, [T][189]
  __shared__ double red[ME_THREADS];
  __shared__ double vel[ME_TRACKS * (ME_T_MAX - 1)];
  __shared__ int redi[ME_THREADS];
  __shared__ uint8_t wrist[ME_T_MAX];
  const int tid = threadIdx.x, T = a.T, nv = T - 1;
  const long long b = blockIdx.x;
  const float* src = a.pred + b * T * a.stride;
  for (int e = tid; e < T * ME_FEAT; e += ME_THREADS) {
    const int t = e / ME_FEAT, f = e - t * ME_FEAT;
    x[e] = src[t * a.stride + f];
  }
  __syncthreads();

  if (a.l1div) {       // sum over frames and features of |x - the sequence's mean of the feature|
    double part = 0.0;
    if (tid < ME_FEAT) {
      double s = 0.0;
      for (int t = 0; t < T; ++t) s += (double)x[t * ME_FEAT + tid];
      const double mean = s / (double)T;
      for (int t = 0; t < T; ++t) part += fabs((double)x[t * ME_FEAT + tid] - mean);
    }
    const double l1 = me_block_sum(part, red);
    if (tid == 0) a.l1div[b] = l1;
  }

  if (a.target) {
    const float* tg = a.target + b * T * a.stride;
    if (a.srgr || a.srgr_count) {
      const float* sem = a.semantic + b * T;
      double ws = 0.0;
      int cnt = 0;
      for (int e = tid; e < T * ME_JOINTS; e += ME_THREADS) {
        const int t = e / ME_JOINTS, j = e - t * ME_JOINTS;
        const float* p = x + t * ME_FEAT + 3 * j;
        const float* q = tg + t * a.stride + 3 * j;
        const double d = fabs((double)p[0] - (double)q[0]) + fabs((double)p[1] - (double)q[1]) + fabs((double)p[2] - (double)q[2]);
        if (d < a.threshold) {
          ++cnt;
          ws += (double)sem[t] * (1.0 / 0.165);
        }
      }
      const double tot = me_block_sum(ws, red);
      redi[tid] = cnt;
      __syncthreads();
      for (int s = ME_THREADS / 2; s > 0; s >>= 1) {
        if (tid < s) redi[tid] += redi[tid + s];
        __syncthreads();
      }
      if (tid == 0) {
        if (a.srgr) a.srgr[b] = tot;
        if (a.srgr_count) a.srgr_count[b] = redi[0];
      }
      __syncthreads();
    }
    if (a.jitter) {
      double acc = 0.0;
      for (int e = tid; e < nv * ME_FEAT; e += ME_THREADS) {
        const int t = e / ME_FEAT, f = e - t * ME_FEAT;
        const double dp = fabs((double)x[(t + 1) * ME_FEAT + f] - (double)x[t * ME_FEAT + f]);
        const double dt = fabs((double)tg[(t + 1) * a.stride + f] - (double)tg[t * a.stride + f]);
        acc += fabs(dp - dt);
      }
      const double tot = me_block_sum(acc, red);
      if (tid == 0) a.jitter[b] = tot;
    }
  }

  if (a.beats || a.align) {
    for (int e = tid; e < ME_TRACKS * nv; e += ME_THREADS) {
      const int k = e / nv, i = e - k * nv;
      const int j = k < 3 ? 5 + k : 6 + k;           // joints 5 6 7 9 10 11
      double s = 0.0;
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const double d = (double)x[(i + 1) * ME_FEAT + 3 * j + c] - (double)x[i * ME_FEAT + 3 * j + c];
        s += d * d;
      }
      vel[k * (ME_T_MAX - 1) + i] = sqrt(s);
    }
    __syncthreads();
    for (int e = tid; e < ME_TRACKS * nv; e += ME_THREADS) {
      const int k = e / nv, i = e - k * nv;
      const double* v = vel + k * (ME_T_MAX - 1);
      const double vi = v[i];
      bool beat = true;
      for (int s = 1; s <= a.order; ++s) {           // strictly below both clipped neighbours at every distance
        const int lo = i - s < 0 ? 0 : i - s, hi = i + s > nv - 1 ? nv - 1 : i + s;
        beat = beat && vi < v[lo] && vi < v[hi];
      }
      if (a.beats) a.beats[(b * ME_TRACKS + k) * nv + i] = beat ? 1 : 0;
      if (k == ME_TRACKS - 1) wrist[i] = beat ? 1 : 0;
    }
    __syncthreads();
    if (a.align) {      // mean over the sequence's onsets of exp(-d^2 / 2 sigma^2), d to the nearest right-wrist beat (none: 0)
      int lo = a.onset_off[b], hi = a.onset_off[b + 1];
      lo = lo < 0 ? 0 : lo > a.n_onsets ? a.n_onsets : lo;
      hi = hi < lo ? lo : hi > a.n_onsets ? a.n_onsets : hi;
      double acc = 0.0;
      for (int o = lo + tid; o < hi; o += ME_THREADS) {
        const double ot = a.onset_t[o];
        double dmin = INFINITY;
        for (int i = 0; i < nv; ++i)
          if (wrist[i]) dmin = fmin(dmin, fabs((double)i / a.fps - ot));
        if (dmin < INFINITY) acc += exp(-(dmin * dmin) / (2.0 * a.sigma * a.sigma));
      }
      const double tot = me_block_sum(acc, red);
      if (tid == 0) a.align[b] = hi > lo ? tot / (double)(hi - lo) : 0.0;
    }
  }

  if (a.processed) {
    double m = INFINITY;
    for (int e = tid; e < T * ME_JOINTS; e += ME_THREADS) m = fmin(m, (double)x[3 * e + 1]);
    red[tid] = m;
    __syncthreads();
    for (int s = ME_THREADS / 2; s > 0; s >>= 1) {
      if (tid < s) red[tid] = fmin(red[tid], red[tid + s]);
      __syncthreads();
    }
    const double floor_y = red[0];
    const double rx = (double)x[0], rz = (double)x[2];
    // facing: across the hips (18 - 13) and shoulders (9 - 5) of frame 0, forward = y x across, q turns forward onto +z
    double ac[3], q[4];
#pragma unroll
    for (int c = 0; c < 3; ++c)
      ac[c] = ((double)x[3 * 18 + c] - (double)x[3 * 13 + c]) + ((double)x[3 * 9 + c] - (double)x[3 * 5 + c]);
    const double an = sqrt(ac[0] * ac[0] + ac[1] * ac[1] + ac[2] * ac[2]);
    double fw[3] = {ac[2] / an, 0.0, -(ac[0] / an)};
    const double fn = sqrt(fw[0] * fw[0] + fw[1] * fw[1] + fw[2] * fw[2]);
#pragma unroll
    for (int c = 0; c < 3; ++c) fw[c] /= fn;
    const double tz[3] = {0.0, 0.0, 1.0};
    me_cross(fw, tz, q + 1);
    q[0] = sqrt(fw[0] * fw[0] + fw[1] * fw[1] + fw[2] * fw[2]) + fw[2];
    const double qn = sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
#pragma unroll
    for (int c = 0; c < 4; ++c) q[c] /= qn;
    float* dst = a.processed + b * T * ME_FEAT;
    for (int e = tid; e < T * ME_JOINTS; e += ME_THREADS) {
      const int t = e / ME_JOINTS, j = e - t * ME_JOINTS;
      double r[3], root[3], w[3];
      me_placed(x, t, j, floor_y, rx, rz, q, r);
      if (j >= 1) {                                 // root-relative joints, wrist-relative hands (7: joints 23..42, 11: joints 43..62)
        me_placed(x, t, 0, floor_y, rx, rz, q, root);
#pragma unroll
        for (int c = 0; c < 3; ++c) r[c] -= root[c];
        if (j >= 23) {
          me_placed(x, t, j < 43 ? 7 : 11, floor_y, rx, rz, q, w);
#pragma unroll
          for (int c = 0; c < 3; ++c) r[c] -= w[c] - root[c];
        }
      }
#pragma unroll
      for (int c = 0; c < 3; ++c) dst[e * 3 + c] = (float)r[c];
    }
  }
}

// Y(z; m, n) = leaky(sum_k A(z; m, k) W[n][k] + bias[n]): row m of batch entry z is the K contiguous floats at A + z a_batch + m a_row, so
// a_row < K makes the rows overlap -- a k = 3 convolution over frame-major rows of C floats is a_row = C, K = 3 C; stride 2, k = 4 is
// a_row = 2 C, K = 4 C.  A workgroup of 4 waves (2 x 2) owns a 64 x 64 block, a wave one 32 x 32 MFMA tile.  Tiles of 32 k go through LDS by
// single floats (the rows are not 16-byte aligned: C = 189), zero outside M, N and K, so no shape needs padding.  Two-level summation as in
// t5_enc.hpp: the chain of a 256-deep chunk, then the sum of the chunks.  grid (ceil(N / 64), ceil(M / 64), batch).
struct MeGemmArgs {
  const float* A;
  long long a_row, a_batch;
  const float* W;          // [N][K]
  const float* bias;       // [N]
  float* Y;
  long long y_row, y_batch;
  int M, N, K;
  float slope;             // LeakyReLU's negative slope (1: none)
};

__global__ void __launch_bounds__(256) me_gemm_kernel(const MeGemmArgs a) {
  __shared__ float As[64 * ME_LDK];
  __shared__ float Ws[64 * ME_LDK];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1, half = lane >> 5, li = lane & 31;
  const int m0 = blockIdx.y * 64, n0 = blockIdx.x * 64;
  const float* A = a.A + (long long)blockIdx.z * a.a_batch;
  const int kk = tid & 31, r0 = tid >> 5;            // the thread fills column kk of rows r0, r0 + 8, ...
  me_f32x16 acc, tot;
#pragma unroll
  for (int e = 0; e < 16; ++e) acc[e] = tot[e] = 0.f;
  for (int k0 = 0; k0 < a.K; k0 += ME_BK) {
    const bool k_ok = k0 + kk < a.K;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const int r = r0 + 8 * i;
      As[r * ME_LDK + kk] = (k_ok && m0 + r < a.M) ? A[(long long)(m0 + r) * a.a_row + k0 + kk] : 0.f;
      Ws[r * ME_LDK + kk] = (k_ok && n0 + r < a.N) ? a.W[(long long)(n0 + r) * a.K + k0 + kk] : 0.f;
    }
    __syncthreads();
#pragma unroll
    for (int s = 0; s < ME_BK; s += 2)
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(As[(wm * 32 + li) * ME_LDK + s + half], Ws[(wn * 32 + li) * ME_LDK + s + half], acc, 0, 0, 0);
    if ((k0 / ME_BK) % ME_CHUNK_TILES == ME_CHUNK_TILES - 1 || k0 + ME_BK >= a.K) {
      tot += acc;
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[e] = 0.f;
    }
    __syncthreads();
  }
  // C / D of the 32 x 32 MFMA: column lane % 32, row (reg % 4) + 8 (reg / 4) + 4 (lane / 32)
  const int n = n0 + wn * 32 + li;
  if (n >= a.N) return;
  const float bn = a.bias[n];
  float* Y = a.Y + (long long)blockIdx.z * a.y_batch;
#pragma unroll
  for (int e = 0; e < 16; ++e) {
    const int m = m0 + wm * 32 + (e & 3) + 8 * (e >> 2) + 4 * half;
    if (m >= a.M) continue;
    float v = tot[e] + bn;
    v = v >= 0.f ? v : v * a.slope;
    Y[(long long)m * a.y_row + n] = v;
  }
}

// state = [n | sum e [F] | sum e e^T [F][F]] in float64, += this batch's embeddings e [B][F]: one thread per entry, the batch in groups of
// 32 sequences (a group in ascending order, then the groups in ascending order)
__global__ void __launch_bounds__(256) me_stats_kernel(const float* __restrict__ e, int B, int F, double* __restrict__ state) {
  const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= 1 + (long long)F + (long long)F * F) return;
  if (idx == 0) {
    state[0] += (double)B;
    return;
  }
  const bool first = idx <= F;
  const int i = first ? (int)(idx - 1) : (int)((idx - 1 - F) / F), j = first ? -1 : (int)((idx - 1 - F) % F);
  double total = 0.0;
  for (int g = 0; g < B; g += 32) {
    double s = 0.0;
    const int end = g + 32 < B ? g + 32 : B;
    for (int b = g; b < end; ++b) {
      const double ei = (double)e[(long long)b * F + i];
      s += first ? ei : ei * (double)e[(long long)b * F + j];
    }
    total += s;
  }
  state[idx] += total;
}

// Pairwise distances of the rows of X [N][D]: workgroup (bi, bj), bj >= bi, owns the 16 x 16 pairs of row blocks bi and bj, thread (ti, tj)
// the pair (16 bi + ti, 16 bj + tj); sum_k (x_i[k] - x_j[k])^2 from the differences, in float64 (a Gram-matrix form cancels when two
// motions are nearly equal).  The block's sum over its pairs i < j goes to partial[bi * nt + bj]; blocks below the diagonal write 0.
__global__ void __launch_bounds__(256) me_div_tile_kernel(const float* __restrict__ X, int N, long long D, double* __restrict__ partial) {
  __shared__ float as[ME_DIV_TILE][ME_DIV_KC + 1];
  __shared__ float bs[ME_DIV_TILE][ME_DIV_KC + 1];
  __shared__ double red[ME_THREADS];
  const int tid = threadIdx.x, bi = blockIdx.y, bj = blockIdx.x, nt = gridDim.x;
  if (bj < bi) {
    if (tid == 0) partial[(long long)bi * nt + bj] = 0.0;
    return;
  }
  const int ti = tid >> 4, tj = tid & 15;
  const int i = bi * ME_DIV_TILE + ti, j = bj * ME_DIV_TILE + tj;
  double acc = 0.0;
  for (long long k0 = 0; k0 < D; k0 += ME_DIV_KC) {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int e = tid + 256 * q, r = e >> 6, kk = e & 63;
      const bool k_ok = k0 + kk < D;
      const int ra = bi * ME_DIV_TILE + r, rb = bj * ME_DIV_TILE + r;
      as[r][kk] = (k_ok && ra < N) ? X[(long long)ra * D + k0 + kk] : 0.f;
      bs[r][kk] = (k_ok && rb < N) ? X[(long long)rb * D + k0 + kk] : 0.f;
    }
    __syncthreads();
#pragma unroll 8
    for (int kk = 0; kk < ME_DIV_KC; ++kk) {
      const double d = (double)as[ti][kk] - (double)bs[tj][kk];
      acc += d * d;
    }
    __syncthreads();
  }
  const double dist = (i < j && j < N) ? sqrt(acc) : 0.0;
  const double tot = me_block_sum(dist, red);
  if (tid == 0) partial[(long long)bi * nt + bj] = tot;
}

// out[0] = (the sum of the count partials in one fixed order) / pairs
__global__ void __launch_bounds__(ME_THREADS) me_div_sum_kernel(const double* __restrict__ partial, long long count, double pairs, double* __restrict__ out) {
  __shared__ double red[ME_THREADS];
  double s = 0.0;
  for (long long e = threadIdx.x; e < count; e += ME_THREADS) s += partial[e];
  const double tot = me_block_sum(s, red);
  if (threadIdx.x == 0) out[0] = tot / pairs;
}
