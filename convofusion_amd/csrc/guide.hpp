// cfd_denoise_guide: one guided update of the sampling loop's latents by a key-pose loss of the predicted clean latents, as a device
// call -- the guidance combine, x0, the loss and its cotangent rows (guide_seed_kernel), the reverse sweep of cfd_denoise_vjp from them
// (rt_grad.hpp, unchanged), the sum over the guidance chunks, the fold of tied tokens' gradients onto their sources and the update
// (guide_update_kernel).  Float32 throughout, no atomics: the same inputs give the same bits.
// Included by cfd_grad.hip after rt_grad.hpp.
#pragma once

#include "guide_tables.hpp"

// Row c * n_tok / L + b of the forward's input is x~[b]: x with every tied token replaced by its source's value (tie == null: x itself).
// One thread per float4; a tie entry outside [0, n_tok) counts as free, so no table makes the kernel read out of bounds.
template <int = 0>
__global__ void guide_replicate_kernel(const float* __restrict__ x, const int32_t* __restrict__ tie, float* __restrict__ xin, long long n_tok,
                                       long long total4) {
  const long long i = blockIdx.x * 256LL + threadIdx.x;
  if (i >= total4) return;
  const long long tok = (i >> 5) % n_tok;
  long long src = tok;
  if (tie) {
    const int v = tie[tok];
    if (v >= 0 && v < n_tok) src = v;
  }
  reinterpret_cast<float4*>(xin)[i] = reinterpret_cast<const float4*>(x)[src * (CFD_LAT / 4) + (i & 31)];
}

struct GuideSeedArgs {
  const float* xin;      // [n][n_tok][128]: x~, replicated (chunk 0 is read)
  const float* eps;      // [n][n_tok][128]: the forward's output, chunk-major
  const float* w;        // [B][n] chunk weights; w[b][0] is not read
  const float* target;   // [n_tok][128]
  const float* mask;     // [n_tok]
  float* d_out;          // [n][n_tok][128]: the cotangent rows
  float* g_dir;          // [n_tok][128]: d loss / d x~ not through the denoiser
  float* partial;        // [n_tok]: sum over the token's 128 elements of r^2
  long long n_tok;
  int n, L;
  float s0, s1, inv_n;   // sqrt(acp_t), sqrt(1 - acp_t), 1 / (kept tokens * 128)
};

// One workgroup of 128 threads per token, one element per thread:
//   eps = e_0 + sum_{k = 1 .. n-1} w_k (e_k - e_0), x0 = (x~ - s1 eps) / s0, r = mask (x0 - target), d_x0 = 2 inv_n r,
//   g_dir = d_x0 / s0, d_out_k = -(s1 / s0) w_k d_x0 (k >= 1), d_out_0 = -(s1 / s0) (1 - sum_k w_k) d_x0.
// The token's sum of r^2: two wave reductions and one addition, in a fixed order.
template <int = 0>
__global__ __launch_bounds__(128) void guide_seed_kernel(GuideSeedArgs a) {
  __shared__ float part[2];
  const long long tok = blockIdx.x;
  const int d = threadIdx.x;
  const long long e = tok * CFD_LAT + d, chunk = a.n_tok * CFD_LAT;
  const float* w = a.w + (tok / a.L) * a.n;
  const float e0 = a.eps[e];
  float eps = e0, sumw = 0.f;
  for (int k = 1; k < a.n; ++k) {
    const float wk = w[k];
    eps = eps + wk * (a.eps[k * chunk + e] - e0);
    sumw += wk;
  }
  const float x0 = (a.xin[e] - a.s1 * eps) / a.s0;
  const float r = a.mask[tok] * (x0 - a.target[e]);
  const float dx0 = 2.f * a.inv_n * r;
  const float back = -(a.s1 / a.s0);
  a.g_dir[e] = dx0 / a.s0;
  a.d_out[e] = back * (1.f - sumw) * dx0;
  for (int k = 1; k < a.n; ++k) a.d_out[k * chunk + e] = back * w[k] * dx0;
  float v = r * r;
  for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
  if ((d & 63) == 0) part[d >> 6] = v;
  __syncthreads();
  if (d == 0) a.partial[tok] = part[0] + part[1];
}

// loss = inv_n * sum of the per-token partials: one workgroup, thread t takes the tokens t, t + 256, ... in ascending order, then a
// fixed tree over the 256 threads.
template <int = 0>
__global__ __launch_bounds__(256) void guide_loss_kernel(const float* __restrict__ partial, long long n_tok, float inv_n, float* __restrict__ loss) {
  __shared__ float sh[256];
  float v = 0.f;
  for (long long i = threadIdx.x; i < n_tok; i += 256) v += partial[i];
  sh[threadIdx.x] = v;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) sh[threadIdx.x] += sh[threadIdx.x + s];
    __syncthreads();
  }
  if (threadIdx.x == 0) *loss = inv_n * sh[0];
}

struct GuideUpdateArgs {
  const float* xin;      // [n][n_tok][128]: chunk 0 = x~ (never the caller's x: x_new may alias that)
  const float* g_dir;    // [n_tok][128]
  const float* g_rows;   // [n][n_tok][128]: the sweep's gradient per forward row
  const int32_t* tie;    // [n_tok] or null
  const int32_t* csr;    // guide_tables.hpp, or null
  float* grad;           // [n_tok][128] or null
  float* x_new;          // [n_tok][128] or null
  long long n_tok;
  int n;
  float step;
};

// g~ of one token: the direct term, then the chunks' rows in ascending order
__device__ __forceinline__ float4 guide_chunk_sum(const GuideUpdateArgs& a, long long tok, int q) {
  float4 g = reinterpret_cast<const float4*>(a.g_dir)[tok * 32 + q];
  for (int c = 0; c < a.n; ++c) {
    const float4 r = reinterpret_cast<const float4*>(a.g_rows)[((long long)c * a.n_tok + tok) * 32 + q];
    g.x += r.x; g.y += r.y; g.z += r.z; g.w += r.w;
  }
  return g;
}

// One thread per float4 of [n_tok][128].  A free token s: g[s] = g~[s] + sum of g~[t] over the tokens t tied to s (ascending, from the
// CSR table), x_new[s] = x~[s] - step g[s].  A tied token computes its SOURCE's g and x_new by the same instructions, so it takes the
// source's new value bit for bit; its own gradient is 0.  Table entries out of range are skipped: no table reads out of bounds.
template <int = 0>
__global__ void guide_update_kernel(GuideUpdateArgs a) {
  const long long i = blockIdx.x * 256LL + threadIdx.x;
  if (i >= a.n_tok * 32) return;
  const long long tok = i >> 5;
  const int q = (int)(i & 31);
  const int v = a.tie ? a.tie[tok] : -1;
  const bool tied = v >= 0 && v < a.n_tok;
  const long long s = tied ? v : tok;
  float4 g = guide_chunk_sum(a, s, q);
  if (a.csr) {
    const long long lo = a.csr[s], hi = a.csr[s + 1];
    const long long beg = lo < 0 ? 0 : (lo > a.n_tok ? a.n_tok : lo), end = hi < beg ? beg : (hi > a.n_tok ? a.n_tok : hi);
    for (long long k = beg; k < end; ++k) {
      const int t = a.csr[a.n_tok + 1 + k];
      if (t < 0 || t >= a.n_tok) continue;
      const float4 r = guide_chunk_sum(a, t, q);
      g.x += r.x; g.y += r.y; g.z += r.z; g.w += r.w;
    }
  }
  if (a.x_new) {
    const float4 x = reinterpret_cast<const float4*>(a.xin)[s * 32 + q];
    reinterpret_cast<float4*>(a.x_new)[i] = make_float4(x.x - a.step * g.x, x.y - a.step * g.y, x.z - a.step * g.z, x.w - a.step * g.w);
  }
  if (a.grad) reinterpret_cast<float4*>(a.grad)[i] = tied ? make_float4(0.f, 0.f, 0.f, 0.f) : g;
}

namespace guide {

struct Bufs {   // GradState::guide_ws
  float *xin = nullptr, *d_out = nullptr, *g_rows = nullptr, *g_dir = nullptr, *partial = nullptr, *loss = nullptr;
};

static int ensure_bufs(Ctx* c, hipStream_t st, size_t n_tok, int n, Bufs& b) {
  auto layout = [&](ArenaLayout a) {
    const size_t n_be = (size_t)n * n_tok * CFD_LAT;
    a.take(b.xin, n_be); a.take(b.d_out, n_be); a.take(b.g_rows, n_be); a.take(b.g_dir, n_tok * CFD_LAT); a.take(b.partial, n_tok); a.take(b.loss, 1);
    return a.bytes();
  };
  DBuf& ws = c->grad.guide_ws;
  const size_t bytes = layout(ArenaLayout(nullptr, 64));
  if (bytes > ws.bytes) HIPCHK(hipStreamSynchronize(st));
  CHK(ws.ensure(bytes));
  layout(ArenaLayout(ws.as<float>(), 64));
  return CFD_OK;
}

// The call's launches: replicate, [time tables + memory side when `full`], the whole forward with saves, seed and loss, the reverse
// sweep from the seeded rows, reduce / fold / update.  wk[1]'s problem is prepared and its timestep set (rtgrad::begin_call).
static int enqueue(Ctx* c, hipStream_t st, const cfd_guide_args* a, const Bufs& b, bool full, float* grad, float* x_new) {
  rtgrad::WorkGuard guard(c);
  rtgrad::begin_sequence(c);
  RtGradState& s = c->grad.rt;
  const long long n_tok = (long long)a->B * a->L, total4 = (long long)a->n * n_tok * (CFD_LAT / 4);
  auto grid1 = [](long long n) { return dim3((unsigned)((n + 255) / 256)); };
  hipLaunchKernelGGL(guide_replicate_kernel<>, grid1(total4), dim3(256), 0, st, a->x, a->tie, b.xin, n_tok, total4);
  HIPCHK(hipGetLastError());
  ++s.launches;
  if (full) CHK(rtgrad::enqueue_memory_side(c, st));
  CHK(rtgrad::enqueue_forward_saved(c, st, b.xin));
  GuideSeedArgs sa{b.xin, c->w->eps.as<float>(), a->w, a->target, a->mask, b.d_out, b.g_dir, b.partial, n_tok, a->n, a->L,
                   a->sqrt_acp, a->sqrt_1m_acp, a->inv_n};
  hipLaunchKernelGGL(guide_seed_kernel<>, dim3((unsigned)n_tok), dim3(128), 0, st, sa);
  HIPCHK(hipGetLastError());
  hipLaunchKernelGGL(guide_loss_kernel<>, dim3(1), dim3(256), 0, st, b.partial, n_tok, a->inv_n, b.loss);
  HIPCHK(hipGetLastError());
  s.launches += 2;
  CHK(rtgrad::enqueue_reverse_sweep(c, st, rtgrad::SweepSeed{b.d_out}, b.g_rows));
  if (grad || x_new) {
    GuideUpdateArgs ua{b.xin, b.g_dir, b.g_rows, a->tie, a->tie ? a->tie_csr : nullptr, grad, x_new, n_tok, a->n, a->step};
    hipLaunchKernelGGL(guide_update_kernel<>, grid1(n_tok * 32), dim3(256), 0, st, ua);
    HIPCHK(hipGetLastError());
    ++s.launches;
  }
  return CFD_OK;
}

}  // namespace guide
