// cfd_denoise_guide: one guided update of the sampling loop's latents by a key-pose loss of the predicted clean latents, as a device
// call -- the guidance combine, x0, the loss and its cotangent rows (guide_seed_kernel), the reverse sweep of cfd_denoise_vjp from them
// (rt_grad.hpp, unchanged), the sum over the guidance chunks, the fold of tied tokens' gradients onto their sources and the update
// (guide_update_kernel).  cfd_denoise_guide_pose puts the VAE decoder between x0 and the loss: guide_x0_kernel writes x0 in the decoder's
// layout, the saving decode and its sweep (cfd_blocks.hip) run on the handle's VAE workspace, guide_pose_seed_kernel forms the loss in
// pose space and its cotangent, guide_pose_back_kernel the cotangent rows from the sweep's d_z.  Float32 throughout, no atomics: the
// same inputs give the same bits.
// Included by cfd_grad.hip after rt_grad.hpp.
#pragma once

#include "guide_tables.hpp"

// (guide_replicate_kernel, the call's first launch, lives in cfd_internal.hpp: cfd_weg_step forms its x~ with it too.)

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

// ---- the pose-space loss (cfd_denoise_guide_pose) --------------------------------------------------------------------------------
// The run's combine of one element, in guide_seed_kernel's arithmetic and order; *sumw: the sum of the weights 1 .. n-1, ascending.
__device__ __forceinline__ float guide_combine(const float* __restrict__ eps_rows, const float* __restrict__ w, int n, long long chunk, long long e,
                                               float* sumw) {
  const float e0 = eps_rows[e];
  float eps = e0, sw = 0.f;
  for (int k = 1; k < n; ++k) {
    const float wk = w[k];
    eps = eps + wk * (eps_rows[k * chunk + e] - e0);
    sw += wk;
  }
  *sumw = sw;
  return eps;
}

// Token l = 2 p + part of latent row b lives at z[part][b][p][:] of the decoder's latent [2][B][L / 2][128] (edit.loop_to_vae).
__device__ __forceinline__ long long guide_z_index(long long tok, int L, long long B) {
  const long long b = tok / L;
  const int l = (int)(tok - b * L);
  return (((long long)(l & 1) * B + b) * (L / 2) + (l >> 1)) * CFD_LAT;
}

struct GuidePoseTokArgs {
  const float* xin;      // [n][n_tok][128]
  const float* eps;      // [n][n_tok][128]
  const float* w;        // [B][n]
  float* z;              // guide_x0_kernel: [2][B][L / 2][128], x0 in the decoder's layout
  const float* d_z;      // guide_pose_back_kernel: [2][B][L / 2][128], the decoder sweep's result
  float* d_out;          // [n][n_tok][128]
  float* g_dir;          // [n_tok][128]
  long long n_tok, B;
  int n, L;
  float s0, s1;
};

// One workgroup of 128 threads per token: x0 = (x~ - s1 eps) / s0 of the combined eps, written where the decoder reads it.
template <int = 0>
__global__ __launch_bounds__(128) void guide_x0_kernel(GuidePoseTokArgs a) {
  const long long tok = blockIdx.x;
  const int d = threadIdx.x;
  const long long e = tok * CFD_LAT + d;
  float sumw;
  const float eps = guide_combine(a.eps, a.w + (tok / a.L) * a.n, a.n, a.n_tok * CFD_LAT, e, &sumw);
  a.z[guide_z_index(tok, a.L, a.B) + d] = (a.xin[e] - a.s1 * eps) / a.s0;
}

// One workgroup of 128 threads per token: d_x0 read back through the layout map, then g_dir and the cotangent rows exactly as
// guide_seed_kernel forms them.
template <int = 0>
__global__ __launch_bounds__(128) void guide_pose_back_kernel(GuidePoseTokArgs a) {
  const long long tok = blockIdx.x;
  const int d = threadIdx.x;
  const long long e = tok * CFD_LAT + d, chunk = a.n_tok * CFD_LAT;
  const float* w = a.w + (tok / a.L) * a.n;
  float sumw = 0.f;
  for (int k = 1; k < a.n; ++k) sumw += w[k];
  const float dx0 = a.d_z[guide_z_index(tok, a.L, a.B) + d];
  const float back = -(a.s1 / a.s0);
  a.g_dir[e] = dx0 / a.s0;
  a.d_out[e] = back * (1.f - sumw) * dx0;
  for (int k = 1; k < a.n; ++k) a.d_out[k * chunk + e] = back * w[k] * dx0;
}

struct GuidePoseSeedArgs {
  const float* feats;          // [B][nframes][189]: the decode of x0 (frames at or beyond a length: exactly 0)
  const float* target;         // [B][nframes][189]
  const float* frame_mask;     // [B][nframes]
  const float* feature_mask;   // [189]
  float* d_feats;              // [B][nframes][189]
  float* partial;              // [B][nframes]: the frame's sum of r^2
  int nframes;
  float inv_n;
};

// Grid (nframes, B), 192 threads, one feature per thread: r = frame_mask feature_mask (feats - target), d_feats = 2 inv_n r.  The
// frame's sum of r^2: three wave reductions added in a fixed order.
template <int = 0>
__global__ __launch_bounds__(192) void guide_pose_seed_kernel(GuidePoseSeedArgs a) {
  __shared__ float part[3];
  const int j = threadIdx.x;
  const long long row = (long long)blockIdx.y * a.nframes + blockIdx.x;
  float v = 0.f;
  if (j < GUIDE_NFEATS) {
    const long long i = row * GUIDE_NFEATS + j;
    const float r = a.frame_mask[row] * a.feature_mask[j] * (a.feats[i] - a.target[i]);
    a.d_feats[i] = 2.f * a.inv_n * r;
    v = r * r;
  }
  for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
  if ((j & 63) == 0) part[j >> 6] = v;
  __syncthreads();
  if (j == 0) a.partial[row] = part[0] + part[1] + part[2];
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
  float *z = nullptr, *d_z = nullptr, *feats = nullptr, *d_feats = nullptr;   // cfd_denoise_guide_pose only
};

// pose_rows: B * nframes of a pose call (its partials are per frame), 0 of cfd_denoise_guide
static int ensure_bufs(Ctx* c, size_t n_tok, int n, Bufs& b, size_t pose_rows = 0) {
  return carve(c->grad.guide_ws, 64, [&](ArenaLayout& a) {
    const size_t n_be = (size_t)n * n_tok * CFD_LAT;
    a.take(b.xin, n_be); a.take(b.d_out, n_be); a.take(b.g_rows, n_be); a.take(b.g_dir, n_tok * CFD_LAT);
    a.take(b.partial, n_tok > pose_rows ? n_tok : pose_rows); a.take(b.loss, 1);
    if (pose_rows) {
      a.take(b.z, n_tok * CFD_LAT); a.take(b.d_z, n_tok * CFD_LAT); a.take(b.feats, pose_rows * GUIDE_NFEATS); a.take(b.d_feats, pose_rows * GUIDE_NFEATS);
    }
  });
}

// The call's launches: replicate, [time tables + memory side when `full`], the whole forward with saves, seed and loss, the reverse
// sweep from the seeded rows, reduce / fold / update.  wk[1]'s problem is prepared and its timestep set (rtgrad::begin_call).
// pose (cfd_denoise_guide_pose): in place of the seed launch x0 in the decoder's layout, the saving decode on the handle's VAE
// workspace, the loss in pose space, the decoder's sweep and the cotangent rows from its d_z; `who` names the call that drops the
// handle's kept decode.
static int enqueue(Ctx* c, hipStream_t st, const cfd_guide_args* a, const Bufs& b, bool full, float* grad, float* x_new,
                   const cfd_guide_pose* pose = nullptr, const char* who = nullptr) {
  rtgrad::WorkGuard guard(c);
  rtgrad::begin_sequence(c);
  RtGradState& s = c->grad.rt;
  const long long n_tok = (long long)a->B * a->L, total4 = (long long)a->n * n_tok * (CFD_LAT / 4);
  auto grid1 = [](long long n) { return dim3((unsigned)((n + 255) / 256)); };
  LAUNCH_COUNTED(s.launches, guide_replicate_kernel<>, grid1(total4), dim3(256), 0, st, a->x, a->tie, b.xin, n_tok, total4);
  if (full) CHK(rtgrad::enqueue_memory_side(c, st));
  CHK(rtgrad::enqueue_forward_saved(c, st, b.xin));
  if (!pose) {
    GuideSeedArgs sa{b.xin, c->w->eps.as<float>(), a->w, a->target, a->mask, b.d_out, b.g_dir, b.partial, n_tok, a->n, a->L,
                     a->sqrt_acp, a->sqrt_1m_acp, a->inv_n};
    LAUNCH_COUNTED(s.launches, guide_seed_kernel<>, dim3((unsigned)n_tok), dim3(128), 0, st, sa);
    LAUNCH_COUNTED(s.launches, guide_loss_kernel<>, dim3(1), dim3(256), 0, st, b.partial, n_tok, a->inv_n, b.loss);
  } else {
    GuidePoseTokArgs ta{b.xin, c->w->eps.as<float>(), a->w, b.z, b.d_z, b.d_out, b.g_dir, n_tok, a->B, a->n, a->L, a->sqrt_acp, a->sqrt_1m_acp};
    LAUNCH_COUNTED(s.launches, guide_x0_kernel<>, dim3((unsigned)n_tok), dim3(128), 0, st, ta);
    const cfd_vae_decode_args f = {pose->wpack, pose->d_model, pose->num_heads, pose->ff_size, pose->num_layers, a->B, pose->nframes, a->L / 2, b.z,
                                   pose->lengths};
    CHK(vae_decode_forward(c, who, &f, b.feats, true, false, st));
    c->vae.ticket = 0;   // this call's own forward: nobody holds its ticket, and its weights were not copied
    const long long rows = (long long)a->B * pose->nframes;
    GuidePoseSeedArgs sa{b.feats, pose->target, pose->frame_mask, pose->feature_mask, b.d_feats, b.partial, pose->nframes, pose->inv_n};
    LAUNCH_COUNTED(s.launches, guide_pose_seed_kernel<>, dim3((unsigned)pose->nframes, (unsigned)a->B), dim3(192), 0, st, sa);
    LAUNCH_COUNTED(s.launches, guide_loss_kernel<>, dim3(1), dim3(256), 0, st, b.partial, rows, pose->inv_n, b.loss);
    CHK(vae_decode_sweep(c, pose->wpack, b.d_feats, b.d_z, st));
    LAUNCH_COUNTED(s.launches, guide_pose_back_kernel<>, dim3((unsigned)n_tok), dim3(128), 0, st, ta);
  }
  CHK(rtgrad::enqueue_reverse_sweep(c, st, rtgrad::SweepSeed{b.d_out}, b.g_rows));
  if (grad || x_new) {
    GuideUpdateArgs ua{b.xin, b.g_dir, b.g_rows, a->tie, a->tie ? a->tie_csr : nullptr, grad, x_new, n_tok, a->n, a->step};
    LAUNCH_COUNTED(s.launches, guide_update_kernel<>, grid1(n_tok * 32), dim3(256), 0, st, ua);
  }
  return CFD_OK;
}

}  // namespace guide
