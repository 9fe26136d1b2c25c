// libcfdenoise: the T5 text encoder with the reference's projection -- token ids to the text memories in one call (cfd_t5_encode;
// kernels and the packed-weight layout: t5_enc.hpp).
#include "cfd_internal.hpp"
#include "t5_enc.hpp"

// One product.  The block shape follows the grid it gives -- 128 x 128 where that still fills the device, 64 x 64 below --; the bits do
// not: an element's k order is the same in both (t5_enc.hpp).
static int enqueue_t5_gemm(const T5GemmArgs& g, int n_cu, hipStream_t st, int& launches, int* big_launches) {
  if (g.K % T5_BK || g.N % 64) return fail(CFD_E_ARG, "t5 product: K %d / N %d", g.K, g.N);
  const long long big = (long long)((g.M + 127) / 128) * (g.N / 128);
  if (g.N % 128 == 0 && big >= n_cu) {
    *big_launches += 1;
    LAUNCH_COUNTED(launches, (t5_gemm_kernel<2, 2>), dim3((unsigned)(g.N / 128), (unsigned)((g.M + 127) / 128)), dim3(256), 0, st, g);
  } else {
    LAUNCH_COUNTED(launches, (t5_gemm_kernel<1, 1>), dim3((unsigned)(g.N / 64), (unsigned)((g.M + 63) / 64)), dim3(256), 0, st, g);
  }
  return CFD_OK;
}

extern "C" int cfd_t5_encode(cfd_handle c, const cfd_t5_args* a, float* out, void* stream) {
  if (!c) return fail(CFD_E_ARG, "null handle");
  c->t5.launches = c->t5.big_launches = 0;
  if (!a || !out || !a->wpack || !a->ids || !a->mask || !a->rel_bias) return fail(CFD_E_ARG, "cfd_t5_encode: bad argument (NULL pointer)");
  if (a->gated_act)
    return fail(CFD_E_ARG, "cfd_t5_encode implements the T5 v1.0 feed-forward (feed_forward_proj \"relu\"), not the gated activation of v1.1");
  if (a->d_model != T5_D || a->d_kv != T5_DKV || a->num_heads != T5_H || a->d_ff != T5_FF || a->num_layers < 1 || a->num_layers > T5_MAX_LAYERS)
    return fail(CFD_E_ARG, "cfd_t5_encode implements d_model 768, d_kv 64, 12 heads, d_ff 3072 and 1 - %d layers only (got %d, %d, %d, %d, %d)",
                T5_MAX_LAYERS, a->d_model, a->d_kv, a->num_heads, a->d_ff, a->num_layers);
  if (a->vocab < 1 || !(a->eps > 0.f)) return fail(CFD_E_ARG, "cfd_t5_encode needs vocab >= 1 and eps > 0 (got %d, %g)", a->vocab, (double)a->eps);
  if (a->proj_w && (!a->proj_b || a->proj_dim < 64 || a->proj_dim % 64))
    return fail(CFD_E_ARG, "cfd_t5_encode: a projection needs its bias and a width that is a positive multiple of 64 (got %d)", a->proj_dim);
  if (a->n_seq < 1 || a->T < 1 || a->T > T5_MAX_T)
    return fail(CFD_E_SHAPE, "cfd_t5_encode needs n_seq >= 1 and 1 <= T <= %d (got %d, %d)", T5_MAX_T, a->n_seq, a->T);
  const long long M = (long long)a->n_seq * a->T;
  if (M > (1LL << 21) || a->n_seq > 65535) return fail(CFD_E_SHAPE, "too many sequences or token rows for one call (%d, %lld)", a->n_seq, M);
  HIPCHK(hipSetDevice(c->cfg.device));
  if (!c->t5.n_cu) HIPCHK(hipDeviceGetAttribute(&c->t5.n_cu, hipDeviceAttributeMultiprocessorCount, c->cfg.device));
  const int n_cu = c->t5.n_cu;
  hipStream_t st = (hipStream_t)stream;

  float *x, *h, *qkv, *ctx, *f;
  CHK(carve(c->t5.ws, 64, [&](ArenaLayout& lay) {
    lay.take(x, (size_t)M * T5_D);
    lay.take(h, (size_t)M * T5_D);
    lay.take(qkv, (size_t)M * 3 * T5_D);
    lay.take(ctx, (size_t)M * T5_D);
    lay.take(f, (size_t)M * T5_FF);
  }));
  c->t5.x = x; c->t5.h = h; c->t5.qkv = qkv; c->t5.ctx = ctx; c->t5.f = f;
  c->t5.rows = M;

  const float* embed = a->wpack;
  const float* blocks = embed + (size_t)a->vocab * T5_D;
  const float* g_final = blocks + (size_t)a->num_layers * t5_block_floats();
  int launches = 0, big = 0;
  T5GemmArgs g;
  for (int l = 0; l < a->num_layers; ++l) {
    const float* g1 = blocks + (size_t)l * t5_block_floats();
    const float* wqkv = g1 + T5_D;
    const float* wo = wqkv + (size_t)3 * T5_D * T5_D;
    const float* g2 = wo + (size_t)T5_D * T5_D;
    const float* wi = g2 + T5_D;
    const float* wo_ff = wi + (size_t)T5_FF * T5_D;
    const bool first = l == 0;                 // block 0 reads x = embed[ids] where it needs it: no gather launch, no copy
    // q | k | v = rs(x) (x g1) Wqkv^T
    g = T5GemmArgs{};
    g.A = first ? embed : x; g.a_ids = first ? a->ids : nullptr; g.lda = T5_D; g.gain = g1; g.W = wqkv;
    g.Y = qkv; g.ldy = 3 * T5_D; g.M = (int)M; g.N = 3 * T5_D; g.K = T5_D; g.flags = T5_ROWSCALE; g.id_max = a->vocab - 1; g.eps = a->eps;
    CHK(enqueue_t5_gemm(g, n_cu, st, launches, &big));
    // ctx = softmax(q k^T + bias) v
    LAUNCH_COUNTED(launches, t5_attn_kernel, dim3((unsigned)((a->T + 63) / 64), T5_H, (unsigned)a->n_seq), dim3(64), 0, st, qkv, a->mask, a->rel_bias, ctx, a->T);
    // h = x + ctx Wo^T
    g = T5GemmArgs{};
    g.A = ctx; g.lda = T5_D; g.W = wo; g.R = first ? embed : x; g.r_ids = first ? a->ids : nullptr; g.ldr = T5_D;
    g.Y = h; g.ldy = T5_D; g.M = (int)M; g.N = T5_D; g.K = T5_D; g.id_max = a->vocab - 1; g.eps = a->eps;
    CHK(enqueue_t5_gemm(g, n_cu, st, launches, &big));
    // f = relu(rs(h) (h g2) Wi^T)
    g = T5GemmArgs{};
    g.A = h; g.lda = T5_D; g.gain = g2; g.W = wi; g.Y = f; g.ldy = T5_FF; g.M = (int)M; g.N = T5_FF; g.K = T5_D;
    g.flags = T5_ROWSCALE | T5_RELU_OUT; g.eps = a->eps;
    CHK(enqueue_t5_gemm(g, n_cu, st, launches, &big));
    // x' = h + f Wo_ff^T
    g = T5GemmArgs{};
    g.A = f; g.lda = T5_FF; g.W = wo_ff; g.R = h; g.ldr = T5_D; g.Y = x; g.ldy = T5_D; g.M = (int)M; g.N = T5_D; g.K = T5_FF; g.eps = a->eps;
    CHK(enqueue_t5_gemm(g, n_cu, st, launches, &big));
  }
  if (a->proj_w) {                             // out = rs(x) relu(x g_f) Wp^T + b
    g = T5GemmArgs{};
    g.A = x; g.lda = T5_D; g.gain = g_final; g.W = a->proj_w; g.bias = a->proj_b; g.Y = out; g.ldy = a->proj_dim; g.M = (int)M; g.N = a->proj_dim;
    g.K = T5_D; g.flags = T5_ROWSCALE | T5_RELU_A; g.eps = a->eps;
    CHK(enqueue_t5_gemm(g, n_cu, st, launches, &big));
  } else {                                     // the last hidden state
    LAUNCH_COUNTED(launches, t5_final_rows_kernel, dim3((unsigned)((M + 3) / 4)), dim3(256), 0, st, x, g_final, out, (int)M, a->eps);
  }
  c->t5.launches = launches;
  c->t5.big_launches = big;
  return CFD_OK;
}
