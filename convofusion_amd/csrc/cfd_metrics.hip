// libcfdenoise: motion evaluation -- the per-sequence metrics, the beat alignment, process_motion, the FGD embedding and its float64
// Frechet statistics in one call (cfd_motion_eval), and the mean pairwise distance (cfd_motion_diversity).  Kernels: metrics_eval.hpp.
#include "cfd_internal.hpp"
#include "metrics_eval.hpp"

constexpr int ME_MAX_SEQ = 65535;
constexpr int ME_MAX_F = 1024;
constexpr int ME_SEQ_CHUNK = 128;       // sequences per pass of the embedding net (its activations: 166 500 floats per sequence at F = 300)

static int enqueue_me_gemm(const float* A, long long a_row, long long a_batch, const float* W, const float* bias, float* Y, long long y_row,
                           long long y_batch, int M, int N, int K, float slope, int batch, hipStream_t st, int& launches) {
  MeGemmArgs g{A, a_row, a_batch, W, bias, Y, y_row, y_batch, M, N, K, slope};
  LAUNCH_COUNTED(launches, me_gemm_kernel, dim3((unsigned)((N + 63) / 64), (unsigned)((M + 63) / 64), (unsigned)batch), dim3(256), 0, st, g);
  return CFD_OK;
}

extern "C" int cfd_motion_eval(cfd_handle c, const cfd_motion_eval_args* a, void* stream) {
  if (!c) return fail(CFD_E_ARG, "null handle");
  c->metrics.launches = 0;
  if (!a || !a->pred) return fail(CFD_E_ARG, "cfd_motion_eval: bad argument (NULL pointer)");
  if (a->n_seq < 1 || a->n_seq > ME_MAX_SEQ) return fail(CFD_E_SHAPE, "cfd_motion_eval: 1 <= n_seq <= %d (got %d)", ME_MAX_SEQ, a->n_seq);
  if (a->n_frames < ME_T_MIN || a->n_frames > ME_T_MAX)
    return fail(CFD_E_SHAPE, "cfd_motion_eval: %d <= n_frames <= %d (got %d)", ME_T_MIN, ME_T_MAX, a->n_frames);
  if (a->stride < ME_FEAT) return fail(CFD_E_SHAPE, "cfd_motion_eval: a frame is %d floats, stride must be at least that (got %lld)", ME_FEAT, a->stride);
  if (a->order < 1 || a->order > ME_T_MAX) return fail(CFD_E_ARG, "cfd_motion_eval: 1 <= order <= %d (got %d)", ME_T_MAX, a->order);
  if (!(a->fps > 0.0) || !(a->sigma > 0.0)) return fail(CFD_E_ARG, "cfd_motion_eval: fps and sigma must be positive (got %g, %g)", a->fps, a->sigma);
  if ((a->srgr || a->srgr_count) && (!a->target || !a->semantic))
    return fail(CFD_E_ARG, "cfd_motion_eval: SRGR needs both target and semantic");
  if ((a->srgr || a->srgr_count) && !(a->srgr_threshold > 0.0))
    return fail(CFD_E_ARG, "cfd_motion_eval: srgr_threshold must be positive (got %g)", a->srgr_threshold);
  if (a->jitter && !a->target) return fail(CFD_E_ARG, "cfd_motion_eval: jitter needs target");
  if ((a->onset_t && !a->onset_off) || (a->align && (!a->onset_off || (a->n_onsets > 0 && !a->onset_t))))
    return fail(CFD_E_ARG, "cfd_motion_eval: the alignment needs onset_off [n_seq + 1] and onset_t [n_onsets]");
  if (a->n_onsets < 0) return fail(CFD_E_ARG, "cfd_motion_eval: n_onsets must not be negative (got %d)", a->n_onsets);
  const bool embed = a->embedding || a->stats;
  if (embed) {
    if (!a->fgd_pack) return fail(CFD_E_ARG, "cfd_motion_eval: the embedding needs fgd_pack");
    if (a->feature_length < 1 || a->feature_length > ME_MAX_F)
      return fail(CFD_E_SHAPE, "cfd_motion_eval: 1 <= feature_length <= %d (got %d)", ME_MAX_F, a->feature_length);
    if (a->n_frames != ME_EMB_FRAMES)
      return fail(CFD_E_SHAPE, "cfd_motion_eval: the embedding net takes %d frames (got %d)", ME_EMB_FRAMES, a->n_frames);
    if (a->embed_raw != 0 && a->embed_raw != 1) return fail(CFD_E_ARG, "cfd_motion_eval: embed_raw is 0 or 1 (got %d)", a->embed_raw);
    if (a->embed_raw && a->stride != ME_FEAT) return fail(CFD_E_SHAPE, "cfd_motion_eval: embed_raw needs dense frames, stride %d (got %lld)", ME_FEAT, a->stride);
  }
  HIPCHK(hipSetDevice(c->cfg.device));
  hipStream_t st = (hipStream_t)stream;
  const int B = a->n_seq, T = a->n_frames, F = a->feature_length;
  const int chunk = B < ME_SEQ_CHUNK ? B : ME_SEQ_CHUNK;

  float *proc_ws, *act, *emb_ws;
  CHK(carve(c->metrics.ws, 64, [&](ArenaLayout& lay) {
    lay.take(proc_ws, embed && !a->embed_raw && !a->processed ? (size_t)B * T * ME_FEAT : 0);
    lay.take(act, embed ? (size_t)chunk * me_act_floats(F) : 0);
    lay.take(emb_ws, embed && !a->embedding ? (size_t)B * F : 0);
  }));
  c->metrics.rows = B;

  const size_t lds = (size_t)T * ME_FEAT * sizeof(float);
  static unsigned long long attr_done = 0;
  CHK(once_per_device(attr_done, c->cfg.device, [&]() -> int {
    HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void*>(&me_stage_a_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                               (int)(ME_T_MAX * ME_FEAT * sizeof(float))));
    return CFD_OK;
  }));
  // (a buffer of 0 floats is still carved as a non-null pointer: whether stage A writes the processed motion is decided here, not by it)
  float* proc = a->processed ? a->processed : (embed && !a->embed_raw ? proc_ws : nullptr);
  MeStageAArgs s{};
  s.pred = a->pred; s.target = a->target; s.semantic = a->semantic; s.stride = a->stride; s.T = T; s.order = a->order; s.n_onsets = a->n_onsets;
  s.fps = a->fps; s.sigma = a->sigma; s.threshold = a->srgr_threshold; s.onset_off = a->onset_off; s.onset_t = a->onset_t;
  s.l1div = a->l1div; s.srgr = a->srgr; s.jitter = a->jitter; s.align = a->align; s.srgr_count = a->srgr_count; s.beats = a->beats;
  s.processed = proc;
  int launches = 0;
  LAUNCH_COUNTED(launches, me_stage_a_kernel, dim3((unsigned)B), dim3(ME_THREADS), lds, st, s);

  if (embed) {
    const size_t f = (size_t)F;
    const float* w1 = a->fgd_pack;          const float* b1 = w1 + f * (3 * ME_FEAT);
    const float* w2 = b1 + f;               const float* b2 = w2 + 2 * f * (3 * f);
    const float* w3 = b2 + 2 * f;           const float* b3 = w3 + 2 * f * (8 * f);
    const float* w4 = b3 + 2 * f;           const float* b4 = w4 + f * (6 * f);
    const float* wf = b4 + f;               const float* bf = wf + f * (59 * f);
    float* emb = a->embedding ? a->embedding : emb_ws;
    const long long n1 = 126LL * F, n2 = 124LL * 2 * F, n3 = 61LL * 2 * F, n4 = 59LL * F;
    float *h1 = act, *h2 = h1 + (size_t)chunk * n1, *h3 = h2 + (size_t)chunk * n2, *h4 = h3 + (size_t)chunk * n3;
    for (int s0 = 0; s0 < B; s0 += chunk) {
      const int nb = B - s0 < chunk ? B - s0 : chunk;
      const float* x = (a->embed_raw ? a->pred : proc) + (size_t)s0 * T * ME_FEAT;
      CHK(enqueue_me_gemm(x, ME_FEAT, (long long)T * ME_FEAT, w1, b1, h1, F, n1, 126, F, 3 * ME_FEAT, 0.2f, nb, st, launches));
      CHK(enqueue_me_gemm(h1, F, n1, w2, b2, h2, 2 * F, n2, 124, 2 * F, 3 * F, 0.2f, nb, st, launches));
      CHK(enqueue_me_gemm(h2, 4 * F, n2, w3, b3, h3, 2 * F, n3, 61, 2 * F, 8 * F, 0.2f, nb, st, launches));
      CHK(enqueue_me_gemm(h3, 2 * F, n3, w4, b4, h4, F, n4, 59, F, 6 * F, 1.f, nb, st, launches));
      CHK(enqueue_me_gemm(h4, n4, 0, wf, bf, emb + (size_t)s0 * F, F, 0, nb, F, 59 * F, 1.f, 1, st, launches));
    }
    if (a->stats) {
      const long long entries = 1 + (long long)F + (long long)F * F;
      LAUNCH_COUNTED(launches, me_stats_kernel, dim3((unsigned)((entries + 255) / 256)), dim3(256), 0, st, emb, B, F, a->stats);
    }
  }
  c->metrics.launches = launches;
  return CFD_OK;
}

extern "C" int cfd_motion_diversity(cfd_handle c, const float* x, int n, long long d, double* out, void* stream) {
  if (!c) return fail(CFD_E_ARG, "null handle");
  c->metrics.launches = 0;
  if (!x || !out) return fail(CFD_E_ARG, "cfd_motion_diversity: bad argument (NULL pointer)");
  if (n < 2 || n > ME_DIV_MAX_N) return fail(CFD_E_SHAPE, "cfd_motion_diversity: 2 <= n <= %d (got %d)", ME_DIV_MAX_N, n);
  if (d < 1 || d > (1LL << 24)) return fail(CFD_E_SHAPE, "cfd_motion_diversity: 1 <= d <= 2^24 (got %lld)", d);
  HIPCHK(hipSetDevice(c->cfg.device));
  hipStream_t st = (hipStream_t)stream;
  const int nt = (n + ME_DIV_TILE - 1) / ME_DIV_TILE;
  CHK(c->metrics.ws.grow((size_t)nt * nt * sizeof(double)));
  double* partial = c->metrics.ws.as<double>();
  int launches = 0;
  LAUNCH_COUNTED(launches, me_div_tile_kernel, dim3((unsigned)nt, (unsigned)nt), dim3(ME_THREADS), 0, st, x, n, d, partial);
  LAUNCH_COUNTED(launches, me_div_sum_kernel, dim3(1), dim3(ME_THREADS), 0, st, (const double*)partial, (long long)nt * nt, 0.5 * (double)n * (double)(n - 1), out);
  c->metrics.rows = n;
  c->metrics.launches = launches;
  return CFD_OK;
}
