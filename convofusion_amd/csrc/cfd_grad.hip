// libcfdenoise: the row-tile gradient engine (rt_grad.hpp: the forward with saved activations and the reverse sweep of small problems,
// compiled here and nowhere else) and the entry points that seed the sweep at the forward's output -- cfd_denoise_vjp, the
// vector-Jacobian product of one forward with respect to its sample, with cfd_denoise_vjp_mem, which adds the product with respect to
// the five memories; and cfd_denoise_guide, the key-pose guided update on that forward and sweep (guide.hpp), with
// cfd_denoise_guide_pose, whose loss sits behind the VAE decoder (the fused decode and its sweep, cfd_blocks.hip).  cfd_weg_eval
// (cfd_weg.hip) is the engine's third caller.
#include "cfd_internal.hpp"

#include "rowtile_bwd.hpp"
#include "rt_grad.hpp"
#include "guide.hpp"

// ---- cfd_denoise_vjp: d_out^T . d(out)/d(sample) of one denoiser forward on the row-tile kernels --------------------------------
// Every refusal, before anything is touched; the row maps come back as the host sees them, with their part of the call's signature.
// `wants`: some result is asked for (cfd_denoise_vjp: grad; cfd_denoise_vjp_mem: grad or a d_mem[j]).
static int check_vjp_args(Ctx* c, const cfd_vjp_args* a, const float* d_out, bool wants, std::vector<long long>* more, HostMaps* hm) {
  if (!c || !a || !a->sample || !d_out || !wants) return fail(CFD_E_ARG, "null argument");
  const int Be = a->Be;
  CHK(check_latent_call(c, Be, a->L, a->mem, CALL_TIMESTEP | CALL_ROW_MAPS, a->timestep));
  if (const char* why = rtgrad::ineligible(c, Be, a->L, a->mem)) return fail(CFD_E_ARG, "cfd_denoise_vjp: %s", why);   // the row-tile path only
  if (c->grad.rt.stop) return fail(CFD_E_STATE, "cfd_debug_weg_stop is set: it names a launch of cfd_weg_eval's sweep");
  HIPCHK(hipSetDevice(c->cfg.device));
  CHK(fetch_row_maps(a->mem, Be, "Be", *hm));
  rtgrad::append_row_maps(*more, a->mem, *hm);
  return CFD_OK;
}

// One body for cfd_denoise_vjp (d_mem == null) and cfd_denoise_vjp_mem: the same arena, workspace, stream and census; the memory
// gradient adds its own buffers (GradState::mem_ws, the float32 folded weights) and launches (rtgrad::MemGrad) and nothing else.
// The call keeps nothing for reuse (mode 0, no signature stored).
static int denoise_vjp(Ctx* c, const cfd_vjp_args* a, const float* d_out, float* out, float* grad, float* const* d_mem, void* stream) {
  rtgrad::Call k{rtgrad::FOR_VJP};
  HostMaps hm;
  bool any_mem = false;
  for (int j = 0; d_mem && j < CFD_NMEM; ++j) any_mem = any_mem || d_mem[j] != nullptr;
  CHK(check_vjp_args(c, a, d_out, grad != nullptr || any_mem, &k.more, &hm));
  k.Be = a->Be; k.L = a->L; k.mem = a->mem; k.maps = &hm; k.mode = 0; k.timestep = a->timestep;
  hipStream_t st = c->own_stream;
  CHK(rtgrad::begin_call(c, k, (hipStream_t)stream));
  rtgrad::MemGrad mg;
  if (any_mem) {
    CHK(rtgrad::ensure_memw_f32(c, st));
    CHK(rtgrad::prepare_mem_grad(c, st, a->Be, a->L, a->mem, hm, d_mem, mg));
  }
  const int r = rtgrad::enqueue_vjp(c, st, a->sample, d_out, grad, any_mem ? &mg : nullptr);
  if (r == CFD_OK && out)
    HIPCHK(hipMemcpyAsync(out, c->wk[1].eps.p, (size_t)a->Be * a->L * CFD_LAT * 4, hipMemcpyDeviceToDevice, st));
  return rtgrad::finish_call(c, r, "cfd_denoise_vjp (sample, memories / their projections)");
}

extern "C" int cfd_denoise_vjp(cfd_handle c, const cfd_vjp_args* a, const float* d_out, float* out, float* grad, void* stream) {
  if (!grad) return fail(CFD_E_ARG, "null argument");
  return denoise_vjp(c, a, d_out, out, grad, nullptr, stream);
}

extern "C" int cfd_denoise_vjp_mem(cfd_handle c, const cfd_vjp_args* a, const float* d_out, float* out, float* grad, float* const d_mem[CFD_NUM_MEM],
                                   void* stream) {
  if (!d_mem) return fail(CFD_E_ARG, "null argument");
  return denoise_vjp(c, a, d_out, out, grad, d_mem, stream);
}

// ---- cfd_denoise_guide: the key-pose guided update as one device call (guide.hpp) ------------------------------------------------
extern "C" int cfd_guide_tie_csr(const int32_t* tie, long long n_tokens, int32_t* csr) {
  if (!tie || !csr || n_tokens < 1 || n_tokens > (1LL << 30)) return fail(CFD_E_ARG, "cfd_guide_tie_csr: bad argument");
  long long bad = -1;
  switch (guide_build_tie_csr(tie, n_tokens, csr, &bad)) {
    case GUIDE_CSR_OK: return CFD_OK;
    case GUIDE_CSR_RANGE: return fail(CFD_E_ARG, "cfd_guide_tie_csr: tie[%lld] = %d is not -1 or a token in [0, %lld)", bad, tie[bad], n_tokens);
    case GUIDE_CSR_SELF: return fail(CFD_E_ARG, "cfd_guide_tie_csr: tie[%lld] ties the token to itself", bad);
    default: return fail(CFD_E_ARG, "cfd_guide_tie_csr: tie[%lld] = %d names a source that is itself tied (no chains)", bad, tie[bad]);
  }
}

// Every refusal, before anything is touched; the row maps come back as the host sees them, with their part of the call's signature.
// pose_call: cfd_denoise_guide_pose, whose loss lives in `pose` -- args' own target and mask must be NULL and its inv_n is not read.
static int check_guide_args(Ctx* c, const cfd_guide_args* a, bool pose_call, const cfd_guide_pose* pose, bool wants, std::vector<long long>* more,
                            HostMaps* hm) {
  const char* who = pose_call ? "cfd_denoise_guide_pose" : "cfd_denoise_guide";
  if (!c || !a || !a->x) return fail(CFD_E_ARG, "null argument");
  if (!wants) return fail(CFD_E_ARG, "%s: none of loss, grad, x_new%s is asked for", who, pose_call ? ", d_out and feats" : " and d_out");
  if (a->n < 1) return fail(CFD_E_ARG, "%s: n = %d guidance chunks (at least 1)", who, a->n);
  if (a->B < 1 || a->L < 1) return fail(CFD_E_ARG, "bad batch / length");
  if (!pose_call) {
    if (!a->target || !a->mask) return fail(CFD_E_ARG, "cfd_denoise_guide: %s is NULL", !a->target ? "target" : "mask");
    if (!(a->inv_n > 0.f)) return fail(CFD_E_ARG, "cfd_denoise_guide: inv_n = %g is not positive (1 / (kept tokens * 128))", (double)a->inv_n);
  } else {
    if (a->target || a->mask)
      return fail(CFD_E_ARG, "cfd_denoise_guide_pose: args->%s is not NULL (the loss is the pose description's; the latent-token loss is cfd_denoise_guide's)",
                  a->target ? "target" : "mask");
    if (!pose) return fail(CFD_E_ARG, "cfd_denoise_guide_pose: pose is NULL");
    const char* null_field = !pose->wpack ? "wpack" : !pose->lengths ? "lengths" : !pose->target ? "target" : !pose->frame_mask ? "frame_mask"
                             : !pose->feature_mask ? "feature_mask" : nullptr;
    if (null_field) return fail(CFD_E_ARG, "cfd_denoise_guide_pose: pose->%s is NULL", null_field);
    if (!(pose->inv_n > 0.f))
      return fail(CFD_E_ARG, "cfd_denoise_guide_pose: inv_n = %g is not positive (1 / (selected frames * selected features))", (double)pose->inv_n);
    if (a->L % 2) return fail(CFD_E_ARG, "cfd_denoise_guide_pose: L = %d is odd (a latent chunk is a body and a hands token)", a->L);
    const cfd_vae_decode_args f = {pose->wpack, pose->d_model, pose->num_heads, pose->ff_size, pose->num_layers, a->B, pose->nframes, a->L / 2, nullptr,
                                   pose->lengths};
    CHK(vae_decode_check("cfd_denoise_guide_pose", &f));
    if (pose->nframes > 16 * (a->L / 2))
      return fail(CFD_E_ARG, "cfd_denoise_guide_pose: nframes = %d exceeds 16 * (L / 2) = %d, the frames of %d latent chunks", pose->nframes,
                  16 * (a->L / 2), a->L / 2);
  }
  if (!a->w) return fail(CFD_E_ARG, "%s: w (the chunk weights) is NULL", who);
  if (!(a->sqrt_acp > 0.f)) return fail(CFD_E_ARG, "%s: sqrt_acp = %g is not positive", who, (double)a->sqrt_acp);
  if (a->tie && !a->tie_csr) return fail(CFD_E_ARG, "%s: a tie without its tie_csr (cfd_guide_tie_csr)", who);
  if (a->reuse_memory_side != 0 && a->reuse_memory_side != 2)
    return fail(CFD_E_ARG, "%s: reuse_memory_side = %d is not 0 or 2", who, a->reuse_memory_side);
  // the row limit first, in 64 bits: Be = n * B is formed only once it fits
  if (const char* why = rtgrad::ineligible(c, (long long)a->n * a->B, a->L, a->mem, true)) return fail(CFD_E_ARG, "%s: %s", who, why);
  const int Be = a->n * a->B;
  CHK(check_latent_call(c, Be, a->L, a->mem, CALL_TIMESTEP | CALL_ROW_MAPS, a->timestep));
  if (c->grad.rt.stop) return fail(CFD_E_STATE, "cfd_debug_weg_stop is set: it names a launch of cfd_weg_eval's sweep");
  HIPCHK(hipSetDevice(c->cfg.device));
  CHK(fetch_row_maps(a->mem, Be, "n * B", *hm));
  more->push_back(a->n);
  rtgrad::append_row_maps(*more, a->mem, *hm);
  return CFD_OK;
}

// One body for cfd_denoise_guide (pose_call false) and cfd_denoise_guide_pose: the same arena, workspace, stream, census and signature --
// the memory side does not depend on the loss, so either call reuses what the other left.
static int denoise_guide(Ctx* c, const cfd_guide_args* a, bool pose_call, const cfd_guide_pose* pose, float* loss, float* grad, float* x_new,
                         float* d_out, float* feats, void* stream) {
  rtgrad::Call k{rtgrad::FOR_GUIDE};
  HostMaps hm;
  CHK(check_guide_args(c, a, pose_call, pose, loss || grad || x_new || d_out || feats, &k.more, &hm));
  const int Be = a->n * a->B;
  k.Be = Be; k.L = a->L; k.mem = a->mem; k.maps = &hm; k.mode = a->reuse_memory_side; k.timestep = a->timestep;
  hipStream_t st = c->own_stream;
  CHK(rtgrad::begin_call(c, k, (hipStream_t)stream));
  guide::Bufs b;
  const size_t pose_rows = pose ? (size_t)a->B * pose->nframes : 0;
  CHK(guide::ensure_bufs(c, (size_t)a->B * a->L, a->n, b, pose_rows));
  const int r = guide::enqueue(c, st, a, b, !k.reuse, grad, x_new, pose, "cfd_denoise_guide_pose");
  if (r == CFD_OK && loss) HIPCHK(hipMemcpyAsync(loss, b.loss, 4, hipMemcpyDeviceToDevice, st));
  if (r == CFD_OK && d_out) HIPCHK(hipMemcpyAsync(d_out, b.d_out, (size_t)Be * a->L * CFD_LAT * 4, hipMemcpyDeviceToDevice, st));
  if (r == CFD_OK && feats) HIPCHK(hipMemcpyAsync(feats, b.feats, pose_rows * GUIDE_NFEATS * 4, hipMemcpyDeviceToDevice, st));
  return rtgrad::finish_call(c, r, pose_call ? "cfd_denoise_guide_pose (x, memories / their projections)" : "cfd_denoise_guide (x, memories / their projections)",
                             &k.sig);
}

extern "C" int cfd_denoise_guide(cfd_handle c, const cfd_guide_args* a, float* loss, float* grad, float* x_new, float* d_out, void* stream) {
  return denoise_guide(c, a, false, nullptr, loss, grad, x_new, d_out, nullptr, stream);
}

extern "C" int cfd_denoise_guide_pose(cfd_handle c, const cfd_guide_args* a, const cfd_guide_pose* pose, float* loss, float* grad, float* x_new,
                                      float* d_out, float* feats, void* stream) {
  return denoise_guide(c, a, true, pose, loss, grad, x_new, d_out, feats, stream);
}
