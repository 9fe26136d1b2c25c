// libcfdenoise: developer / test hooks (include/cfdenoise_dev.h) -- stage-wise taps and internal buffers (the GEMM test / micro-benchmark
// hooks live in cfd_forward.hip, next to the product instances they launch).
#include "cfd_internal.hpp"

// ---- test hooks -----------------------------------------------------------------------------------------
extern "C" int cfd_debug_stop_stage(cfd_handle c, int stage) {
  if (!c) return fail(CFD_E_ARG, "null handle");
  c->stop_stage = stage;
  return CFD_OK;
}

extern "C" int cfd_debug_forward_operands(cfd_handle c, int policy) {
  if (!c) return fail(CFD_E_ARG, "null handle");
  if (policy != 0 && policy != 15) return fail(CFD_E_ARG, "cfd_debug_forward_operands: policy %d (0: split pairs, 15: single-fp16 tiles of the long memories)", policy);
  if (c->run.open) return fail(CFD_E_STATE, "a sampling run is open on this handle");
  if (policy != c->fwd_operands) c->wk[0].fwd_mem_valid = false;   // the work lists carry XA_F16 and k16 / v16 are made per call: nothing of the last forward is reused
  c->fwd_operands = policy;
  return CFD_OK;
}

extern "C" int cfd_debug_live_buffers(long long* count, long long* bytes) {
  if (!count || !bytes) return fail(CFD_E_ARG, "null argument");
  *count = g_dbuf_live; *bytes = g_dbuf_live_bytes;
  return CFD_OK;
}

extern "C" int cfd_debug_vae_workspace(cfd_handle c, long long* bytes) {
  if (!c || !bytes) return fail(CFD_E_ARG, "null argument");
  *bytes = (long long)c->vae.ws.bytes;
  return CFD_OK;
}

extern "C" int cfd_debug_weg_stop(cfd_handle c, int stop) {
  if (!c) return fail(CFD_E_ARG, "null handle");
  if (stop != 0) {
    if (!c->rt_on || !c->weg_rt_on) return fail(CFD_E_STATE, "cfd_debug_weg_stop: this handle does not evaluate on the row-tile path");
    const int l = stop / 16, k = stop % 16;
    const bool ok = stop > 0 && ((l < c->nl && k >= 1 && k <= 9 && !(l == c->nl - 1 && k < 5)) || stop == 10);
    if (!ok) return fail(CFD_E_ARG, "cfd_debug_weg_stop: %d names no launch of the reverse sweep (16 l + k, k = 1 .. 9; the top layer has no B1 .. B4; 10 = the embedding)", stop);
  }
  c->grad.rt.stop = stop;
  return CFD_OK;
}

// the buffers of the row-tile WEG evaluation's arena (include/cfdenoise_dev.h: cfd_debug_weg_stop)
static int weg_debug_buffer(Ctx* c, const char* what, float** p, size_t* n) {
  RtGradState& s = c->grad.rt;
  if (s.sig.empty() || !s.B) return fail(CFD_E_STATE, "'%s': no row-tile WEG evaluation has run on this handle", what);
  const size_t M = (size_t)s.B * s.L;
  int l = -1, k = -1;
  if (!strcmp(what, "weg.g")) {
    if (s.stop_gi < 0) return fail(CFD_E_STATE, "weg.g: the sweep has not written a running gradient yet");
    *p = s.G[s.stop_gi]; *n = M * CFD_D;
  } else if (!strcmp(what, "weg.g0") || !strcmp(what, "weg.g1") || !strcmp(what, "weg.g2")) { *p = s.G[what[5] - '0']; *n = M * CFD_D; }
  else if (!strcmp(what, "weg.dh")) { *p = s.dh; *n = M * CFD_FF; }
  else if (!strcmp(what, "weg.dy")) { *p = s.dy; *n = M * CFD_D; }
  else if (!strcmp(what, "weg.dz")) { *p = s.dz; *n = M * CFD_D; }
  else if (!strcmp(what, "weg.dO")) { *p = s.dO; *n = M * CFD_D; }
  else if (!strcmp(what, "weg.dqkv")) { *p = s.dqkv; *n = M * 3 * CFD_D; }
  else if (!strcmp(what, "weg.dP")) { *p = s.dP; *n = M * (size_t)s.Sp_tot; }
  else if (!strcmp(what, "weg.att")) { *p = s.att; *n = M * (size_t)c->nl * s.St; }
  else if (!strcmp(what, "weg.d_att")) { *p = s.d_att; *n = M * (size_t)c->nl * s.St; }
  else if (sscanf(what, "weg.x.%d.%d", &l, &k) == 2 && l >= 0 && l <= c->nl && k >= 0 && k < 5) { *p = s.sv.x[l][k]; *n = M * CFD_D; }
  else return fail(CFD_E_ARG, "unknown buffer '%s'", what);
  return CFD_OK;
}

extern "C" int cfd_debug_weg_fill(cfd_handle c, float value) {
  if (!c) return fail(CFD_E_ARG, "null handle");
  HIPCHK(hipSetDevice(c->cfg.device));
  static const char* const names[] = {"weg.g0", "weg.g1", "weg.g2", "weg.dh", "weg.dy", "weg.dz", "weg.dO", "weg.dqkv", "weg.dP"};
  HIPCHK(hipDeviceSynchronize());
  for (const char* nm : names) {
    float* p = nullptr;
    size_t n = 0;
    CHK(weg_debug_buffer(c, nm, &p, &n));
    std::vector<float> v(n, value);
    HIPCHK(hipMemcpy(p, v.data(), n * 4, hipMemcpyHostToDevice));
  }
  return CFD_OK;
}

extern "C" int cfd_debug_read(cfd_handle c, const char* what, float* dst_dev, size_t numel) {
  if (!c || !what || !dst_dev) return fail(CFD_E_ARG, "null argument");
  HIPCHK(hipSetDevice(c->cfg.device));
  if (!strcmp(what, "setup_launches")) {   // launches the last cfd_sample_begin spent on timestep-only tables (0: all served from the cache)
    const float f = (float)c->setup_launches;
    HIPCHK(hipMemcpy(dst_dev, &f, 4, hipMemcpyHostToDevice));
    return CFD_OK;
  }
  if (!strcmp(what, "sat")) {   // the saturation census as one float (not cleared)
    unsigned int n[2] = {0, 0};
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(hipMemcpy(n, c->sat.p, 8, hipMemcpyDeviceToHost));
    const float f = (float)n[0] + (float)n[1];
    HIPCHK(hipMemcpy(dst_dev, &f, 4, hipMemcpyHostToDevice));
    return CFD_OK;
  }
#if RT_STAMP
  if (!strcmp(what, "rt_ring")) {   // developer build: the launch time line (rowtile.hpp), 4 x 4096 64-bit words + the sequence counter
    HIPCHK(hipDeviceSynchronize());
    if (numel * 4 < sizeof(unsigned long long) * 4 * 4096 + 8) return fail(CFD_E_ARG, "rt_ring needs %zu bytes", sizeof(unsigned long long) * 4 * 4096 + 8);
    HIPCHK(hipMemcpyFromSymbol(dst_dev, HIP_SYMBOL(g_rt_ring), sizeof(unsigned long long) * 4 * 4096, 0, hipMemcpyDeviceToDevice));
    HIPCHK(hipMemcpyFromSymbol(reinterpret_cast<char*>(dst_dev) + sizeof(unsigned long long) * 4 * 4096, HIP_SYMBOL(g_rt_seq), 4, 0, hipMemcpyDeviceToDevice));
    return CFD_OK;
  }
#endif
  if (!strcmp(what, "weg.info")) {   // the last row-tile WEG evaluation: launches, Sp_tot, rt_xbwd_dy_kernel instance (keys), objective kernel (1: weg_focus_kernel), G index
    if (numel < 5) return fail(CFD_E_ARG, "weg.info needs 5 floats");
    const float f[5] = {(float)c->grad.rt.launches, (float)c->grad.rt.Sp_tot, (float)c->grad.rt.dy_keys, (float)c->grad.rt.focus_large, (float)c->grad.rt.stop_gi};
    HIPCHK(hipMemcpy(dst_dev, f, sizeof(f), hipMemcpyHostToDevice));
    return CFD_OK;
  }
  if (!strcmp(what, "xa.info")) {   // the last cfd_forward's cross-attention: kernel instance, work-list form
    if (numel < 7) return fail(CFD_E_ARG, "xa.info needs 7 floats");
    const Problem& p = c->wk[0].pb;
    const float f[7] = {(float)(p.path.xa_reached ? p.path.xa_inst : XA_INST_NONE), (float)p.xa_nwg, (float)p.xa_tpw, (float)p.xa_n16, (float)p.xa_nseg, p.xa_flush ? 1.f : 0.f, (float)p.xa_one};
    HIPCHK(hipMemcpy(dst_dev, f, sizeof(f), hipMemcpyHostToDevice));
    return CFD_OK;
  }
  if (!strcmp(what, "vae.info")) {   // the last cfd_vae_decode_vjp: launches, padded frames per sequence
    if (numel < 2) return fail(CFD_E_ARG, "vae.info needs 2 floats");
    const float f[2] = {(float)c->vae.launches, (float)c->vae.fp};
    HIPCHK(hipMemcpy(dst_dev, f, sizeof(f), hipMemcpyHostToDevice));
    return CFD_OK;
  }
  if (!strcmp(what, "t5.info")) {   // the last cfd_t5_encode: launches (0: refused), token rows, workspace bytes as allocated, launches that ran 128 x 128 blocks
    if (numel < 4) return fail(CFD_E_ARG, "t5.info needs 4 floats");
    const float f[4] = {(float)c->t5.launches, (float)c->t5.rows, (float)c->t5.ws.bytes, (float)c->t5.big_launches};
    HIPCHK(hipMemcpy(dst_dev, f, sizeof(f), hipMemcpyHostToDevice));
    return CFD_OK;
  }
  if (!strcmp(what, "audio.info")) {   // the last cfd_audio_encode / cfd_audio_power / cfd_audio_onsets: launches (0: refused), frames per waveform, output rows, workspace bytes as allocated
    if (numel < 4) return fail(CFD_E_ARG, "audio.info needs 4 floats");
    const float f[4] = {(float)c->audio.launches, (float)c->audio.frames, (float)c->audio.rows, (float)c->audio.ws.bytes};
    HIPCHK(hipMemcpy(dst_dev, f, sizeof(f), hipMemcpyHostToDevice));
    return CFD_OK;
  }
  if (!strcmp(what, "audio_enc_vjp.info")) {   // the last cfd_audio_encoder_vjp: launches (0: refused), rows, row segments, workspace bytes as allocated
    if (numel < 4) return fail(CFD_E_ARG, "audio_enc_vjp.info needs 4 floats");
    const float f[4] = {(float)c->audio_enc.launches, (float)c->audio_enc.rows, (float)c->audio_enc.segments, (float)c->audio_enc.ws.bytes};
    HIPCHK(hipMemcpy(dst_dev, f, sizeof(f), hipMemcpyHostToDevice));
    return CFD_OK;
  }
  if (!strcmp(what, "metrics.info")) {   // the last cfd_motion_eval / cfd_motion_diversity: launches (0: refused), sequences, workspace bytes as allocated
    if (numel < 3) return fail(CFD_E_ARG, "metrics.info needs 3 floats");
    const float f[3] = {(float)c->metrics.launches, (float)c->metrics.rows, (float)c->metrics.ws.bytes};
    HIPCHK(hipMemcpy(dst_dev, f, sizeof(f), hipMemcpyHostToDevice));
    return CFD_OK;
  }
  // the residual stream behind the last block, [rows][768] (in front of the final norm), and what the last block's launches left:
  // h = x + ctx Wo^T [rows][768], q | k | v [rows][2304], ctx [rows][768], f [rows][3072]
  const struct { const char* name; const float* p; long long width; } t5_taps[] = {
      {"t5.x", c->t5.x, 768}, {"t5.h", c->t5.h, 768}, {"t5.qkv", c->t5.qkv, 2304}, {"t5.ctx", c->t5.ctx, 768}, {"t5.f", c->t5.f, 3072}};
  for (const auto& t : t5_taps) {
    if (strcmp(what, t.name)) continue;
    if (!t.p) return fail(CFD_E_STATE, "no cfd_t5_encode has run on this handle");
    if (numel > (size_t)(c->t5.rows * t.width)) return fail(CFD_E_ARG, "buffer '%s' holds %lld floats, asked for %zu", t.name, c->t5.rows * t.width, numel);
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(hipMemcpy(dst_dev, t.p, numel * 4, hipMemcpyDeviceToDevice));
    return CFD_OK;
  }
  if (!strncmp(what, "vae.", 4)) {
    float* p = nullptr;
    size_t n = 0;
    CHK(vae_debug_buffer(c, what, &p, &n));
    if (numel > n) return fail(CFD_E_ARG, "buffer '%s' holds %zu floats, asked for %zu", what, n, numel);
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(hipMemcpy(dst_dev, p, numel * 4, hipMemcpyDeviceToDevice));
    return CFD_OK;
  }
  if (!strncmp(what, "weg.", 4)) {
    float* p = nullptr;
    size_t n = 0;
    CHK(weg_debug_buffer(c, what, &p, &n));
    if (numel > n) return fail(CFD_E_ARG, "buffer '%s' holds %zu floats, asked for %zu", what, n, numel);
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(hipMemcpy(dst_dev, p, numel * 4, hipMemcpyDeviceToDevice));
    return CFD_OK;
  }
  const DBuf* b = nullptr;
  if (!strcmp(what, "x")) b = &c->w->x;
  else if (!strcmp(what, "temb")) b = &c->w->temb_tab;
  else if (!strcmp(what, "ss")) b = &c->w->ss_tab;
  else if (!strcmp(what, "eps")) b = &c->w->eps;
  else if (!strcmp(what, "sc")) b = &c->w->sc;
  else if (!strcmp(what, "xa_stamps")) b = &c->w->xa_stamps;
  else return fail(CFD_E_ARG, "unknown buffer '%s'", what);
  if (numel * 4 > b->bytes) return fail(CFD_E_ARG, "buffer '%s' holds %zu bytes, asked for %zu", what, b->bytes, numel * 4);
  HIPCHK(hipDeviceSynchronize());
  HIPCHK(hipMemcpy(dst_dev, b->p, numel * 4, hipMemcpyDeviceToDevice));
  return CFD_OK;
}
