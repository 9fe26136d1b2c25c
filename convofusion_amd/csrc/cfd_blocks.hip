// libcfdenoise: float32 building blocks on device tensors -- the conditioning producers (cfd_linear_act) and the pieces of
// ConvoFusionVae.decode (cfd_layer_norm, cfd_mha, cfd_add, cfd_zero_rows) -- ConvoFusionVae.encode in one launch (cfd_vae_encode) and the
// fused decode, forward-only, kept for a later sweep, or with its sweep in one call (cfd_vae_decode, cfd_vae_decode_sweep, cfd_vae_decode_vjp).
#include "cfd_internal.hpp"
#include "vae_enc.hpp"
#include "vae_dec.hpp"

// ---- conditioning producers ---------------------------------------------------------------------------------
int enqueue_linear_act(const float* x, long long n_rows, int K, const float* W, const float* b, int N, int act, float* out, hipStream_t st) {
  const long long gy = (n_rows + 31) / 32;
  if (gy > 65535) return fail(CFD_E_ARG, "too many rows for one launch (%lld)", n_rows);
  hipLaunchKernelGGL(linear_act_kernel<>, dim3((unsigned)((N + 63) / 64), (unsigned)gy), dim3(256), 0, st, x, n_rows, K, W, b, N, act, out);
  hipError_t e = hipGetLastError();
  return e == hipSuccess ? CFD_OK : fail(CFD_E_HIP, "linear_act_kernel launch failed: %s", hipGetErrorString(e));
}

extern "C" int cfd_linear_act(cfd_handle c, const float* x, long long n_rows, int K, const float* W, const float* b, int N, int act,
                              float* out, void* stream) {
  if (!c || !x || !W || !out || n_rows < 1 || K < 1 || N < 1 || act < 0 || act > 2) return fail(CFD_E_ARG, "bad argument");
  HIPCHK(hipSetDevice(c->cfg.device));
  return enqueue_linear_act(x, n_rows, K, W, b, N, act, out, (hipStream_t)stream);
}

extern "C" int cfd_layer_norm(cfd_handle c, const float* x, long long rows, int D, const float* gamma, const float* beta, float eps,
                              float* out, void* stream) {
  if (!c || !x || !gamma || !beta || !out || rows < 1 || D < 1 || D > 2048) return fail(CFD_E_ARG, "bad argument (D <= 2048)");
  HIPCHK(hipSetDevice(c->cfg.device));
  hipLaunchKernelGGL(layernorm_f32_kernel<>, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, (hipStream_t)stream, x, gamma, beta, out, rows, D, eps);
  HIPCHK(hipGetLastError());
  return CFD_OK;
}

extern "C" int cfd_mha(cfd_handle c, const float* q, const float* k, const float* v, int Lq, int Lk, int bs, int E, int H,
                       const uint8_t* key_padding_mask, float* out, void* stream) {
  if (!c || !q || !k || !v || !out || Lq < 1 || Lk < 1 || bs < 1 || H < 1 || E % H) return fail(CFD_E_ARG, "bad argument");
  if (E / H > 64 || Lk > MHA_MAX_KEYS) return fail(CFD_E_SHAPE, "cfd_mha supports head_dim <= 64 and <= %d keys", MHA_MAX_KEYS);
  HIPCHK(hipSetDevice(c->cfg.device));
  const long long items = (long long)Lq * bs * H;
  const float scale = (float)(1.0 / std::sqrt((double)(E / H)));
  hipLaunchKernelGGL(mha_f32_kernel<>, dim3((unsigned)((items + 3) / 4)), dim3(256), 0, (hipStream_t)stream, q, k, v, key_padding_mask, out, Lq, Lk,
                     bs, E, H, scale);
  HIPCHK(hipGetLastError());
  return CFD_OK;
}

extern "C" int cfd_add(cfd_handle c, float* x, const float* y, size_t numel, void* stream) {
  if (!c || !x || !y || numel < 1) return fail(CFD_E_ARG, "bad argument");
  HIPCHK(hipSetDevice(c->cfg.device));
  hipLaunchKernelGGL(add_f32_kernel<>, dim3((unsigned)((numel + 255) / 256)), dim3(256), 0, (hipStream_t)stream, x, y, (long long)numel);
  HIPCHK(hipGetLastError());
  return CFD_OK;
}

extern "C" int cfd_zero_rows(cfd_handle c, float* x, const uint8_t* keep, long long rows, int D, void* stream) {
  if (!c || !x || !keep || rows < 1 || D < 1) return fail(CFD_E_ARG, "bad argument");
  HIPCHK(hipSetDevice(c->cfg.device));
  const long long n = rows * D;
  hipLaunchKernelGGL(zero_rows_f32_kernel<>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, x, keep, rows, D);
  HIPCHK(hipGetLastError());
  return CFD_OK;
}


// ---- ConvoFusionVae.encode (vae.py:162-266): csrc/vae_enc.hpp ----------------------------------------------------------------------
template <int RT>
static int launch_vae_encode(Ctx* c, const VaeEncArgs& a, int groups, int lds, hipStream_t st) {
  static unsigned long long attr_done = 0;
  CHK(once_per_device(attr_done, c->cfg.device, [&]() -> int {
    HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void*>(&vae_encode_kernel<RT>), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
    return CFD_OK;
  }));
  int launches = 0;   // (the call has no read-out; the launch goes the counted way for its check)
  LAUNCH_COUNTED(launches, vae_encode_kernel<RT>, dim3((unsigned)groups, 2), dim3(256), lds, st, a);
  return CFD_OK;
}

extern "C" int cfd_vae_encode(cfd_handle c, const float* wpack, int d_model, int num_heads, int ff_size, int num_layers, int latent_size,
                              const float* features, int bs, int nframes, long long row_stride, const int* lengths, float* mu_logvar,
                              float* feats_out, int seqs_per_group, void* stream) {
  if (!c || !wpack || !features || !lengths || !mu_logvar || !feats_out) return fail(CFD_E_ARG, "bad argument (NULL pointer)");
  if (d_model != VE_D || num_heads != 2 || ff_size != VE_FF || latent_size != 1 || num_layers < 1 || num_layers > VE_MAX_LAYERS || num_layers % 2 == 0)
    return fail(CFD_E_ARG, "cfd_vae_encode implements d_model 128, 2 heads, ff 1024, latent_size 1 and odd num_layers <= %d only "
                "(got %d, %d, %d, %d, %d)", VE_MAX_LAYERS, d_model, num_heads, ff_size, latent_size, num_layers);
  if (seqs_per_group < 0 || seqs_per_group > 3) return fail(CFD_E_ARG, "seqs_per_group must be 0 (automatic) or 1 - 3");
  if (bs < 1 || nframes < 16 || nframes % 16 || row_stride < VE_NFEATS)
    return fail(CFD_E_SHAPE, "cfd_vae_encode needs bs >= 1, nframes a positive multiple of 16 and row_stride >= 189 (got %d, %d, %lld)", bs,
                nframes, row_stride);
  const long long n_seq = (long long)bs * (nframes / 16);
  if (n_seq > (1LL << 30)) return fail(CFD_E_SHAPE, "too many sequences (%lld)", n_seq);
  const int nb = (num_layers - 1) / 2;
  HIPCHK(hipSetDevice(c->cfg.device));
  // row tiles per workgroup: G = 16 RT / 18 sequences share one pass over the weights.  Automatic choice: the fewest row-tile passes per
  // CU, counting padding rows, over the shapes whose LDS fits (smaller tiles give more workgroups at small batches).  Every shape holds
  // more than 256 registers per lane (VGPRs + AGPRs), so one workgroup runs per CU whatever its LDS.
  static int n_cu = 0;
  if (!n_cu) HIPCHK(hipDeviceGetAttribute(&n_cu, hipDeviceAttributeMultiprocessorCount, c->cfg.device));
  const int lds_max = 160 * 1024;
  int rt = 0;
  if (seqs_per_group) {
    rt = seqs_per_group + 1;
    if (ve_lds_bytes(rt, nb) > lds_max) return fail(CFD_E_SHAPE, "%d sequences per workgroup do not fit LDS at %d layers", seqs_per_group, num_layers);
  } else {
    long long best = 0;
    for (int t = 4; t >= 2; --t) {
      const int lds = ve_lds_bytes(t, nb);
      if (lds > lds_max) continue;
      const long long groups = 2 * ((n_seq + (16 * t / VE_T) - 1) / (16 * t / VE_T));
      const long long cost = (groups + n_cu - 1) / n_cu * t;
      if (!rt || cost < best) rt = t, best = cost;
    }
  }
  const int G = 16 * rt / VE_T;
  const long long groups = (n_seq + G - 1) / G;
  VaeEncArgs a;
  a.w = wpack;
  a.stack_floats = ve_stack_floats(num_layers);
  a.feats = features;
  a.row_stride = row_stride;
  a.lengths = lengths;
  a.mulv = mu_logvar;
  a.feats_out = feats_out;
  a.nframes = nframes;
  a.n_chunks = nframes / 16;
  a.n_seq = (int)n_seq;
  a.num_layers = num_layers;
  const int lds = ve_lds_bytes(rt, nb);
  hipStream_t st = (hipStream_t)stream;
  if (rt == 4) return launch_vae_encode<4>(c, a, (int)groups, lds, st);
  if (rt == 3) return launch_vae_encode<3>(c, a, (int)groups, lds, st);
  return launch_vae_encode<2>(c, a, (int)groups, lds, st);
}


// ---- ConvoFusionVae.decode, forward-only or kept for its sweep d(feats)/d(z) (autograd over vae.py:268-372): csrc/vae_dec.hpp ------------------
// One call path: cfd_vae_decode = vae_decode_forward; cfd_vae_decode_sweep = vae_decode_sweep; cfd_vae_decode_vjp = the two in a row.

static_assert(VE_NFEATS == GUIDE_NFEATS, "guide.hpp indexes the decode's output by GUIDE_NFEATS");

// the limits of the three entry points and of cfd_denoise_guide_pose (`who` names the caller in the message)
int vae_decode_check(const char* who, const cfd_vae_decode_args* p) {
  if (p->d_model != VE_D || p->num_heads != 2 || p->ff_size != VE_FF || p->num_layers < 1 || p->num_layers > VE_MAX_LAYERS || p->num_layers % 2 == 0)
    return fail(CFD_E_ARG, "%s implements d_model 128, 2 heads, ff 1024 and odd num_layers <= %d only (got %d, %d, %d, %d)", who,
                VE_MAX_LAYERS, p->d_model, p->num_heads, p->ff_size, p->num_layers);
  if (p->bs < 1 || p->bs > 65535) return fail(CFD_E_ARG, "%s takes 1 <= bs <= 65535 sequences (got %d)", who, p->bs);
  if (p->nframes < 1 || p->nframes > VD_MAX_FRAMES) return fail(CFD_E_ARG, "%s takes 1 <= nframes <= %d (got %d)", who, VD_MAX_FRAMES, p->nframes);
  if (p->n_chunks < 1 || p->n_chunks > VD_MAX_CHUNKS) return fail(CFD_E_ARG, "%s takes 1 <= n_chunks <= %d (got %d)", who, VD_MAX_CHUNKS, p->n_chunks);
  return CFD_OK;
}

// The shape fields of `a` from (nl, bs, nframes, n_chunks) and its workspace pointers named for `y`, whose granule is VD_GRANULE floats:
// every buffer starts on a float4.  save: the VJP workspace, every layer resident, in the order of VaeDecArgs.  Forward-only: what is live between
// two forward launches (vd_xslot, vd_lslot) -- per token row (nb + 2) stream slots, q | k | v and o: (nb + 6) * 512 bytes, 4096 at 5 layers
// -- and the memory's K | V, nl * 16 KiB per (stack, sequence); every other pointer null.  keep_w, the copy of the weights for a sweep in a
// later call, comes last and is only counted when `copy_w` asks for it: cfd_vae_decode_vjp sweeps inside the call and reads the caller's.
constexpr size_t VD_GRANULE = 4;
static void vae_decode_layout(VaeDecArgs& a, int nl, int bs, int nframes, int n_chunks, ArenaLayout& y, bool save, bool copy_w) {
  a.nl = nl;
  a.nb = (nl - 1) / 2;
  a.stack_floats = vd_stack_floats(nl);
  a.bs = bs;
  a.nframes = nframes;
  a.nt = (nframes + 15) / 16;
  a.fp = 16 * a.nt;
  a.n_chunks = n_chunks;
  a.rows = 2LL * bs * a.fp;
  const long long R = a.rows, L = nl, sb = 2LL * bs;
  a.x1 = a.x2 = a.lse = a.qc = a.g = a.g1 = a.d_o = a.dd = a.dqkv = a.gskip = a.pkv = a.dzl = a.keep_w = nullptr;
  a.keep_len = nullptr;
  if (!save) {
    y.take(a.x0, (a.nb + 2) * R * VE_D); y.take(a.qkv, R * 3 * VE_D); y.take(a.o, R * VE_D); y.take(a.mkv, L * sb * 16 * 256);
    return;
  }
  y.take(a.x0, (L + 1) * R * VE_D); y.take(a.x1, L * R * VE_D); y.take(a.x2, L * R * VE_D); y.take(a.qkv, L * R * 3 * VE_D);
  y.take(a.o, L * R * VE_D); y.take(a.lse, L * R * 2); y.take(a.qc, L * R * VE_D); y.take(a.mkv, L * sb * 16 * 256);
  y.take(a.g, L * R * VE_D); y.take(a.g1, R * VE_D); y.take(a.d_o, R * VE_D); y.take(a.dd, R * 2); y.take(a.dqkv, R * 3 * VE_D);
  y.take(a.gskip, (a.nb ? a.nb : 1) * R * VE_D); y.take(a.pkv, L * sb * a.nt * 16 * 256); y.take(a.dzl, L * sb * 16 * VE_D);
  y.take(a.keep_len, bs);
  y.take(a.keep_w, copy_w ? 2 * a.stack_floats : 0);
}

template <bool SAVE>
static int vae_decode_forward_launches(const VaeDecArgs& a, bool copy_w, hipStream_t st, int& n) {
  const dim3 grid((unsigned)a.nt, (unsigned)a.bs, 2), blk(256);
  // copy_w: about 256 more blocks, spread over the grid's first axis, copy the weights for a sweep in a later call
  const unsigned copy = SAVE && copy_w ? (unsigned)((256 + 2 * a.bs - 1) / (2 * a.bs)) : 0;
  LAUNCH_COUNTED(n, vd_mem_kernel<SAVE>, dim3((unsigned)a.nl + copy, (unsigned)a.bs, 2), blk, 0, st, a);
  for (int l = 0; l <= a.nl; ++l) {
    LAUNCH_COUNTED(n, vd_fwd_rows_kernel<SAVE>, grid, blk, 0, st, a, l);
    if (l < a.nl) LAUNCH_COUNTED(n, vd_self_fwd_kernel<SAVE>, grid, blk, 0, st, a, l);
  }
  return CFD_OK;
}

// The forward of `p` into feats (may be null with save).  Whatever forward the handle kept is dropped first: this one overwrites it.
// save: the activations and the lengths stay in the workspace and the handle's ticket names them; copy_w: the weights too.
int vae_decode_forward(Ctx* c, const char* who, const cfd_vae_decode_args* p, float* feats, bool save, bool copy_w, hipStream_t st) {
  auto& v = c->vae;
  v.ticket = 0;
  v.dropped_by = who;
  VaeDecArgs a;
  CHK(carve(v.ws, VD_GRANULE, [&](ArenaLayout& y) { vae_decode_layout(a, p->num_layers, p->bs, p->nframes, p->n_chunks, y, save, copy_w); }, &v.grew));
  a.w = p->wpack;
  a.qpe = p->wpack + 2 * a.stack_floats;
  a.mpe = a.qpe + (long long)VD_MAX_FRAMES * VE_D;
  a.z = p->z;
  a.lengths = p->lengths;
  a.d_feats = nullptr;
  a.feats = feats;
  a.d_z = nullptr;
  v.g = a.g; v.dzl = a.dzl; v.x0 = save ? a.x0 : nullptr;
  v.bs = a.bs; v.fp = a.fp; v.nl = a.nl; v.rows = a.rows; v.nframes = a.nframes; v.n_chunks = a.n_chunks;
  int n = 0;
  CHK(save ? vae_decode_forward_launches<true>(a, copy_w, st, n) : vae_decode_forward_launches<false>(a, false, st, n));
  v.launches = v.fwd_launches = n;
  if (save) v.ticket = ++v.serial;
  return CFD_OK;
}

// The reverse sweep over the handle's kept forward: reads the workspace (activations, lengths), d_feats and the packed weights `w` -- null:
// the copy the forward kept, so that nothing of the caller's is read but d_feats.
int vae_decode_sweep(Ctx* c, const float* w, const float* d_feats, float* d_z, hipStream_t st) {
  auto& v = c->vae;
  VaeDecArgs a;
  ArenaLayout y(v.ws.as<float>(), VD_GRANULE);   // over the forward's allocation: the sweep neither sizes nor grows
  vae_decode_layout(a, v.nl, v.bs, v.nframes, v.n_chunks, y, true, true);
  a.w = w ? w : a.keep_w;
  a.lengths = a.keep_len;
  a.qpe = a.mpe = a.z = nullptr;
  a.feats = nullptr;
  a.d_feats = d_feats;
  a.d_z = d_z;
  const dim3 grid((unsigned)a.nt, (unsigned)a.bs, 2), blk(256);
  int n = 0;
  for (int l = a.nl - 1; l >= 0; --l) {
    LAUNCH_COUNTED(n, vd_bwd_rows_kernel, grid, blk, 0, st, a, l);
    if (l > 0) LAUNCH_COUNTED(n, vd_self_bwd_kernel, grid, blk, 0, st, a, l);
  }
  LAUNCH_COUNTED(n, vd_dz_kernel, dim3((unsigned)a.bs, 2, (unsigned)a.nl), blk, 0, st, a);
  LAUNCH_COUNTED(n, vd_dz_sum_kernel, dim3((unsigned)a.bs, 2), blk, 0, st, a);
  v.launches = v.fwd_launches + n;
  return CFD_OK;
}

extern "C" int cfd_vae_decode(cfd_handle c, const cfd_vae_decode_args* p, float* feats, uint64_t* ticket, void* stream) {
  if (!c || !p || !p->wpack || !p->z || !p->lengths || (!feats && !ticket)) return fail(CFD_E_ARG, "bad argument (NULL pointer)");
  CHK(vae_decode_check("cfd_vae_decode", p));
  HIPCHK(hipSetDevice(c->cfg.device));
  CHK(vae_decode_forward(c, "cfd_vae_decode", p, feats, ticket != nullptr, ticket != nullptr, (hipStream_t)stream));
  if (ticket) *ticket = c->vae.ticket;
  return CFD_OK;
}

extern "C" uint64_t cfd_vae_decode_ticket(cfd_handle c) { return c ? c->vae.ticket : 0; }

extern "C" int cfd_vae_decode_sweep(cfd_handle c, uint64_t ticket, const float* d_feats, float* d_z, void* stream) {
  if (!c || !d_feats || !d_z) return fail(CFD_E_ARG, "bad argument (NULL pointer)");
  const auto& v = c->vae;
  if (!ticket || ticket != v.ticket) {
    if (v.ticket) return fail(CFD_E_STATE, "cfd_vae_decode_sweep: ticket %llu is stale: the handle keeps the forward of ticket %llu", (unsigned long long)ticket, (unsigned long long)v.ticket);
    if (!v.dropped_by) return fail(CFD_E_STATE, "cfd_vae_decode_sweep: ticket %llu: no cfd_vae_decode has kept a forward on this handle", (unsigned long long)ticket);
    return fail(CFD_E_STATE, "cfd_vae_decode_sweep: ticket %llu is stale: a later %s%s dropped the kept forward", (unsigned long long)ticket, v.dropped_by,
                v.grew ? ", which also grew the VAE workspace," : "");
  }
  HIPCHK(hipSetDevice(c->cfg.device));
  return vae_decode_sweep(c, nullptr, d_feats, d_z, (hipStream_t)stream);
}

extern "C" int cfd_vae_decode_vjp(cfd_handle c, const cfd_vae_decode_vjp_args* p, float* feats, float* d_z, void* stream) {
  if (!c || !p || !p->wpack || !p->z || !p->lengths || !p->d_feats || !d_z) return fail(CFD_E_ARG, "bad argument (NULL pointer)");
  const cfd_vae_decode_args f = {p->wpack, p->d_model, p->num_heads, p->ff_size, p->num_layers, p->bs, p->nframes, p->n_chunks, p->z, p->lengths};
  CHK(vae_decode_check("cfd_vae_decode_vjp", &f));
  HIPCHK(hipSetDevice(c->cfg.device));
  CHK(vae_decode_forward(c, "cfd_vae_decode_vjp", &f, feats, true, false, (hipStream_t)stream));
  c->vae.ticket = 0;   // this call's own forward: nobody holds its ticket, and its weights were not copied
  return vae_decode_sweep(c, p->wpack, p->d_feats, d_z, (hipStream_t)stream);
}

// "vae.g.<l>": the running gradient at layer l's output, rows ((stack * bs + b) * fp + f), fp = nframes rounded up to 16; "vae.dz.<l>": layer
// l's contribution to d_z as [2][bs][16][128]; "vae.x.<l>": the forward's stream at layer l's input (l = num_layers: the last layer's output)
int vae_debug_buffer(Ctx* c, const char* what, float** p, size_t* n) {
  const auto& v = c->vae;
  if (!v.g) return fail(CFD_E_STATE, "'%s': no cfd_vae_decode_vjp has run on this handle (or a forward-only cfd_vae_decode since)", what);
  int l = -1;
  if (sscanf(what, "vae.g.%d", &l) == 1 && l >= 0 && l < v.nl) { *p = v.g + (size_t)l * v.rows * VE_D; *n = (size_t)v.rows * VE_D; }
  else if (sscanf(what, "vae.dz.%d", &l) == 1 && l >= 0 && l < v.nl) { *p = v.dzl + (size_t)l * 2 * v.bs * 16 * VE_D; *n = (size_t)2 * v.bs * 16 * VE_D; }
  else if (sscanf(what, "vae.x.%d", &l) == 1 && l >= 0 && l <= v.nl) { *p = v.x0 + (size_t)l * v.rows * VE_D; *n = (size_t)v.rows * VE_D; }
  else return fail(CFD_E_ARG, "unknown buffer '%s'", what);
  return CFD_OK;
}
