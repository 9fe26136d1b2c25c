// libcfdenoise: word-excitation guidance -- the launch-by-launch float32 pieces (cfd_gemm_f32 ... cfd_weg_focus) and cfd_weg_eval: one evaluation of the word-excitation-guidance objective and its gradient, all launches enqueued from C++
// (float32 launch sequence: weg_eval.hpp; small problems on the row-tile gradient engine: weg_rt.hpp, which calls into cfd_grad.hip).
// cfd_weg_step, at the end: the evaluation with every row its own utterance and the per-row gated, tied update, on the engine only.
#include "cfd_internal.hpp"
#include "grad.hpp"

#include "weg_eval.hpp"
#include "weg_rt.hpp"

extern "C" int cfd_gemm_f32(cfd_handle c, int M, int N, int K, int nb1, int nb2, const cfd_mat* A, const cfd_mat* B, const cfd_mat* Cm,
                            const float* bias, float alpha, int accumulate, void* stream) {
  if (!c || !A || !B || !Cm || !A->p || !B->p || !Cm->p || M < 1 || N < 1 || K < 1 || nb1 < 1 || nb2 < 1) return fail(CFD_E_ARG, "bad argument");
  if ((long long)nb1 * nb2 > 65535) return fail(CFD_E_SHAPE, "cfd_gemm_f32: at most 65535 batch entries");
  HIPCHK(hipSetDevice(c->cfg.device));
  MatView a{A->p, A->rs, A->cs, A->b1, A->b2}, b{B->p, B->rs, B->cs, B->b1, B->b2};
  launch_gemm_f32((hipStream_t)stream, a, b, const_cast<float*>(Cm->p), Cm->rs, Cm->cs, Cm->b1, Cm->b2, M, N, K, nb1, nb2, bias, alpha, accumulate);
  HIPCHK(hipGetLastError());
  return CFD_OK;
}

extern "C" int cfd_softmax(cfd_handle c, float* scores, long long rows, int Lk, const uint8_t* key_padding_mask, long long rows_per_batch,
                           void* stream) {
  if (!c || !scores || rows < 1 || Lk < 1 || rows_per_batch < 1) return fail(CFD_E_ARG, "bad argument");
  HIPCHK(hipSetDevice(c->cfg.device));
  hipLaunchKernelGGL(softmax_f32_kernel<>, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, (hipStream_t)stream, scores, key_padding_mask, rows, Lk,
                     rows_per_batch);
  HIPCHK(hipGetLastError());
  return CFD_OK;
}

extern "C" int cfd_softmax_bwd(cfd_handle c, const float* p, float* dp, const float* extra, long long rows, int Lk, void* stream) {
  if (!c || !p || !dp || rows < 1 || Lk < 1) return fail(CFD_E_ARG, "bad argument");
  HIPCHK(hipSetDevice(c->cfg.device));
  hipLaunchKernelGGL(softmax_bwd_f32_kernel<>, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, (hipStream_t)stream, p, dp, extra, rows, Lk);
  HIPCHK(hipGetLastError());
  return CFD_OK;
}

extern "C" int cfd_layer_norm_bwd(cfd_handle c, const float* x, const float* gamma, const float* dy, float* dx, long long rows, int D, float eps,
                                  int accumulate, void* stream) {
  if (!c || !x || !gamma || !dy || !dx || rows < 1 || D < 1 || D > 2048) return fail(CFD_E_ARG, "bad argument (D <= 2048)");
  HIPCHK(hipSetDevice(c->cfg.device));
  hipLaunchKernelGGL(layernorm_bwd_f32_kernel<>, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, (hipStream_t)stream, x, gamma, dy, dx, rows, D, eps,
                     accumulate, (const float*)nullptr, (const float*)nullptr);
  HIPCHK(hipGetLastError());
  return CFD_OK;
}

extern "C" int cfd_ew(cfd_handle c, int op, const float* a, const float* b, float* out, size_t numel, int D, int R1, long long s0, long long s1,
                      float alpha, void* stream) {
  if (!c || !a || !out || numel < 1 || op < 0 || op >= EW_NOPS) return fail(CFD_E_ARG, "bad argument");
  if (op >= EW_SILU_BWD && !b) return fail(CFD_E_ARG, "cfd_ew: this op needs the second operand");
  if (op >= EW_ADD_BCAST && (D < 1 || R1 < 1)) return fail(CFD_E_ARG, "cfd_ew: D and R1 must be positive");
  HIPCHK(hipSetDevice(c->cfg.device));
  hipLaunchKernelGGL(ew_f32_kernel<>, dim3((unsigned)((numel + 255) / 256)), dim3(256), 0, (hipStream_t)stream, op, a, b, out, (long long)numel,
                     D > 0 ? D : 1, R1 > 0 ? R1 : 1, s0, s1, alpha);
  HIPCHK(hipGetLastError());
  return CFD_OK;
}

extern "C" int cfd_weg_focus(cfd_handle c, const float* att, int B, int NL, int L, int S, const int32_t* tok_off, const int32_t* tok_idx, int last,
                             int nt_max, const float kernel3[3], float* workspace, float* losses, float* max_att, float* d_att, void* stream) {
  if (!c || !att || !tok_off || !tok_idx || !kernel3 || !workspace || !losses || !max_att || !d_att || B < 1 || NL < 1 || nt_max < 1)
    return fail(CFD_E_ARG, "bad argument");
  // F.pad(..., mode='reflect') with pad 1 needs at least 2 entries per axis (word_excitation_guidance.py:35)
  if (L < 2 || last - 1 < 2 || last > S) return fail(CFD_E_SHAPE, "text slice [1, %d) of %d keys / %d frames is too short for the 3x3 reflect-padded smoothing", last, S, L);
  HIPCHK(hipSetDevice(c->cfg.device));
  hipLaunchKernelGGL(weg_focus_kernel<>, dim3((unsigned)B), dim3(256), 0, (hipStream_t)stream, att, tok_off, tok_idx, B, NL, L, S, last, nt_max,
                     kernel3[0], kernel3[1], kernel3[2], workspace, losses, max_att, d_att, (const int*)nullptr, B);
  HIPCHK(hipGetLastError());
  return CFD_OK;
}

// The staging buffer (WegState::io) in floats: [latents | timestep row | losses | max_att | grad], losses and max_att rounded up to 64
struct WegStaging {
  size_t n_lat, n_max, o_lat = 0, o_trow, o_loss, o_max, o_grad, n_io;
  WegStaging(int B, int L, int D, int n_tok)
      : n_lat((size_t)B * L * CFD_LAT), n_max((size_t)std::max(1, n_tok)), o_trow(n_lat), o_loss(o_trow + (size_t)D),
        o_max(o_loss + (size_t)((B + 63) / 64 * 64)), o_grad(o_max + (n_max + 63) / 64 * 64), n_io(o_grad + n_lat) {}
};

struct WegEval {   // one evaluation, handed from stage to stage
  Ctx* c;
  const cfd_weg_args* a;
  hipStream_t caller, st;     // the caller's stream; the handle's own, which the evaluation runs on
  int B, L, D, n_tok, nt_max;
  WegStaging lay;
  float* io = nullptr;
  weg::Args args{};           // what the launches read and write: staged addresses only
  bool use_rt = false, reuse = false;   // on the row-tile gradient engine (weg_rt.hpp), else the float32 launch sequence; the memory side is skipped
  const void* arena = nullptr;
  weg::Ctx x{};               // the float32 launch sequence's pass
  std::vector<long long> sig, key;
};

// Every refusal, before anything is touched; yields the most focus tokens of a batch row.
static int check_args(Ctx* c, const cfd_weg_args* a, const float* losses, const float* max_att, const float* grad, int* nt_max_out) {
  if (!c || !a || !a->latents || !a->tok_off || !losses || !max_att || !grad) return fail(CFD_E_ARG, "null argument");
  CHK(check_latent_call(c, a->B, a->L, a->mem, CALL_TIMESTEP, a->timestep));   // (one memory per row: no row maps)
  const int B = a->B;
  if (c->cfg.text_encoded_dim > 2048) return fail(CFD_E_SHAPE, "model width above 2048");
  const int St = a->mem[2].S, n_tok = a->tok_off[B];
  if (a->tok_off[0] != 0 || n_tok < 0 || (n_tok > 0 && !a->tok_idx)) return fail(CFD_E_ARG, "bad focus-token table");
  // F.pad(..., mode='reflect') with pad 1 needs at least 2 entries per axis (word_excitation_guidance.py:35)
  if (a->last - 1 < 2 || a->last > St) return fail(CFD_E_SHAPE, "text slice [1, %d) of %d keys is too short for the 3x3 reflect-padded smoothing", a->last, St);
  int nt_max = 1;
  for (int b = 0; b < B; ++b) {
    if (a->tok_off[b + 1] < a->tok_off[b]) return fail(CFD_E_ARG, "bad focus-token table");
    nt_max = std::max(nt_max, a->tok_off[b + 1] - a->tok_off[b]);
  }
  for (int t = 0; t < n_tok; ++t)
    if (a->tok_idx[t] < 1 || a->tok_idx[t] > a->last - 1) return fail(CFD_E_ARG, "focus index %d is outside the text slice [1, %d)", a->tok_idx[t], a->last);
  // test hook (cfd_debug_weg_stop): a stop names a launch of the row-tile reverse sweep, so the evaluation must take that path
  if (c->grad.rt.stop && !wegrt::eligible(c, a)) return fail(CFD_E_STATE, "cfd_debug_weg_stop is set, but this evaluation is not eligible for the row-tile path");
  *nt_max_out = nt_max;
  return CFD_OK;
}

// The focus-token tables go to the device when they change (the stream may still read the old copy).
static int upload_focus_tokens(WegEval& e) {
  WegState& w = e.c->weg;
  std::vector<int32_t> tok(e.a->tok_off, e.a->tok_off + e.B + 1);
  tok.insert(tok.end(), e.a->tok_idx, e.a->tok_idx + e.n_tok);
  if (tok == w.tok_host) return CFD_OK;
  HIPCHK(hipStreamSynchronize(e.st));
  CHK(w.tok.ensure((size_t)(e.B + 1 + std::max(1, e.n_tok)) * 4));
  HIPCHK(hipMemcpy(w.tok.p, tok.data(), tok.size() * 4, hipMemcpyHostToDevice));
  w.tok_host = tok;
  ++w.tok_version;
  return CFD_OK;
}

// Latents and the timestep's sinusoid row into the staging buffer; from here on the launches see staged addresses only.
static int stage_inputs(WegEval& e) {
  Ctx* c = e.c;
  const cfd_weg_args* a = e.a;
  const WegStaging& y = e.lay;
  if (y.n_io * 4 > c->weg.io.bytes) HIPCHK(hipStreamSynchronize(e.st));
  CHK(c->weg.io.ensure(y.n_io * 4));
  float* io = e.io = c->weg.io.as<float>();
  HIPCHK(hipMemcpyAsync(io + y.o_lat, a->latents, y.n_lat * 4, hipMemcpyDeviceToDevice, e.st));
  HIPCHK(hipMemcpyAsync(io + y.o_trow, c->tsin.as<float>() + (size_t)a->timestep * e.D, (size_t)e.D * 4, hipMemcpyDeviceToDevice, e.st));
  const int32_t* tok = c->weg.tok.as<int32_t>();
  e.args = weg::Args{io + y.o_lat, io + y.o_trow, a->mem, tok, tok + e.B + 1, a->last, e.nt_max, {a->kernel3[0], a->kernel3[1], a->kernel3[2]},
                     io + y.o_loss, io + y.o_max, io + y.o_grad};
  return CFD_OK;
}

// The evaluation's first step, on the path check_args' shapes decide: small problems (the product shape) are a call on the row-tile
// gradient engine -- rtgrad::begin_call prepares its problem and arena and decides the reuse of the memory side
// (cfd_weg_args::reuse_memory_side; the modes are described there) -- everything else runs the float32 launch sequence of
// weg_eval.hpp, which only starts behind the caller's stream here (size_f32_sequence_and_reuse follows the staging).
static int begin(WegEval& e) {
  const cfd_weg_args* a = e.a;
  e.use_rt = wegrt::eligible(e.c, a);
  if (!e.use_rt) return rtgrad::begin_on_own_stream(e.c, e.caller);
  rtgrad::Call k{rtgrad::FOR_WEG, a->B, a->L, a->mem, nullptr, {}, a->reuse_memory_side, a->timestep};
  CHK(rtgrad::begin_call(e.c, k, e.caller));
  e.sig = k.sig;
  e.reuse = k.reuse;
  e.arena = e.c->grad.rt_ws.p;
  return CFD_OK;
}

// The float32 launch sequence's arena and its own reuse rule: the signature carries the timestep, so reuse_memory_side = 2 with a new
// timestep is treated as 0.
static int size_f32_sequence_and_reuse(WegEval& e) {
  Ctx* c = e.c;
  const cfd_weg_args* a = e.a;
  WegState& w = c->weg;
  e.sig = {e.B, e.L};
  rtgrad::append_memories(e.sig, a->mem);
  e.sig.push_back(a->timestep);
  e.x = weg::Ctx::sizing_pass(c, e.st, e.B, e.L, e.D);
  weg::run(e.x, e.args);
  if (e.x.err) return fail(e.x.err, "missing tensor '%s' (state-dict key denoiser.%s)", e.x.missing.c_str(), e.x.missing.c_str());
  if (e.x.off > w.ws.bytes) HIPCHK(hipStreamSynchronize(e.st));
  CHK(w.ws.ensure(e.x.off));
  e.arena = w.ws.p;
  e.sig.insert(e.sig.end(), {(long long)(size_t)e.arena, (long long)e.x.off});
  e.reuse = a->reuse_memory_side != 0 && e.sig == c->grad.sig;
  e.x.real_pass(w.ws.as<char>(), e.reuse);
  return CFD_OK;
}

// Everything the launch sequence and its (by-value) kernel arguments depend on, the timestep excepted (its row is staged).
static void build_graph_key(WegEval& e) {
  const WegState& w = e.c->weg;
  e.key = {e.B, e.L, e.a->last, e.nt_max, w.tok_version, (long long)(size_t)w.tok.p, (long long)(size_t)e.io, (long long)e.lay.n_io,
           (long long)(size_t)e.arena, (long long)e.reuse, (long long)e.use_rt, (long long)(e.use_rt ? e.c->grad.rt.T : 0)};
  rtgrad::append_memories(e.key, e.a->mem);
  for (int k = 0; k < 3; ++k) { long long bits = 0; memcpy(&bits, &e.a->kernel3[k], 4); e.key.push_back(bits); }
}

// The evaluation's launches (this is what a graph captures).
static int enqueue_eval(WegEval& e) {
  if (e.use_rt) CHK(wegrt::enqueue(e.c, e.st, !e.reuse, e.args));
  else weg::run(e.x, e.args);
  return CFD_OK;
}

// One graph variant's life: a new key drops the graph of the old one; a key runs eagerly at its first use, is captured and
// instantiated at its second, and replayed from then on.
static int run_through_graph(WegEval& e, WegState::Graph& g) {
  hipStream_t st = e.st;
  if (g.key != e.key) g.reset(e.key);
  const bool on = e.c->weg_graph_on;
  if (on && g.gx.exec) {
    HIPCHK(hipGraphLaunch(g.gx.exec, st));
  } else if (on && g.uses >= 1) {
    g.gx.reset();   // (a graph whose instantiation failed last time)
    HIPCHK(hipStreamBeginCapture(st, hipStreamCaptureModeThreadLocal));
    const int rr = enqueue_eval(e);
    hipError_t err = hipStreamEndCapture(st, &g.gx.graph);
    if (rr != CFD_OK) { g.gx.reset(); return rr; }
    if (err != hipSuccess) return fail(CFD_E_HIP, "capturing the WEG evaluation failed: %s", hipGetErrorString(err));
    HIPCHK(hipGraphInstantiate(&g.gx.exec, g.gx.graph, nullptr, nullptr, 0));
    HIPCHK(hipGraphLaunch(g.gx.exec, st));
  } else {
    CHK(enqueue_eval(e));
  }
  ++g.uses;
  HIPCHK(hipGetLastError());
  return CFD_OK;
}

// Eagerly under the stop hook -- neither a use of a graph key nor a change of one -- and through the variant's graph otherwise.
static int run(WegEval& e) {
  GradState& g = e.c->grad;
  g.sig.clear();                                  // (an evaluation that fails leaves nothing to reuse; on the engine begin_call has cleared it already)
  if (g.rt.stop) {
    CHK(enqueue_eval(e));
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(e.st));
  } else {
    CHK(run_through_graph(e, e.c->weg.graph[e.reuse ? 1 : 0]));
  }
  g.sig = e.sig;
  return CFD_OK;
}

// Results to the caller; with loss_host the call waits and reads its census, without it the caller's stream continues behind the evaluation.
static int deliver(WegEval& e, float* losses, float* max_att, float* grad, float* loss_host) {
  Ctx* c = e.c;
  const WegStaging& y = e.lay;
  const int B = e.B;
  HIPCHK(hipMemcpyAsync(losses, e.io + y.o_loss, (size_t)B * 4, hipMemcpyDeviceToDevice, e.st));
  HIPCHK(hipMemcpyAsync(max_att, e.io + y.o_max, y.n_max * 4, hipMemcpyDeviceToDevice, e.st));
  HIPCHK(hipMemcpyAsync(grad, e.io + y.o_grad, y.n_lat * 4, hipMemcpyDeviceToDevice, e.st));
  if (loss_host) {                                   // torch.mean(losses) over the batch (word_excitation_guidance.py:80)
    std::vector<float> l(B);
    HIPCHK(hipMemcpyAsync(l.data(), e.io + y.o_loss, (size_t)B * 4, hipMemcpyDeviceToHost, e.st));
    HIPCHK(hipStreamSynchronize(e.st));
    CHK(check_saturation(c, "cfd_weg_eval (latents, memories / their projections)"));   // (without loss_host: read by the next call that waits on this handle)
    float sum = 0.f;
    for (int b = 0; b < B; ++b) sum += l[b];
    *loss_host = sum / (float)B;
  } else {
    c->census_pending = true;                        // (read by the handle's next entry point: settle_deferred_census)
    HIPCHK(hipEventRecord(c->grad.ev, e.st));
    HIPCHK(hipStreamWaitEvent(e.caller, c->grad.ev, 0));
  }
  return CFD_OK;
}

extern "C" int cfd_weg_eval(cfd_handle c, const cfd_weg_args* a, float* losses, float* max_att, float* grad, float* loss_host, void* stream) {
  int nt_max = 0;
  CHK(check_args(c, a, losses, max_att, grad, &nt_max));
  HIPCHK(hipSetDevice(c->cfg.device));
  const int D = c->cfg.text_encoded_dim, n_tok = a->tok_off[a->B];
  WegEval e{c, a, (hipStream_t)stream, c->own_stream, a->B, a->L, D, n_tok, nt_max, WegStaging(a->B, a->L, D, n_tok)};
  CHK(begin(e));
  CHK(upload_focus_tokens(e));
  CHK(stage_inputs(e));
  if (!e.use_rt) CHK(size_f32_sequence_and_reuse(e));
  build_graph_key(e);
  CHK(run(e));
  if (c->grad.rt.stop) return CFD_OK;               // test hook: losses / max_att / grad are not delivered, the sweep was left early
  return deliver(e, losses, max_att, grad, loss_host);
}

// ---- cfd_weg_step: every row its own utterance, evaluation and gated update in one call (row-tile gradient engine only) --------------
struct WegStep {   // one call, handed from stage to stage
  Ctx* c;
  const cfd_weg_rows_args* a;
  hipStream_t caller, st;
  int B, L, n_tok, nt_max = 1, last_max = 0;
  float *xin = nullptr, *g = nullptr, *step = nullptr;   // WegState::rows
};

// What a table of per-row slices and focus tokens must satisfy (cfd_weg_step and the focus kernels' test hook): offsets ascending from
// 0, every slice at least 2 wide and inside the St keys, every focus index inside its own row's slice.  Yields the most focus tokens of
// a row and the widest slice's end.
static int check_row_tables(const char* who, int B, int St, const int32_t* tok_off, const int32_t* tok_idx, const int32_t* last_rows, int* nt_max_out,
                            int* last_max_out) {
  const int n_tok = tok_off[B];
  if (tok_off[0] != 0 || n_tok < 0 || (n_tok > 0 && !tok_idx)) return fail(CFD_E_ARG, "%s: bad focus-token table", who);
  int nt_max = 1, last_max = 0;
  for (int b = 0; b < B; ++b) {
    if (tok_off[b + 1] < tok_off[b] || tok_off[b + 1] > n_tok) return fail(CFD_E_ARG, "%s: bad focus-token table", who);
    const int last = last_rows[b];
    // F.pad(..., mode='reflect') with pad 1 needs at least 2 entries per axis (word_excitation_guidance.py:35)
    if (last - 1 < 2 || last > St)
      return fail(CFD_E_SHAPE, "%s: row %d: text slice [1, %d) of %d keys is too short for the 3x3 reflect-padded smoothing", who, b, last, St);
    for (int t = tok_off[b]; t < tok_off[b + 1]; ++t)
      if (tok_idx[t] < 1 || tok_idx[t] > last - 1)
        return fail(CFD_E_ARG, "%s: row %d: focus index %d is outside the row's text slice [1, %d)", who, b, tok_idx[t], last);
    nt_max = std::max(nt_max, tok_off[b + 1] - tok_off[b]);
    last_max = std::max(last_max, last);
  }
  *nt_max_out = nt_max;
  *last_max_out = last_max;
  return CFD_OK;
}

// Every refusal, before anything is touched.
static int check_step_args(Ctx* c, const cfd_weg_rows_args* a, const float* losses, const float* max_att, int* nt_max, int* last_max) {
  if (!c || !a || !a->latents || !a->tok_off || !a->last_rows || !losses || !max_att) return fail(CFD_E_ARG, "cfd_weg_step: null argument");
  CHK(check_latent_call(c, a->B, a->L, a->mem, CALL_TIMESTEP, a->timestep));   // (one memory per row: no row maps)
  if (c->cfg.text_encoded_dim > 2048) return fail(CFD_E_SHAPE, "model width above 2048");
  if (const char* why = rtgrad::ineligible(c, a->B, a->L, a->mem)) return fail(CFD_E_ARG, "cfd_weg_step runs on the row-tile gradient engine only: %s", why);
  if ((a->tie != nullptr) != (a->tie_csr != nullptr)) return fail(CFD_E_ARG, "cfd_weg_step: tie and tie_csr go together (cfd_guide_tie_csr)");
  if (a->reuse_memory_side < 0 || a->reuse_memory_side > 2) return fail(CFD_E_ARG, "cfd_weg_step: reuse_memory_side = %d is not 0, 1 or 2", a->reuse_memory_side);
  if (c->grad.rt.stop) return fail(CFD_E_STATE, "cfd_debug_weg_stop is set: cfd_weg_step runs its whole launch sequence");
  const int St = a->mem[2].S;
  CHK(check_row_tables("cfd_weg_step", a->B, St, a->tok_off, a->tok_idx, a->last_rows, nt_max, last_max));
  // the general focus kernel's workspace blocks must fit what the arena sets aside for them (rt_grad.hpp, prepare: fws)
  if (!wegrt::focus_small(a->L, *last_max, *nt_max) && 3ll * a->L * (*last_max - 1) + 3ll * *nt_max > 3ll * a->L * St + 3ll * St + 64)
    return fail(CFD_E_ARG, "cfd_weg_step: %d focus tokens in one row exceed the objective's workspace", *nt_max);
  return CFD_OK;
}

// offsets | indices | last_rows to the device when they change (the stream may still read the old copy)
static int upload_row_tables(Ctx* c, hipStream_t st, int B, const int32_t* tok_off, const int32_t* tok_idx, const int32_t* last_rows, const int32_t** off_dev,
                             const int32_t** idx_dev, const int32_t** last_dev) {
  WegState& w = c->weg;
  const int n_idx = std::max(1, tok_off[B]);
  std::vector<int32_t> tok(tok_off, tok_off + B + 1);
  for (int t = 0; t < n_idx; ++t) tok.push_back(t < tok_off[B] ? tok_idx[t] : 0);
  tok.insert(tok.end(), last_rows, last_rows + B);
  if (tok != w.tok_host) {
    HIPCHK(hipStreamSynchronize(st));
    w.tok_host.clear();
    CHK(w.tok.ensure(tok.size() * 4));
    HIPCHK(hipMemcpy(w.tok.p, tok.data(), tok.size() * 4, hipMemcpyHostToDevice));
    w.tok_host = tok;
    ++w.tok_version;
  }
  *off_dev = w.tok.as<int32_t>();
  *idx_dev = *off_dev + B + 1;
  *last_dev = *idx_dev + n_idx;
  return CFD_OK;
}

// Room for x~ | g~ | the rows' steps, and the steps on their way to the device (null row_step: no copy, the update takes every step as 0).
static int stage_step(WegStep& e) {
  WegState& w = e.c->weg;
  CHK(carve(w.rows, 64, [&](ArenaLayout& l) {
    l.take(e.xin, (size_t)e.n_tok * CFD_LAT); l.take(e.g, (size_t)e.n_tok * CFD_LAT); l.take(e.step, (size_t)e.B);
  }));
  if (!e.a->row_step) { e.step = nullptr; return CFD_OK; }
  HIPCHK(hipStreamSynchronize(e.st));   // (the previous call's copy may still read step_host)
  w.step_host.assign(e.a->row_step, e.a->row_step + e.B);
  HIPCHK(hipMemcpyAsync(e.step, w.step_host.data(), (size_t)e.B * 4, hipMemcpyHostToDevice, e.st));
  return CFD_OK;
}

extern "C" int cfd_weg_step(cfd_handle c, const cfd_weg_rows_args* a, float* losses, float* max_att, float* grad, float* x_new, float* losses_host,
                            void* stream) {
  int nt_max = 1, last_max = 0;
  CHK(check_step_args(c, a, losses, max_att, &nt_max, &last_max));
  HIPCHK(hipSetDevice(c->cfg.device));
  WegStep e{c, a, (hipStream_t)stream, c->own_stream, a->B, a->L, a->B * a->L, nt_max, last_max};
  rtgrad::Call k{rtgrad::FOR_WEG, a->B, a->L, a->mem, nullptr, {}, a->reuse_memory_side, a->timestep};
  CHK(rtgrad::begin_call(c, k, e.caller));
  const int32_t *off_dev, *idx_dev, *last_dev;
  CHK(upload_row_tables(c, e.st, e.B, a->tok_off, a->tok_idx, a->last_rows, &off_dev, &idx_dev, &last_dev));
  CHK(stage_step(e));
  weg::Args args{a->latents, nullptr, a->mem, off_dev, idx_dev, last_max, nt_max, {a->kernel3[0], a->kernel3[1], a->kernel3[2]}, losses, max_att, e.g, last_dev};
  const int r = wegrt::enqueue_step(c, e.st, !k.reuse, args, e.xin, e.step, a->tie, a->tie_csr, grad, x_new);
  if (r != CFD_OK) {                                 // (whatever was enqueued still reads the caller's buffers)
    (void)hipStreamSynchronize(e.st);
    return r;
  }
  if (losses_host) {
    HIPCHK(hipMemcpyAsync(losses_host, losses, (size_t)e.B * 4, hipMemcpyDeviceToHost, e.st));
    HIPCHK(hipStreamSynchronize(e.st));
    CHK(check_saturation(c, "cfd_weg_step (latents, memories / their projections)"));
  } else {
    c->census_pending = true;                        // (read by the handle's next entry point: settle_deferred_census)
    HIPCHK(hipEventRecord(c->grad.ev, e.st));
    HIPCHK(hipStreamWaitEvent(e.caller, c->grad.ev, 0));
  }
  c->grad.sig = k.sig;
  return CFD_OK;
}

// ---- developer hook: one launch of a focus kernel as cfd_weg_step launches it (include/cfdenoise_dev.h) ------------------------------
extern "C" int cfd_test_weg_focus_rows(cfd_handle c, const float* att, int B, int NL, int L, int S, const int32_t* tok_off, const int32_t* tok_idx,
                                       const int32_t* last_rows, int last, int nt_max, const float kernel3[3], int per_row, int small, float* workspace,
                                       float* losses, float* max_att, float* d_att, void* stream) {
  if (!c || !att || !tok_off || !kernel3 || !workspace || !losses || !max_att || !d_att || B < 1 || NL < 1 || L < 2)
    return fail(CFD_E_ARG, "cfd_test_weg_focus_rows: bad argument");
  std::vector<int32_t> lasts(last_rows ? last_rows : &last, last_rows ? last_rows + B : &last + 1);
  lasts.resize((size_t)B, last);
  int nt_need = 1, last_max = 0;
  CHK(check_row_tables("cfd_test_weg_focus_rows", B, S, tok_off, tok_idx, lasts.data(), &nt_need, &last_max));
  if (last_max > last || nt_need > nt_max) return fail(CFD_E_ARG, "cfd_test_weg_focus_rows: last = %d / nt_max = %d do not cover the rows (%d / %d)", last, nt_max, last_max, nt_need);
  if (small && !wegrt::focus_small(L, last, nt_max)) return fail(CFD_E_ARG, "cfd_test_weg_focus_rows: the shape does not fit weg_focus_small_kernel");
  HIPCHK(hipSetDevice(c->cfg.device));
  hipStream_t st = (hipStream_t)stream;
  const int n_idx = std::max(1, tok_off[B]);
  std::vector<int32_t> tok(tok_off, tok_off + B + 1);
  for (int t = 0; t < n_idx; ++t) tok.push_back(t < tok_off[B] ? tok_idx[t] : 0);
  tok.insert(tok.end(), lasts.begin(), lasts.end());
  DBuf tab;
  CHK(tab.ensure(tok.size() * 4));
  HIPCHK(hipMemcpy(tab.p, tok.data(), tok.size() * 4, hipMemcpyHostToDevice));
  const int32_t *off_dev = tab.as<int32_t>(), *idx_dev = off_dev + B + 1, *last_dev = last_rows ? idx_dev + n_idx : nullptr;
  const int grad_rows = per_row ? 1 : B;
  if (small)
    hipLaunchKernelGGL(weg_focus_small_kernel<>, dim3((unsigned)B), dim3(256), 0, st, att, off_dev, idx_dev, B, NL, L, S, last, kernel3[0], kernel3[1],
                       kernel3[2], losses, max_att, d_att, last_dev, grad_rows);
  else
    hipLaunchKernelGGL(weg_focus_kernel<>, dim3((unsigned)B), dim3(256), 0, st, att, off_dev, idx_dev, B, NL, L, S, last, nt_max, kernel3[0], kernel3[1],
                       kernel3[2], workspace, losses, max_att, d_att, last_dev, grad_rows);
  HIPCHK(hipGetLastError());
  HIPCHK(hipStreamSynchronize(st));   // (tab leaves scope)
  return CFD_OK;
}
