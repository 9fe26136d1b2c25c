// libcfdenoise: the sampling loop -- scheduler coefficients, the captured iteration, cfd_sample_* / cfd_dyadic_steps -- and the stand-alone
// scheduler / RNG entry points.
#include "cfd_internal.hpp"

// ---- scheduler coefficients: diffusers 0.14.0 DDPMScheduler.step / DDIMScheduler.step, float32 ----------
static void ddpm_coef(const float* ac, int T, int n_inf, int t, StepCoef* o) {
  const int prev_t = t - T / n_inf;
  const float ap_t = ac[t];
  const float ap_prev = prev_t >= 0 ? ac[prev_t] : 1.0f;
  const float bp_t = 1.0f - ap_t, bp_prev = 1.0f - ap_prev;
  const float cur_alpha = ap_t / ap_prev;
  const float cur_beta = 1.0f - cur_alpha;
  o->sb = sqrtf(bp_t);
  o->sa = sqrtf(ap_t);
  o->c0 = (sqrtf(ap_prev) * cur_beta) / bp_t;
  o->cx = sqrtf(cur_alpha) * bp_prev / bp_t;
  float var = bp_prev / bp_t * cur_beta;
  if (var < 1e-20f) var = 1e-20f;
  o->sigma = t > 0 ? sqrtf(var) : 0.0f;
  o->use_noise = t > 0 ? 1.0f : 0.0f;
  o->order = o->r0inv = 0.f;
}
static void ddim_coef(const float* ac, int T, int n_inf, int t, float eta, int set_alpha_to_one, StepCoef* o) {
  const int prev_t = t - T / n_inf;
  const float ap_t = ac[t];
  const float ap_prev = prev_t >= 0 ? ac[prev_t] : (set_alpha_to_one ? 1.0f : ac[0]);
  const float bp_t = 1.0f - ap_t, bp_prev = 1.0f - ap_prev;
  const float var = (bp_prev / bp_t) * (1.0f - ap_t / ap_prev);
  const float std = eta * sqrtf(var);
  o->sb = sqrtf(bp_t);
  o->sa = sqrtf(ap_t);
  o->c0 = sqrtf(ap_prev);
  o->cx = sqrtf(1.0f - ap_prev - std * std);
  o->sigma = std;
  o->use_noise = eta > 0.f ? 1.0f : 0.0f;
  o->order = o->r0inv = 0.f;
}

// DDIM inversion (prompt-to-prompt's next_step, scheduler kind 3): the step at t moves from t_cur = t - T // n_inf to t.  Kind 1's row
// shape: sa / sb from a_cur (x0 = (x - sb eps) / sa), c0 / cx from a_nxt (x = c0 x0 + cx eps); deterministic (no eta, no noise).
static void ddim_inverse_coef(const float* ac, int T, int n_inf, int t, int set_alpha_to_one, StepCoef* o) {
  const int t_cur = t - T / n_inf;
  const float a_cur = t_cur >= 0 ? ac[t_cur] : (set_alpha_to_one ? 1.0f : ac[0]);
  const float a_nxt = ac[t];
  o->sb = sqrtf(1.0f - a_cur);
  o->sa = sqrtf(a_cur);
  o->c0 = sqrtf(a_nxt);
  o->cx = sqrtf(1.0f - a_nxt);
  o->sigma = 0.f;
  o->use_noise = 0.f;
  o->order = o->r0inv = 0.f;
}

// diffusers 0.14.0 DPMSolverMultistepScheduler (dpmsolver++, solver_order 2, midpoint, lower_order_final), float32 as its torch tables:
// alpha_t = sqrt(abar), sigma_t = sqrt(1 - abar), lambda_t = log(alpha_t) - log(sigma_t).  Step at t towards prev_t; t_prev_model = the
// timestep of the previous step's model output (its x0 is the history m1), or -1 for a first-order step.
static float dpmpp_lambda(const float* ac, int t) { return logf(sqrtf(ac[t])) - logf(sqrtf(1.0f - ac[t])); }
static void dpmpp_coef(const float* ac, int t, int prev_t, int t_prev_model, StepCoef* o) {
  const float lam_t = dpmpp_lambda(ac, prev_t), lam_s0 = dpmpp_lambda(ac, t);
  const float h = lam_t - lam_s0;
  o->sb = sqrtf(1.0f - ac[t]);
  o->sa = sqrtf(ac[t]);
  o->c0 = sqrtf(1.0f - ac[prev_t]) / o->sb;
  o->cx = sqrtf(ac[prev_t]) * (expf(-h) - 1.0f);
  o->sigma = 0.f;
  o->use_noise = 0.f;
  if (t_prev_model >= 0) {
    const float h_0 = lam_s0 - dpmpp_lambda(ac, t_prev_model);
    const float r0 = h_0 / h;
    o->r0inv = 1.0f / r0;
    o->order = 2.f;
  } else {
    o->r0inv = 0.f;
    o->order = 1.f;
  }
}

// The per-iteration coefficient rows of a loop over the timestep table ts[0..N) (what cfd_sample_begin uploads).  Kind 2 needs the table
// strictly decreasing in [1, T): the first executed iteration k0 is first order (diffusers' lower_order_nums is 0 there: no history), the
// last one too when N < 15 (lower_order_final, from the full table's length), all others second order.  Kind 3 (DDIM inversion) needs the
// table strictly increasing.
static int step_coefficients(int kind, const float* ac, int T, int n_inf, const int32_t* ts, int N, float eta, int set_alpha_to_one,
                             StepCoef* coef, int k0 = 0) {
  for (int i = 0; i < N; ++i) {
    const int t = ts[i];
    if (t < 0 || t >= T) return fail(CFD_E_ARG, "timestep %d out of range", t);
    memset(&coef[i], 0, sizeof(StepCoef));
    if (kind == 0) ddpm_coef(ac, T, n_inf, t, &coef[i]);
    else if (kind == 1) ddim_coef(ac, T, n_inf, t, eta, set_alpha_to_one, &coef[i]);
    else if (kind == 3) {
      if (i > 0 && t <= ts[i - 1])
        return fail(CFD_E_ARG, "DDIM inversion: the timestep table must increase strictly (entry %d is %d after %d)", i, t, ts[i - 1]);
      ddim_inverse_coef(ac, T, n_inf, t, set_alpha_to_one, &coef[i]);
    } else {
      if (t < 1 || (i > 0 && t >= ts[i - 1]))
        return fail(CFD_E_ARG, "DPM-Solver++: the timestep table must decrease strictly and stay in [1, %d) (entry %d is %d)", T, i, t);
      const bool first = i <= k0 || (i == N - 1 && N < 15);
      dpmpp_coef(ac, t, i + 1 < N ? ts[i + 1] : 0, first ? -1 : ts[i - 1], &coef[i]);
    }
  }
  return CFD_OK;
}

// f(PRED) for the stand-alone step kernels: prediction_type 1 ("sample") is PRED 1, everything else PRED 0 (the callers refuse other values)
template <class F>
static void with_pred(int prediction_type, F&& f) { prediction_type == 1 ? f(std::integral_constant<int, 1>{}) : f(std::integral_constant<int, 0>{}); }

// An instance of cfg_step_kernel and its arguments, cut from the weighted instance's (and the trajectory ring)
template <bool WTAB, bool TRAJ, int PRED>
struct StepInst {
  static constexpr auto kernel = cfg_step_kernel<0, WTAB, TRAJ, PRED>;
  static CfgStepArgsOf<WTAB, TRAJ> args(const CfgStepArgsW& cw, float* traj) {
    CfgStepArgsOf<WTAB, TRAJ> a;
    static_cast<CfgStepArgsOf<WTAB, false>&>(a) = cw;   // (the default instance takes its CfgStepArgs part)
    if constexpr (TRAJ) a.traj = traj;
    return a;
  }
};
// The one place that maps (weighted, trajectory, prediction_type) to an instance of cfg_step_kernel, f(StepInst<>{}, its name in a launch
// error): six of them -- prediction_type 1 ("sample": the combine is x0) has no trajectory instance, inversion refuses the type
// (check_run_args); traj: an inversion run recording its trajectory, the step also stores into slot *d_step + 1.
template <class F>
static int with_step_inst(bool weighted, bool traj, int prediction_type, F&& f) {
  if (prediction_type == 1)
    return weighted ? f(StepInst<true, false, 1>{}, "cfg_step_kernel_weighted_x0") : f(StepInst<false, false, 1>{}, "cfg_step_kernel_x0");
  if (traj) return weighted ? f(StepInst<true, true, 0>{}, "cfg_step_kernel_weighted_traj") : f(StepInst<false, true, 0>{}, "cfg_step_kernel_traj");
  return weighted ? f(StepInst<true, false, 0>{}, "cfg_step_kernel_weighted") : f(StepInst<false, false, 0>{}, "cfg_step_kernel<>");
}

// The instances of begin_step_kernel / inpaint_now_kernel that take the argument struct Args (rows.hpp: BeginArgsOf, the other way round)
template <class Args>
struct BeginInst {
  static constexpr bool EDIT = std::is_base_of<BeginArgsE, Args>::value, ANCHOR = std::is_same<Args, BeginArgsA>::value,
                        TIE = std::is_same<Args, BeginArgsT>::value;
  static_assert(std::is_same<Args, BeginArgsOf<EDIT, ANCHOR, TIE>>::value, "not an argument struct of begin_step_kernel");
  static constexpr auto begin_step = begin_step_kernel<0, EDIT, ANCHOR, TIE>;
  static constexpr auto inpaint_now = inpaint_now_kernel<0, EDIT, ANCHOR, TIE>;
};

// What every instance's arguments start with (preseq / inoise / pl are the default instance's alone: default_begin_args)
static BeginArgs base_begin_args(Ctx* c) {
  const cfd_sample_args& s = c->run.args;
  return BeginArgs{c->run.latents.as<float>(), c->w->sample_sp.as<char>(), s.B, s.L, s.G, nullptr, nullptr, 0, c->run.coef.as<StepCoef>(),
                   c->w->d_step.as<int>()};
}

static BeginArgs default_begin_args(Ctx* c) {
  BeginArgs ba = base_begin_args(c);
  ba.preseq = c->run.args.preseq;
  ba.inoise = c->run.inoise.as<float>();
  ba.pl = c->run.args.preseq_len;
  return ba;
}

static BeginArgsE edit_begin_args(Ctx* c) {
  BeginArgsE be;
  static_cast<BeginArgs&>(be) = base_begin_args(c);
  be.keep = c->run.ekeep.as<uint8_t>();
  be.src = c->run.esrc.as<float>();
  be.eps = c->run.enoise.as<float>();
  return be;
}

static BeginArgsT tied_begin_args(Ctx* c) {
  BeginArgsT bt;
  static_cast<BeginArgsE&>(bt) = edit_begin_args(c);
  bt.tie = c->run.etie.as<int32_t>();
  return bt;
}

static BeginArgsA anchor_begin_args(Ctx* c) {
  BeginArgsA ba;
  static_cast<BeginArgs&>(ba) = base_begin_args(c);
  ba.keep = c->run.ekeep.as<uint8_t>();
  ba.ring = c->run.mode.anchor_ring;
  ba.slot = (long long)c->run.args.B * c->run.args.L * CFD_LAT;
  ba.n = c->run.mode.anchor_n;
  return ba;
}

// Which overwrite the open run does at the start of an iteration: f(that instance's arguments), the instance being BeginInst<> of their
// type.  The one place that maps RunMode to an instance of begin_step_kernel / inpaint_now_kernel.
template <class F>
static int with_begin_args(Ctx* c, F&& f) {
  if (c->run.mode.tie) return f(tied_begin_args(c));      // the tied and the kept tokens
  if (c->run.mode.edit) return f(edit_begin_args(c));     // the kept tokens, re-noised from the source
  if (c->run.mode.anchor) return f(anchor_begin_args(c)); // the kept tokens, from the trajectory
  return f(default_begin_args(c));                   // the first preseq_len tokens, if the run has a preseq
}

static int enqueue_loop_iteration(Ctx* c, hipStream_t st) {
  const cfd_sample_args& s = c->run.args;
  const RunMode& m = c->run.mode;
  const long long n8 = (long long)s.B * s.L * (CFD_LAT / 8);
  CHK(with_begin_args(c, [&](auto a) {
    using I = BeginInst<decltype(a)>;
    LAUNCH(CFD_PROF_OTHER, I::begin_step, dim3((unsigned)((n8 + 255) / 256)), dim3(256), st, a);
    return (int)CFD_OK;
  }));
  CHK(enqueue_denoise(c, st));
  CfgStepArgsW cw;
  memset(&cw, 0, sizeof(cw));
  cw.eps = c->w->eps.as<float>(); cw.latents = c->run.latents.as<float>(); cw.B = s.B; cw.L = s.L; cw.G = s.G;
  for (int k = 0; k < 8; ++k) { cw.w[k] = s.guidance_weight[k]; cw.pos[k] = c->run.chunk_pos[k]; }
  cw.kind = s.scheduler; cw.clip = s.clip_sample; cw.hist = c->run.hist.as<float>(); cw.coef = c->run.coef.as<StepCoef>(); cw.d_step = c->w->d_step.as<int>();
  cw.noise = s.step_noise; cw.seed = s.seed; cw.utt0 = s.first_utterance;
  cw.advance = c->w->d_step.as<int>();   // the last workgroup of cfg_step_kernel advances the loop index
  if (m.weighted) {   // the caller's 7 chunks, weights from the run's table (those of a chunk it does not evaluate are all 0)
    cw.G = 7;
    for (int k = 0; k < 8; ++k) cw.pos[k] = c->run.wpos[k];
    cw.wtab = c->run.wtab.as<float>();
  }
  const long long n4 = (long long)s.B * s.L * CFD_LAT / 4;
  const dim3 grid((unsigned)std::min<long long>((n4 + 255) / 256, 256)), block(256);
  return with_step_inst(m.weighted, m.traj != nullptr, s.prediction_type, [&](auto inst, const char* name) {
    LAUNCH_AS(CFD_PROF_OTHER, name, inst.kernel, grid, block, st, inst.args(cw, m.traj));
    return (int)CFD_OK;
  });
}

// What every set-up starts with: the device, no forward hints, the census an earlier call deferred
static int setup_preamble(Ctx* c) {
  HIPCHK(hipSetDevice(c->cfg.device));
  c->hint_now = c->hint_same_mem = false;
  return settle_deferred_census(c);
}

// The refusals about the scheduler's tables that do not depend on the kind of run (`who`: the entry point, for the message)
static int check_scheduler_tables(const cfd_sample_args& s, const char* who) {
  if (!s.alphas_cumprod || s.num_train_timesteps < 1 || s.num_inference_steps < 1 || s.num_inference_steps > s.num_train_timesteps)
    return fail(CFD_E_ARG, "bad scheduler tables");
  if (s.timesteps && (s.num_timesteps < 1 || s.num_timesteps > s.num_train_timesteps)) return fail(CFD_E_ARG, "bad num_timesteps");
  if (!s.timesteps && s.scheduler == 0 && s.num_train_timesteps % s.num_inference_steps)
    return fail(CFD_E_ARG, "%s: DDPM: num_inference_steps = %d does not divide num_train_timesteps = %d: the loop's timestep table for such "
                           "counts differs between diffusers releases (unpinned); pass the scheduler's table in cfd_sample_args.timesteps",
                who, s.num_inference_steps, s.num_train_timesteps);
  return CFD_OK;
}

// skip_zero_weight_chunks: the batch is chunk-major, so dropping trailing zero-weight chunks = using the first G' * B rows (c->run.args.G)
static void trim_zero_weight_chunks(Ctx* c, const cfd_sample_args& s) {
  if (s.skip_zero_weight_chunks)
    while (c->run.args.G > 1 && s.guidance_weight[c->run.args.G - 1] == 0.0f) c->run.args.G -= 1;
}

// The tables of a run over N iterations, on the stream: the timestep table (the caller's, or (arange(N) * (T // n_inf)).round()[::-1],
// + steps_offset for DDIM), its step coefficients (k0: the first executed iteration), the step index cleared, the saturation census
// opened (what the caller reads next counts THIS call's launches only), the time tables and the memories' once-per-run work; then the one
// wait (the host tables go out of scope).  coef_out: the coefficient rows for a caller that reads them on the host.
static int upload_run_tables(Ctx* c, const cfd_sample_args& s, int N, int k0, hipStream_t st, std::vector<StepCoef>* coef_out = nullptr) {
  const int n_inf = s.num_inference_steps, T = s.num_train_timesteps, ratio = T / n_inf;
  std::vector<int32_t> ts(N);
  std::vector<StepCoef> coef(N);
  for (int i = 0; i < N; ++i) ts[i] = s.timesteps ? s.timesteps[i] : (N - 1 - i) * ratio + (s.scheduler == 1 ? s.steps_offset : 0);
  CHK(step_coefficients(s.scheduler, s.alphas_cumprod, T, n_inf, ts.data(), N, s.eta, s.set_alpha_to_one, coef.data(), k0));
  CHK(c->run.coef.ensure((size_t)N * sizeof(StepCoef)));
  HIPCHK(hipMemcpyAsync(c->run.coef.p, coef.data(), (size_t)N * sizeof(StepCoef), hipMemcpyHostToDevice, st));
  HIPCHK(hipMemsetAsync(c->w->d_step.p, 0, 16, st));
  CHK(sat_begin(c, st));
  CHK(build_time_tables(c, ts.data(), N, st));   // (a run over the same table finds them built)
  CHK(prepare_static_memside(c, st));
  HIPCHK(hipStreamSynchronize(st));
  if (coef_out) coef_out->swap(coef);
  return CFD_OK;
}

// Chunks of a weighted run (cfd_sample_begin_weighted): uploads the weight table, decides which chunks are evaluated (prune: every chunk
// k >= 1 whose column is 0 throughout is not, except the last one when the run keeps its attention maps) and compacts the host copy of
// the memories' row maps (G * B entries each) to the evaluated chunks, in the caller's order.  keep_idx[k]: the compacted index of chunk
// k, or -1.  c->run.args.G becomes the number of evaluated chunks.
static int weighted_chunks(Ctx* c, const float* wtab, int prune, int N, bool keep_last, HostMaps& hm, int keep_idx[8], hipStream_t st) {
  const cfd_sample_args& s = c->run.args;
  const int B = s.B, G = s.G;
  const size_t n = (size_t)N * B * 8;
  for (size_t e = 0; e < n; ++e)
    if (e % 8 != 0 && !std::isfinite(wtab[e]))
      return fail(CFD_E_ARG, "weights[%zu][%zu][%zu] is not finite", e / 8 / B, e / 8 % B, e % 8);
  bool keep[8] = {true, false, false, false, false, false, false, false};
  for (int k = 1; k < G; ++k) {
    keep[k] = !prune || (keep_last && k == G - 1);
    for (size_t r = 0; r < (size_t)N * B && !keep[k]; ++r) keep[k] = wtab[r * 8 + k] != 0.0f;
  }
  int ge = 0;
  for (int k = 0; k < 8; ++k) keep_idx[k] = (k < G && keep[k]) ? ge++ : -1;
  CHK(c->run.wtab.ensure(n * sizeof(float)));
  HIPCHK(hipMemcpyAsync(c->run.wtab.p, wtab, n * sizeof(float), hipMemcpyHostToDevice, st));
  HIPCHK(hipStreamSynchronize(st));   // (the caller's host table is not kept beyond the call)
  c->run.args.G = ge;
  if (ge == G) return CFD_OK;
  for (std::vector<int>& m : hm.m) {   // (keep_idx[k] <= k: in place)
    for (int k = 0; k < G; ++k)
      if (keep_idx[k] >= 0)
        for (int u = 0; u < B; ++u) m[(size_t)keep_idx[k] * B + u] = m[(size_t)k * B + u];
    m.resize((size_t)ge * B);
  }
  return CFD_OK;
}

// The run's keep mask on the device: the validated host copy (the caller waits for the stream before hkeep goes out of scope), or,
// with an empty hkeep (no mask given), no kept token.
static int upload_keep_mask(Ctx* c, const std::vector<uint8_t>& hkeep, size_t n, hipStream_t st) {
  CHK(c->run.ekeep.ensure(n));
  if (!hkeep.empty()) HIPCHK(hipMemcpyAsync(c->run.ekeep.p, hkeep.data(), n, hipMemcpyHostToDevice, st));
  else HIPCHK(hipMemsetAsync(c->run.ekeep.p, 0, n, st));
  return CFD_OK;
}

// What an opener adds to cfd_sample_begin's run; every field is optional.  weights (with prune / chunks_evaluated as in
// cfd_sample_begin_weighted; NULL: the default guidance weights, chunks_evaluated then gets the run's G on success), edit, traj (the
// inversion's trajectory ring), anchor, tie, replay (a DDPM noise space: the anchored instance over its trajectory, a start at its
// first_iteration).  A new run kind touches: its field here, its RunMode field (cfd_internal.hpp), its block in init_latents_and_kind,
// which turns the one into the other, and -- if it overwrites tokens at the start of an iteration -- its row in with_begin_args and its
// branch in BOTH begin_step_kernel and inpaint_now_kernel (rows.hpp).  What it refuses goes into its opener, or into
// check_run_args where it depends on the other fields; a host table it brings is fetched next to fetch_keep_mask / fetch_tie_table.
struct BeginExt {
  const char* opener = "cfd_sample_begin";
  const float* weights = nullptr;
  int prune = 0;
  int* chunks_evaluated = nullptr;
  const cfd_edit_args* edit = nullptr;
  float* traj = nullptr;
  const cfd_anchor_args* anchor = nullptr;
  const cfd_tie_args* tie = nullptr;
  const cfd_replay_args* replay = nullptr;
};

// What the stages of sample_begin hand to each other
struct BeginState {
  Ctx* c;
  const cfd_sample_args& s;   // the caller's arguments (c->run.args: the run's copy, G = the evaluated chunks, no host pointers)
  const BeginExt& x;
  hipStream_t st;
  int N;                      // loop iterations (the length of scheduler.timesteps)
  int k0;                     // the first executed iteration (an edit's or a replay's first_iteration)
  int n_ring = 0;             // attention rings given (0 or CFD_NMEM)
  size_t lat_bytes;
  std::vector<uint8_t> hkeep; // the keep mask and the tie table on the host, validated (empty: none given)
  std::vector<int32_t> htie;
  cfd_memory mem_in[CFD_NMEM];
  HostMaps hm;                // the memories' row maps on the host: fetched once (select_chunks), compacted and permuted here, uploaded once
  bool maps_new = false;      // ... they are no longer the caller's: setup_run_problem uploads them (SampleRun::perm_map)
  int keep_idx[8];            // weighted run: the compacted index of chunk k, or -1
};

static int check_run_args(const BeginState& r) {
  const cfd_sample_args& s = r.s;
  if (s.B < 1 || (s.G != 1 && s.G != 7 && (s.G < 1 || s.G > 8))) return fail(CFD_E_ARG, "bad B / G");
  if (s.scheduler < 0 || s.scheduler > 3)
    return fail(CFD_E_ARG, "scheduler must be 0 (DDPM), 1 (DDIM), 2 (DPM-Solver++ (2M)) or 3 (DDIM inversion)");
  if (s.scheduler == 3) {
    if (!s.timesteps) return fail(CFD_E_ARG, "DDIM inversion: pass the ascending timestep table in cfd_sample_args.timesteps");
    if (s.eta != 0.f) return fail(CFD_E_ARG, "DDIM inversion is deterministic: eta must be 0 (got %g)", (double)s.eta);
    if (s.clip_sample) return fail(CFD_E_ARG, "DDIM inversion: clip_sample must be 0 (a clipped x0 is not invertible)");
    if (s.preseq) return fail(CFD_E_ARG, "DDIM inversion takes no preseq (the rollout's prefix in-painting)");
    if (s.dynamic_memory_mask) return fail(CFD_E_ARG, "DDIM inversion takes no dynamic memories (dynamic_memory_mask = %d)", s.dynamic_memory_mask);
    if (r.x.edit) return fail(CFD_E_ARG, "DDIM inversion does not go together with an edit (cfd_sample_begin_edit)");
  }
  if (s.prediction_type != 0 && s.prediction_type != 1)
    return fail(CFD_E_ARG, "%s: prediction_type = %d is not 0 (epsilon) or 1 (sample)", r.x.opener, s.prediction_type);
  if (s.prediction_type == 1) {   // no trajectory to check these against (as DPM-Solver++'s refusals)
    if (s.scheduler == 3) return fail(CFD_E_ARG, "%s: DDIM inversion needs prediction_type = 0 (epsilon): inverting an x0-predicting model is not implemented", r.x.opener);
    if (r.x.anchor) return fail(CFD_E_ARG, "%s: an anchored run needs prediction_type = 0 (epsilon): its trajectory is an epsilon inversion's", r.x.opener);
    if (r.x.replay) return fail(CFD_E_ARG, "%s: the replay of a noise space needs prediction_type = 0 (epsilon): cfd_ddpm_invert solves it for an epsilon model", r.x.opener);
  }
  if (s.scheduler == 2 && !s.timesteps)
    return fail(CFD_E_ARG, "DPM-Solver++: pass the scheduler's timestep table in cfd_sample_args.timesteps (the library does not build it)");
  if (s.scheduler == 2 && s.clip_sample) return fail(CFD_E_ARG, "DPM-Solver++ has no clip_sample (clip_sample must be 0)");
  CHK(check_scheduler_tables(s, r.x.opener));
  if (s.preseq && (s.preseq_len < 1 || s.preseq_len > s.L)) return fail(CFD_E_ARG, "bad preseq_len");
  if (r.x.edit && (r.k0 < 0 || r.k0 >= r.N))   // (a replay's: its opener)
    return fail(CFD_E_ARG, "cfd_sample_begin_edit: first_iteration = %d is not in [0, %d)", r.k0, r.N);
  return CFD_OK;
}

// The keep mask of an edit, anchored or replay run on the host, every entry 0 or 1
static int fetch_keep_mask(BeginState& r) {
  const BeginExt& x = r.x;
  const uint8_t* keep_in = x.edit ? x.edit->keep : x.anchor ? x.anchor->keep : x.replay ? x.replay->keep : nullptr;
  if (!keep_in) return CFD_OK;
  const char* who = x.edit ? "cfd_sample_begin_edit" : x.anchor ? "cfd_sample_begin_anchored" : "cfd_sample_begin_replay";
  r.hkeep.resize((size_t)r.s.B * r.s.L);
  HIPCHK(hipMemcpy(r.hkeep.data(), keep_in, r.hkeep.size(), hipMemcpyDeviceToHost));
  for (size_t e = 0; e < r.hkeep.size(); ++e)
    if (r.hkeep[e] > 1) return fail(CFD_E_ARG, "%s: keep[%zu][%zu] = %d is not 0 or 1", who, e / r.s.L, e % r.s.L, (int)r.hkeep[e]);
  return CFD_OK;
}

// The tie table on the host: range, no self-tie, a source is free (neither tied nor kept), no token both kept and tied
static int fetch_tie_table(BeginState& r) {
  if (!r.x.tie) return CFD_OK;
  const cfd_sample_args& s = r.s;
  const std::vector<uint8_t>& hkeep = r.hkeep;
  std::vector<int32_t>& htie = r.htie;
  if (s.L < 1) return fail(CFD_E_ARG, "bad L");
  const long long nt = (long long)s.B * s.L;
  htie.resize((size_t)nt);
  HIPCHK(hipMemcpy(htie.data(), r.x.tie->tie, htie.size() * sizeof(int32_t), hipMemcpyDeviceToHost));
  for (long long e = 0; e < nt; ++e) {
    const long long t = htie[(size_t)e];
    const int b = (int)(e / s.L), l = (int)(e % s.L);
    if (t == -1) continue;
    if (t < -1 || t >= nt) return fail(CFD_E_ARG, "cfd_sample_begin_tied: tie[%d][%d] = %lld is not -1 or a token in [0, %lld)", b, l, t, nt);
    if (t == e) return fail(CFD_E_ARG, "cfd_sample_begin_tied: tie[%d][%d] = %lld ties the token to itself", b, l, t);
    if (htie[(size_t)t] != -1)
      return fail(CFD_E_ARG, "cfd_sample_begin_tied: tie[%d][%d] = %lld names a source (%lld, %lld) that is itself tied (no chains)", b, l, t,
                  t / s.L, t % s.L);
    if (!hkeep.empty() && hkeep[(size_t)t])
      return fail(CFD_E_ARG, "cfd_sample_begin_tied: tie[%d][%d] = %lld names a source (%lld, %lld) that is kept (a source must be free)", b, l,
                  t, t / s.L, t % s.L);
    if (!hkeep.empty() && hkeep[(size_t)e]) return fail(CFD_E_ARG, "cfd_sample_begin_tied: token (%d, %d) is both kept and tied", b, l);
  }
  return CFD_OK;
}

// The run's copy of the arguments and its evaluated chunks: the trailing zero-weight chunks trimmed, or a weighted run's table
static int select_chunks(BeginState& r) {
  Ctx* c = r.c;
  const cfd_sample_args& s = r.s;
  c->run.args = s;
  c->run.stream = r.st;
  c->setup_launches = 0;
  for (int j = 0; j < CFD_NMEM; ++j) r.n_ring += s.att_ring[j] != nullptr;
  if (r.n_ring != 0 && r.n_ring != CFD_NMEM) return fail(CFD_E_ARG, "att_ring: give all five buffers or none");
  if (r.n_ring && s.skip_zero_weight_chunks && s.G > 1 && s.guidance_weight[s.G - 1] == 0.0f)
    return fail(CFD_E_ARG, "att_ring keeps the maps of the LAST guidance chunk: it must be evaluated (skip_zero_weight_chunks = 0)");
  trim_zero_weight_chunks(c, s);
  c->run.args.timesteps = nullptr;   // (host pointer: not kept beyond this call)
  c->run.iters = r.N;
  for (int k = 0; k < 8; ++k) c->run.chunk_pos[k] = k;
  for (int j = 0; j < CFD_NMEM; ++j) r.mem_in[j] = s.mem[j];
  CHK(fetch_row_maps(r.mem_in, c->run.args.G * s.B, r.x.weights ? "G * B" : "Be", r.hm));
  if (r.x.weights) CHK(weighted_chunks(c, r.x.weights, r.x.prune, r.N, r.n_ring != 0, r.hm, r.keep_idx, r.st));
  r.maps_new = c->run.args.G != s.G && r.x.weights;
  return CFD_OK;
}

// Chunk permutation (see chunk_pos): group the chunks that use one shared copy of the largest memory
static int permute_chunks(BeginState& r) {
  Ctx* c = r.c;
  const int G = c->run.args.G, B = r.s.B, Be = G * B;
  bool all_maps = c->permute && G > 2;
  int jb = 0;
  for (int j = 0; j < CFD_NMEM; ++j) {
    if (!r.mem_in[j].row_map && !r.maps_new) all_maps = false;   // (a weighted run's compacted maps count as maps)
    if (r.s.mem[j].S > r.s.mem[jb].S) jb = j;
  }
  if (!all_maps) return CFD_OK;
  const std::vector<int>& hm = r.hm.m[jb];
  std::vector<int> key(G);   // the shared memory index of a uniform chunk, or -1
  for (int g = 0; g < G; ++g) {
    key[g] = hm[(size_t)g * B];
    for (int u = 1; u < B; ++u)
      if (hm[(size_t)g * B + u] != key[g]) { key[g] = -1; break; }
  }
  std::vector<int> order;   // order[position] = original chunk: uniform chunks grouped by key, first occurrence first
  std::vector<char> used(G, 0);
  for (int g = 0; g < G; ++g) {
    if (used[g] || key[g] < 0) continue;
    for (int h = g; h < G; ++h)
      if (!used[h] && key[h] == key[g]) { order.push_back(h); used[h] = 1; }
  }
  for (int g = 0; g < G; ++g)
    if (!used[g]) order.push_back(g);
  bool ident = true;
  for (int pnum = 0; pnum < G; ++pnum) ident = ident && order[pnum] == pnum;
  if (ident) return CFD_OK;
  for (int pnum = 0; pnum < G; ++pnum) c->run.chunk_pos[order[pnum]] = pnum;
  std::vector<int> pm(Be);
  for (std::vector<int>& m : r.hm.m) {
    for (int pnum = 0; pnum < G; ++pnum)
      for (int u = 0; u < B; ++u) pm[(size_t)pnum * B + u] = m[(size_t)order[pnum] * B + u];
    m = pm;
  }
  r.maps_new = true;
  return CFD_OK;
}

// The run's row maps on the device where the stages above changed them, each uploaded once
static int upload_run_maps(Ctx* c, const HostMaps& hm, cfd_memory mem_in[CFD_NMEM]) {
  for (int j = 0; j < CFD_NMEM; ++j) {
    CHK(c->run.perm_map[j].ensure(hm.m[j].size() * 4));
    HIPCHK(hipMemcpy(c->run.perm_map[j].p, hm.m[j].data(), hm.m[j].size() * 4, hipMemcpyHostToDevice));
    mem_in[j].row_map = c->run.perm_map[j].as<int32_t>();
  }
  return CFD_OK;
}

// The problem of the run's forward, and everything the run asks of it (PathAsk, forward_path.hpp): the rows of an attention ring -- the
// full-conditioning chunk's, at its position --, the memories rewritten between iterations, the operand policy (single-fp16 key / value
// tiles of the long memories wanted) and that the batch is G replicas of the run's B rows (begin_step_kernel writes G identical copies).
static int setup_run_problem(BeginState& r) {
  Ctx* c = r.c;
  const cfd_sample_args& s = r.s;
  if (r.maps_new) CHK(upload_run_maps(c, r.hm, r.mem_in));
  PathAsk ask;
  if (r.n_ring) { ask.ring_row0 = c->run.chunk_pos[c->run.args.G - 1] * s.B; ask.ring_rows = s.B; }
  ask.dynamic_mask = s.dynamic_memory_mask;
  ask.f16 = (c->xa_operands >= 0 ? c->xa_operands : (s.operand_policy & 15)) != 0;
  ask.chunk_rows = s.B;
  return setup_problem(c, c->run.args.G * s.B, s.L, r.mem_in, &r.hm, nullptr, ask, 0, r.N);
}

// The reference keeps att_mats of the full-conditioning chunk of EVERY iteration (convofusion.py:517-523).  On the row-tile path the
// second cross-attention launch has the probabilities in registers anyway: the rows of the last chunk store them into slot *d_step
// of the caller's ring, inside the captured iteration -- no second forward, no host round trip.
static int wire_att_ring(BeginState& r) {
  Ctx* c = r.c;
  const cfd_sample_args& s = r.s;
  Problem& pb = c->w->pb;
  if (!r.n_ring) return CFD_OK;
  // ... and on the tile kernels the fused cross-attention kernel has them in its softmax: its ATT instance keeps them, att_fixup_kernel
  // normalises them once per step (xattn_fused.hpp, XaAtt).  What cannot keep them: a run without the fused kernel (memories made per
  // step: dynamic memories; CFD_FUSED_XATTN=0).
  if ((!pb.path.rt && !pb.path.keeps_maps()) || s.dynamic_memory_mask)
    return fail(CFD_E_SHAPE, "att_ring needs the row-tile path or the fused cross-attention kernel (one timestep per step, no dynamic memory): "
                             "this run has L = %d, %lld token rows; take the maps with one forward per iteration instead", s.L,
                (long long)c->run.args.G * s.B * s.L);
  for (int j = 0; j < CFD_NMEM; ++j) {
    pb.att_slot[j] = (long long)s.B * c->nl * s.L * pb.S[j];
    // slot *d_step of the ring base: an edit run's d_step starts at k0 and executed iteration j goes to the caller's slot j
    pb.att[j] = s.att_ring[j] - (long long)r.k0 * pb.att_slot[j];
  }
  return CFD_OK;
}

// The attention-concentration census (cfd_sample_args::census_tau): the runs of the fused kernel's pair and F16 instances on projections
// made once per run -- the runs the operand policy is about
static int attention_census(BeginState& r) {
  Ctx* c = r.c;
  const ForwardPath& path = c->w->pb.path;
  const bool fused_run = path.xattn == XATTN_FUSED && !path.keeps_maps() && !r.s.dynamic_memory_mask;
  c->acen.tau = r.s.census_tau > 0.f ? r.s.census_tau : 0.f;
  c->acen.on = fused_run && c->acen.tau > 0.f;
  if (c->acen.on) CHK(c->acen.buf.ensure((size_t)c->nl * XA_CEN_SLOTS * XA_CEN_STRIDE * sizeof(unsigned)));
  return CFD_OK;
}

// The source, noise and mask buffers of the edit instances.  source: the edit's (the noise eps = the initial draw, now in the latents);
// NULL, a tied run without an edit: no kept token, the source and noise buffers are never read.
static int edit_buffers(BeginState& r, const float* source) {
  Ctx* c = r.c;
  CHK(c->run.enoise.ensure(r.lat_bytes));
  CHK(c->run.esrc.ensure(r.lat_bytes));
  if (source) {
    HIPCHK(hipMemcpyAsync(c->run.enoise.p, c->run.latents.p, r.lat_bytes, hipMemcpyDeviceToDevice, r.st));
    HIPCHK(hipMemcpyAsync(c->run.esrc.p, source, r.lat_bytes, hipMemcpyDeviceToDevice, r.st));
  }
  return upload_keep_mask(c, r.hkeep, (size_t)r.s.B * r.s.L, r.st);
}

// The anchored instance over a caller's ring of `steps` + 1 slots, read in place, and the keep mask
static int anchor_over(BeginState& r, const float* ring, int steps) {
  CHK(upload_keep_mask(r.c, r.hkeep, (size_t)r.s.B * r.s.L, r.st));
  HIPCHK(hipStreamSynchronize(r.st));   // (hkeep goes out of scope)
  r.c->run.mode.anchor = true;
  r.c->run.mode.anchor_ring = ring;
  r.c->run.mode.anchor_n = steps;
  return CFD_OK;
}

// The run's initial latents and what its kind adds: one block per field of BeginExt, each filling its part of RunMode
static int init_latents_and_kind(BeginState& r) {
  Ctx* c = r.c;
  const cfd_sample_args& s = r.s;
  const BeginExt& x = r.x;
  hipStream_t st = r.st;
  CHK(c->run.latents.ensure(r.lat_bytes));
  if (s.init_latents) HIPCHK(hipMemcpyAsync(c->run.latents.p, s.init_latents, r.lat_bytes, hipMemcpyDeviceToDevice, st));
  else CHK(enqueue_philox_fill(c->run.latents.as<float>(), s.B, s.L * CFD_LAT, (uint64_t)s.seed, 0u, s.first_utterance, 1u, 1.0f, st));
  // A tied run.  The scheduler step still steps a tied token (from the copied value and the token's own prediction) and, for DPM-Solver++,
  // keeps its x0 history; neither survives: the token is overwritten with its source at the start of the next iteration and once more
  // after the last (cfd_sample_read), and the history of a token feeds that token's step alone.
  if (x.tie) {   // the run's own copy of the table
    CHK(c->run.etie.ensure(r.htie.size() * sizeof(int32_t)));
    HIPCHK(hipMemcpyAsync(c->run.etie.p, r.htie.data(), r.htie.size() * sizeof(int32_t), hipMemcpyHostToDevice, st));
    if (!x.edit) CHK(edit_buffers(r, nullptr));   // (hkeep is empty here)
    HIPCHK(hipStreamSynchronize(st));   // (htie goes out of scope)
    c->run.mode.tie = true;
  }
  if (x.edit) {   // k0 > 0: every token starts at sa_k0 * source + sb_k0 * eps
    CHK(edit_buffers(r, x.edit->source));
    if (r.k0 > 0) {
      const long long n8 = (long long)s.B * s.L * (CFD_LAT / 8);
      hipLaunchKernelGGL(edit_init_kernel<>, dim3((unsigned)((n8 + 255) / 256)), dim3(256), 0, st, c->run.latents.as<float>(), c->run.esrc.as<float>(),
                         c->run.enoise.as<float>(), n8, c->run.coef.as<StepCoef>(), r.k0);
      HIPCHK(hipGetLastError());
    }
    HIPCHK(hipStreamSynchronize(st));   // (hkeep goes out of scope)
    c->run.mode.edit = true;
  }
  if (x.traj) {   // slot 0 of the trajectory: the initial latents (the source of the inversion)
    HIPCHK(hipMemcpyAsync(x.traj, c->run.latents.p, r.lat_bytes, hipMemcpyDeviceToDevice, st));
    HIPCHK(hipStreamSynchronize(st));
    c->run.mode.traj = x.traj;
  }
  if (x.anchor) CHK(anchor_over(r, x.anchor->trajectory, x.anchor->steps));
  if (x.replay) {   // the anchored instance over the noise space's trajectory; the opener pointed init_latents / step_noise into the rings
    CHK(anchor_over(r, x.replay->trajectory, x.replay->steps));
    c->run.mode.replay = true;
  }
  c->run.mode.k0 = r.k0;   // (0 but for an edit or a replay that starts later)
  c->run.iters = r.N - r.k0;
  // DPM-Solver++: the x0 history of the run, zeroed.  The first executed iteration is first order and never reads it, so the eager warm-up
  // iteration, which runs as that iteration and writes its x0 here, needs no save / restore: the first replay overwrites that before
  // anything reads it.
  if (s.scheduler == 2) {
    CHK(c->run.hist.ensure(r.lat_bytes));
    HIPCHK(hipMemsetAsync(c->run.hist.p, 0, r.lat_bytes, st));
  }
  CHK(c->run.inoise.ensure(s.preseq ? (size_t)s.B * s.preseq_len * CFD_LAT * 4 : 16));
  if (s.preseq) {
    HIPCHK(hipMemcpy2DAsync(c->run.inoise.p, (size_t)s.preseq_len * CFD_LAT * 4, c->run.latents.p, (size_t)s.L * CFD_LAT * 4,
                            (size_t)s.preseq_len * CFD_LAT * 4, s.B, hipMemcpyDeviceToDevice, st));
  }
  return CFD_OK;
}

// Eager warm-up of every kernel variant (sets function attributes outside capture); the iteration is idempotent on the workspace and
// the state it mutates (latents, in-paint noise, step index) is restored.
static int warm_up_iteration(BeginState& r) {
  Ctx* c = r.c;
  hipStream_t st = r.st;
  const bool preseq = r.s.preseq != nullptr;
  DBuf save_lat, save_in;
  CHK(save_lat.ensure(r.lat_bytes));
  HIPCHK(hipMemcpyAsync(save_lat.p, c->run.latents.p, r.lat_bytes, hipMemcpyDeviceToDevice, st));
  if (preseq) {
    CHK(save_in.ensure(c->run.inoise.bytes));
    HIPCHK(hipMemcpyAsync(save_in.p, c->run.inoise.p, c->run.inoise.bytes, hipMemcpyDeviceToDevice, st));
  }
  if (r.k0) HIPCHK(hipMemsetD32Async((hipDeviceptr_t)c->w->d_step.p, r.k0, 1, st));   // (d_step[0] = k0: coefficients, tables, ring slot 0)
  CHK(enqueue_loop_iteration(c, st));
  HIPCHK(hipMemcpyAsync(c->run.latents.p, save_lat.p, r.lat_bytes, hipMemcpyDeviceToDevice, st));
  if (preseq) HIPCHK(hipMemcpyAsync(c->run.inoise.p, save_in.p, c->run.inoise.bytes, hipMemcpyDeviceToDevice, st));
  HIPCHK(hipMemsetAsync(c->w->d_step.p, 0, 16, st));
  if (r.k0) HIPCHK(hipMemsetD32Async((hipDeviceptr_t)c->w->d_step.p, r.k0, 1, st));
  if (c->acen.on) HIPCHK(hipMemsetAsync(c->acen.buf.p, 0, (size_t)c->nl * XA_CEN_SLOTS * XA_CEN_STRIDE * sizeof(unsigned), st));   // (the warm-up counted too)
  HIPCHK(hipStreamSynchronize(st));
  return CFD_OK;
}

// Capture and replay on the handle's own stream (the legacy default stream cannot be captured); all set-up work was enqueued on the
// caller's stream and has been waited for.
static int capture_iteration(Ctx* c) {
  hipStream_t cap = c->own_stream;
  c->run.stream = cap;
  c->memside_in_forward = false;
  HIPCHK(hipStreamBeginCapture(cap, hipStreamCaptureModeThreadLocal));
  int r = enqueue_loop_iteration(c, cap);
  c->run.counts = c->memside_in_forward;   // (the hoisted / row-tile iteration has no counting launch: cfd_sample_read then skips the census read)
  c->memside_in_forward = false;
  c->acen.measured = c->acen.on && c->acen.hits > 0;
  c->acen.on = false;
  hipError_t e = hipStreamEndCapture(cap, &c->run.graph.graph);   // (sample_begin has emptied the holder)
  if (r != CFD_OK) { c->run.graph.reset(); return r; }
  if (e != hipSuccess) return fail(CFD_E_HIP, "stream capture failed: %s", hipGetErrorString(e));
  HIPCHK(hipGraphInstantiate(&c->run.graph.exec, c->run.graph.graph, nullptr, nullptr, 0));
  return CFD_OK;
}

// Opens a sampling run: the stages above, in the order the stream sees them
static int sample_begin(Ctx* c, const cfd_sample_args* args, void* stream, const BeginExt& x) {
  if (!c || !args) return fail(CFD_E_ARG, "null argument");
  if (x.weights && args->G != 7) return fail(CFD_E_ARG, "%s: a weight table needs the 7-chunk guidance batch (G = %d)", x.opener, args->G);
  if (c->run.open) return fail(CFD_E_STATE, "a sampling run is already open");
  CHK(setup_preamble(c));
  struct AcenOff { Ctx* c; ~AcenOff() { c->acen.on = false; } } acen_off{c};   // (the census slots go only into THIS run's launches)
  c->acen.valid = c->acen.measured = false;
  c->acen.hits = 0;
  cfd_sample_args s_w;
  if (x.weights) {   // a weighted run ignores guidance_weight and skip_zero_weight_chunks (its table says which chunks count)
    s_w = *args;
    s_w.skip_zero_weight_chunks = 0;
    args = &s_w;
  }
  c->run.mode = RunMode{};
  // N = loop iterations (the length of scheduler.timesteps); num_inference_steps = the count given to set_timesteps, which fixes the
  // stride `prev_t = t - T // n_inf` of the step formulas.  They differ only for a caller-supplied table.
  BeginState r{c, *args, x, (hipStream_t)stream, args->timesteps ? args->num_timesteps : args->num_inference_steps,
               x.edit ? x.edit->first_iteration : x.replay ? x.replay->first_iteration : 0};
  r.lat_bytes = (size_t)args->B * args->L * CFD_LAT * 4;
  CHK(check_run_args(r));
  CHK(fetch_keep_mask(r));
  CHK(fetch_tie_table(r));
  CHK(select_chunks(r));
  CHK(permute_chunks(r));
  if (x.weights) {
    for (int k = 0; k < 8; ++k) c->run.wpos[k] = c->run.chunk_pos[r.keep_idx[k] >= 0 ? r.keep_idx[k] : 0];
    c->run.mode.weighted = true;
    if (x.chunks_evaluated) *x.chunks_evaluated = c->run.args.G;
  }
  CHK(setup_run_problem(r));
  CHK(wire_att_ring(r));
  CHK(attention_census(r));
  CHK(upload_run_tables(c, r.s, r.N, r.k0, r.st));
  CHK(check_saturation(c, "cfd_sample_begin (memories / their once-per-run projections)"));
  CHK(init_latents_and_kind(r));
  c->run.graph.reset();
  CHK(warm_up_iteration(r));
  CHK(capture_iteration(c));
  c->run.open = true;
  c->run.pos = 0;
  c->acen.valid = true;
  if (!x.weights && x.chunks_evaluated) *x.chunks_evaluated = c->run.args.G;
  return CFD_OK;
}

// The openers: each checks what its kind of run needs, then says what it adds to the plain run (BeginExt).
extern "C" int cfd_sample_begin(cfd_handle c, const cfd_sample_args* args, void* stream) {
  return sample_begin(c, args, stream, BeginExt{});
}

extern "C" int cfd_sample_begin_weighted(cfd_handle c, const cfd_sample_args* args, const float* weights, int prune, int* chunks_evaluated,
                                         void* stream) {
  if (!c || !args) return fail(CFD_E_ARG, "null argument");
  if (!weights) return fail(CFD_E_ARG, "cfd_sample_begin_weighted: the weight table is NULL");
  if (args->G != 7) return fail(CFD_E_ARG, "cfd_sample_begin_weighted needs the 7-chunk guidance batch (G = %d)", args->G);
  return sample_begin(c, args, stream, BeginExt{"cfd_sample_begin_weighted", weights, prune, chunks_evaluated});
}

extern "C" int cfd_sample_begin_edit(cfd_handle c, const cfd_sample_args* args, const cfd_edit_args* e, const float* weights, int prune,
                                     int* chunks_evaluated, void* stream) {
  if (!c || !args || !e) return fail(CFD_E_ARG, "null argument");
  if (!e->source) return fail(CFD_E_ARG, "cfd_sample_begin_edit: the source latents are NULL");
  if (args->preseq) return fail(CFD_E_ARG, "cfd_sample_begin_edit: an edit run has no preseq (the rollout's prefix in-painting)");
  BeginExt x{"cfd_sample_begin_edit", weights, prune, chunks_evaluated};
  x.edit = e;
  return sample_begin(c, args, stream, x);
}

extern "C" int cfd_sample_begin_tied(cfd_handle c, const cfd_sample_args* args, const cfd_edit_args* e, const cfd_tie_args* t,
                                     const float* weights, int prune, int* chunks_evaluated, void* stream) {
  if (!c || !args || !t) return fail(CFD_E_ARG, "null argument");
  if (!t->tie) return fail(CFD_E_ARG, "cfd_sample_begin_tied: the tie table is NULL");
  if (e && !e->source) return fail(CFD_E_ARG, "cfd_sample_begin_tied: the source latents of the edit are NULL");
  if (e && e->first_iteration != 0)
    return fail(CFD_E_ARG, "cfd_sample_begin_tied: a tied run starts at iteration 0 (first_iteration = %d: no strength)", e->first_iteration);
  if (args->scheduler == 3) return fail(CFD_E_ARG, "cfd_sample_begin_tied: DDIM inversion (scheduler 3) takes no ties");
  if (args->preseq) return fail(CFD_E_ARG, "cfd_sample_begin_tied: a tied run has no preseq (give the prefix as kept tokens of an edit)");
  if (args->dynamic_memory_mask)
    return fail(CFD_E_ARG, "cfd_sample_begin_tied: a tied run takes no dynamic memories (dynamic_memory_mask = %d: dyadic runs)",
                args->dynamic_memory_mask);
  BeginExt x{"cfd_sample_begin_tied", weights, prune, chunks_evaluated};
  x.edit = e;
  x.tie = t;
  return sample_begin(c, args, stream, x);
}

extern "C" int cfd_sample_begin_invert(cfd_handle c, const cfd_sample_args* args, float* trajectory, const float* weights, int prune,
                                       int* chunks_evaluated, void* stream) {
  if (!c || !args) return fail(CFD_E_ARG, "null argument");
  if (!trajectory) return fail(CFD_E_ARG, "cfd_sample_begin_invert: the trajectory is NULL");
  if (args->scheduler != 3) return fail(CFD_E_ARG, "cfd_sample_begin_invert: scheduler must be 3 (DDIM inversion), not %d", args->scheduler);
  BeginExt x{"cfd_sample_begin_invert", weights, prune, chunks_evaluated};
  x.traj = trajectory;
  return sample_begin(c, args, stream, x);
}

extern "C" int cfd_sample_begin_anchored(cfd_handle c, const cfd_sample_args* args, const cfd_anchor_args* an, const float* weights,
                                         int prune, int* chunks_evaluated, void* stream) {
  if (!c || !args || !an) return fail(CFD_E_ARG, "null argument");
  if (!an->trajectory) return fail(CFD_E_ARG, "cfd_sample_begin_anchored: the trajectory is NULL");
  if (args->scheduler != 1) return fail(CFD_E_ARG, "cfd_sample_begin_anchored: an anchored run is a DDIM run (scheduler 1, not %d)", args->scheduler);
  if (args->eta != 0.f || args->clip_sample)
    return fail(CFD_E_ARG, "cfd_sample_begin_anchored: the DDIM run must be deterministic and unclipped (eta = %g, clip_sample = %d)",
                (double)args->eta, args->clip_sample);
  if (args->preseq) return fail(CFD_E_ARG, "cfd_sample_begin_anchored: an anchored run has no preseq");
  const int n_iter = args->timesteps ? args->num_timesteps : args->num_inference_steps;
  if (an->steps != n_iter || an->B != args->B || an->L != args->L)
    return fail(CFD_E_ARG, "cfd_sample_begin_anchored: the trajectory is [%d + 1][%d][%d][128], this run has %d iterations of [%d][%d][128]",
                an->steps, an->B, an->L, n_iter, args->B, args->L);
  BeginExt x{"cfd_sample_begin_anchored", weights, prune, chunks_evaluated};
  x.anchor = an;
  return sample_begin(c, args, stream, x);
}

extern "C" int cfd_sample_begin_replay(cfd_handle c, const cfd_sample_args* args, const cfd_replay_args* r, const float* weights, int prune,
                                       int* chunks_evaluated, void* stream) {
  if (!c || !args || !r) return fail(CFD_E_ARG, "null argument");
  if (!r->trajectory || !r->noise) return fail(CFD_E_ARG, "cfd_sample_begin_replay: the trajectory or the noise is NULL");
  if (args->scheduler != 0) return fail(CFD_E_ARG, "cfd_sample_begin_replay: a noise space is replayed by a DDPM run (scheduler 0, not %d)", args->scheduler);
  if (args->preseq) return fail(CFD_E_ARG, "cfd_sample_begin_replay: a replay has no preseq");
  if (args->dynamic_memory_mask)
    return fail(CFD_E_ARG, "cfd_sample_begin_replay: a replay takes no dynamic memories (dynamic_memory_mask = %d)", args->dynamic_memory_mask);
  const int n_iter = args->timesteps ? args->num_timesteps : args->num_inference_steps;
  if (r->steps != n_iter || r->B != args->B || r->L != args->L)
    return fail(CFD_E_ARG, "cfd_sample_begin_replay: the noise space is [%d][%d][%d][128], this run has %d iterations of [%d][%d][128]", r->steps,
                r->B, r->L, n_iter, args->B, args->L);
  if (r->first_iteration < 0 || r->first_iteration >= n_iter)   // (here, not in check_run_args: init_latents below is computed from it)
    return fail(CFD_E_ARG, "cfd_sample_begin_replay: first_iteration = %d is not in [0, %d)", r->first_iteration, n_iter);
  cfd_sample_args s = *args;   // the run starts from the level iteration k0 enters and takes the recorded noise as its step noise
  s.init_latents = r->trajectory + (size_t)(n_iter - r->first_iteration) * args->B * args->L * CFD_LAT;
  s.step_noise = r->noise;
  BeginExt x{"cfd_sample_begin_replay", weights, prune, chunks_evaluated};
  x.replay = r;
  return sample_begin(c, &s, stream, x);
}

// ---- level batches: J noise levels of one run as one forward (Problem::tmode 2; cfd_ddpm_invert, cfd_sample_parallel) ----------------
static void (*const ddpm_extract_kernel_weighted)(const ExtractArgs) = ddpm_extract_kernel<0, true>;   // (one macro argument for LAUNCH)
static void (*const picard_step_kernel_weighted)(const PicardStepArgs) = picard_step_kernel<0, true>;

// What a level batch's callers refuse alike (`who`: the entry point, for the message)
static int level_batch_refusals(Ctx* c, const cfd_sample_args* args, const char* who, const char* why0, int levels_per_batch) {
  if (args->scheduler != 0) return fail(CFD_E_ARG, "%s: %s (scheduler 0, not %d)", who, why0, args->scheduler);
  if (args->prediction_type != 0)
    return fail(CFD_E_ARG, "%s needs prediction_type = 0 (epsilon), not %d: its level kernels step an epsilon model", who, args->prediction_type);
  if (args->preseq) return fail(CFD_E_ARG, "%s takes no preseq (the rollout's prefix in-painting)", who);
  if (args->dynamic_memory_mask) return fail(CFD_E_ARG, "%s takes no dynamic memories (dynamic_memory_mask = %d)", who, args->dynamic_memory_mask);
  for (int j = 0; j < CFD_NMEM; ++j)
    if (args->att_ring[j]) return fail(CFD_E_ARG, "%s keeps no attention maps (att_ring)", who);
  if (levels_per_batch < 0) return fail(CFD_E_ARG, "%s: levels_per_batch = %d", who, levels_per_batch);
  if (c->run.open) return fail(CFD_E_STATE, "a sampling run is open on this handle");
  return CFD_OK;
}

// The guidance combine of a level batch and its sizes, as level_batch_setup leaves them
struct LevelBatch {
  int B, L, N, Ge, J;
  Combine g;             // Gc: 7 for a weighted run, else Ge; wtab: dev [N][B][8] or null
};

// J, the levels of a batch: the caller's count, or the workspace budget divided by the budget's unit -- per_level, the bytes setup_problem
// allocated per level when the default was measured (token rows, the memories' per-forward projections, and score buffers the workspace
// no longer holds), not what is allocated today: the formula defines the default J, and with it the GEMM tile classes of the timings
// below, so it stays as it is; an estimate, not an enforced cap.  At most N, and at most 32768 batch rows (a launch's grid).
// (default 4 GiB: at the product shape ~150 levels for one utterance, ~40 for eight; measured 0.042 s at J = 100 against 0.059 s at
//  J = 41 and 0.187 s at J = 40 against 0.279 s at J = 8 for N = 1000, profiles/r13_ddpm_inversion_time.json)
static int levels_per_batch_of(Ctx* c, const cfd_memory mem_in[CFD_NMEM], int R, int L, int N, int levels_per_batch, size_t workspace_bytes,
                               int* J_out) {
  size_t per_level = 0;
  int sp_tot = 0;
  for (int j = 0; j < CFD_NMEM; ++j) {
    if (mem_in[j].U < 1 || mem_in[j].S < 1) return fail(CFD_E_ARG, "memory %s: null/empty", MEM_NAMES[j]);
    const size_t sp = (size_t)(mem_in[j].S + 31) / 32 * 32;
    sp_tot += (int)sp;
    per_level += (size_t)mem_in[j].U * sp * ((size_t)CFD_D * 4 * (1 + 2 * c->nl) + 4 * (c->nl + 1));
  }
  per_level += (size_t)R * L * ((size_t)CFD_D * 4 * 6 + (size_t)CFD_FF * 4 + (size_t)sp_tot * 8 + CFD_LAT * 8) +
               (size_t)R * ((size_t)CFD_D * 64 * 4 + (size_t)CFD_NHEAD * L * ((L + 31) / 32 * 32) * 8);
  const size_t budget = workspace_bytes ? workspace_bytes : (size_t)4 << 30;
  const long long J = levels_per_batch ? levels_per_batch : (long long)(budget / per_level);
  *J_out = (int)std::max<long long>(1, std::min<long long>({J, (long long)N, 32768 / R > 0 ? 32768 / R : 1}));
  return CFD_OK;
}

// The level batch's memories: instance lv * U + u = the caller's memory u at level lv, through level row maps made from the host copy `hm`
// of the caller's maps (R rows per level; hm becomes the level maps, J * R rows); masks once per level
static int level_batch_memories(Ctx* c, const cfd_memory mem_in[CFD_NMEM], int R, int J, HostMaps& hm, cfd_memory vm[CFD_NMEM]) {
  const int Be = J * R;
  for (int j = 0; j < CFD_NMEM; ++j) {
    const int U = mem_in[j].U;
    std::vector<int>& lm = hm.m[j];
    lm.resize((size_t)Be);
    for (int lv = 1; lv < J; ++lv)
      for (int r = 0; r < R; ++r) lm[(size_t)lv * R + r] = lv * U + lm[r];
    CHK(c->lv_map[j].ensure((size_t)Be * 4));
    HIPCHK(hipMemcpy(c->lv_map[j].p, lm.data(), (size_t)Be * 4, hipMemcpyHostToDevice));
    vm[j] = mem_in[j];
    vm[j].row_map = c->lv_map[j].as<int32_t>();
    vm[j].U = J * U;
    if (mem_in[j].key_padding_mask) {
      const size_t mb = (size_t)U * mem_in[j].S;
      CHK(c->lv_mask[j].ensure(mb * (size_t)J));
      for (int lv = 0; lv < J; ++lv)
        HIPCHK(hipMemcpy(c->lv_mask[j].as<uint8_t>() + (size_t)lv * mb, mem_in[j].key_padding_mask, mb, hipMemcpyDeviceToDevice));
      vm[j].key_padding_mask = c->lv_mask[j].as<uint8_t>();
    }
  }
  return CFD_OK;
}

// Everything a level batch needs before its first forward: the evaluated chunks and their row maps, J from the workspace budget, the
// level row maps and masks, the problem (tmode 2, table of N rows) and the run's tables (upload_run_tables: the saturation census is
// opened and the stream waited for).  The caller sets Problem::lv_i0 per batch and reads the census at its end.  coef_out: the
// coefficient rows on the host.
static int level_batch_setup(Ctx* c, const cfd_sample_args& s, const char* who, const float* wtab, int prune, int levels_per_batch,
                             size_t workspace_bytes, hipStream_t st, LevelBatch* lb, std::vector<StepCoef>* coef_out = nullptr) {
  if (wtab && s.G != 7) return fail(CFD_E_ARG, "%s: a weight table needs the 7-chunk guidance batch (G = %d)", who, s.G);
  if (s.B < 1 || s.L < 2 || s.G < 1 || s.G > 8) return fail(CFD_E_ARG, "bad B / L / G");
  CHK(check_scheduler_tables(s, who));
  CHK(setup_preamble(c));
  const int N = s.timesteps ? s.num_timesteps : s.num_inference_steps;
  // the evaluated chunks and their memories' row maps, as a run with these arguments would have them (weighted_chunks works on c->run.args)
  c->run.args = s;
  c->run.args.timesteps = nullptr;
  cfd_memory mem_in[CFD_NMEM], vm[CFD_NMEM];
  for (int j = 0; j < CFD_NMEM; ++j) mem_in[j] = s.mem[j];
  memset(lb, 0, sizeof(*lb));
  HostMaps hm;
  if (!wtab) trim_zero_weight_chunks(c, s);
  CHK(fetch_row_maps(mem_in, c->run.args.G * s.B, "G * B", hm));
  if (wtab) {
    int keep_idx[8];
    CHK(weighted_chunks(c, wtab, prune, N, false, hm, keep_idx, st));
    for (int k = 0; k < 8; ++k) lb->g.pos[k] = keep_idx[k] >= 0 ? keep_idx[k] : 0;
    lb->g.Gc = 7;
    lb->g.wtab = c->run.wtab.as<float>();
  } else {
    for (int k = 0; k < 8; ++k) { lb->g.pos[k] = k < c->run.args.G ? k : 0; lb->g.w[k] = s.guidance_weight[k]; }
    lb->g.Gc = c->run.args.G;
  }
  lb->g.clip = s.clip_sample;
  lb->B = s.B; lb->L = s.L; lb->N = N; lb->Ge = c->run.args.G;
  const int R = lb->Ge * s.B;   // rows of a level
  CHK(levels_per_batch_of(c, mem_in, R, s.L, N, levels_per_batch, workspace_bytes, &lb->J));
  CHK(level_batch_memories(c, mem_in, R, lb->J, hm, vm));
  CHK(setup_problem(c, lb->J * R, s.L, vm, &hm, nullptr, PathAsk{}, 2, N));   // (operands are split pairs throughout)
  Problem& pb = c->w->pb;
  pb.lv_rows = R;
  pb.lv_i0 = 0;
  for (int j = 0; j < CFD_NMEM; ++j) pb.lv_U[j] = mem_in[j].U;
  // (time tables: every level's rows, once; prepare_static_memside, tmode 2: the scale planes only, the projections are made per level
  //  in the forward)
  return upload_run_tables(c, s, N, 0, st, coef_out);
}

// ---- edit-friendly DDPM inversion: every level of the table in a few level-batched forwards (cfdenoise.h: cfd_ddpm_invert) ----------
extern "C" int cfd_ddpm_invert(cfd_handle c, const cfd_sample_args* args, const cfd_ddpm_invert_args* inv, int* chunks_evaluated,
                               int* levels_per_batch_used, void* stream) {
  if (!c || !args || !inv) return fail(CFD_E_ARG, "null argument");
  if (!inv->source || !inv->trajectory || !inv->noise) return fail(CFD_E_ARG, "cfd_ddpm_invert: the source, the trajectory or the noise is NULL");
  CHK(level_batch_refusals(c, args, "cfd_ddpm_invert", "the noise space is a DDPM run's", inv->levels_per_batch));
  const cfd_sample_args& s = *args;
  hipStream_t st = (hipStream_t)stream;
  LevelBatch lb;
  CHK(level_batch_setup(c, s, "cfd_ddpm_invert", inv->weights, inv->prune, inv->levels_per_batch, inv->workspace_bytes, st, &lb));
  const int B = lb.B, L = lb.L, N = lb.N, Ge = lb.Ge, J = lb.J;
  Problem& pb = c->w->pb;
  ExtractArgs xa;
  memset(&xa, 0, sizeof(xa));
  xa.g = lb.g;
  const size_t lat_bytes = (size_t)B * L * CFD_LAT * 4;
  HIPCHK(hipMemcpyAsync(inv->trajectory, inv->source, lat_bytes, hipMemcpyDeviceToDevice, st));   // slot 0: the source
  LevelArgs la{inv->source, inv->level_noise, inv->trajectory, c->w->sample_sp.as<char>(), c->run.coef.as<StepCoef>(), B, L, Ge, N, 0, J,
               (unsigned long long)s.seed, s.first_utterance};
  xa.eps = c->w->eps.as<float>(); xa.traj = inv->trajectory; xa.noise = inv->noise; xa.coef = c->run.coef.as<StepCoef>();
  xa.B = B; xa.L = L; xa.G = Ge; xa.N = N; xa.J = J;
  const long long n8 = (long long)J * B * L * (CFD_LAT / 8);
  const dim3 grid((unsigned)((n8 + 255) / 256)), block(256);
  // Batches from the noisiest levels' end of the table downwards: the noise of iteration i needs slot N - i - 1, the level of iteration
  // i + 1 (the source for the last one), which the batch before has built.  The last batch starts at iteration 0 whatever N % J is, so
  // that one problem set-up and one work list serve every batch: the levels it shares with the batch before are evaluated again and
  // their rows written again -- the trajectory slots to the same bits, the noise rows to the re-association between two batch
  // compositions (measured 4e-7); what stays is the last batch's.
  for (int hi = N; hi > 0; hi -= J) {
    const int i0 = std::max(hi - J, 0);
    pb.lv_i0 = la.i0 = xa.i0 = i0;
    LAUNCH(CFD_PROF_OTHER, ddpm_level_kernel<>, grid, block, st, la);
    CHK(enqueue_denoise(c, st));
    if (lb.g.wtab) LAUNCH(CFD_PROF_OTHER, ddpm_extract_kernel_weighted, grid, block, st, xa);
    else LAUNCH(CFD_PROF_OTHER, ddpm_extract_kernel<>, grid, block, st, xa);
  }
  // the per-level projections count into the handle's census: read here, so that a clamped projection fails THIS call
  HIPCHK(hipStreamSynchronize(st));
  c->memside_in_forward = false;
  CHK(check_saturation(c, "cfd_ddpm_invert (source levels, memories / their per-level projections)"));
  if (chunks_evaluated) *chunks_evaluated = Ge;
  if (levels_per_batch_used) *levels_per_batch_used = J;
  return CFD_OK;
}

// The stride of a sweep (cfdenoise.h: cfd_sample_parallel): the largest s in [1, p] with err[k][b] / (L * 128) <= tau^2 * v(i0 + k) for
// every 1 <= k < s and every b; err[k][b]: the squared change of X(i0 + k), v(i) = sigma_i^2 (an iteration that adds no noise: the value
// of the iteration before it).  A NaN fails the comparison: the window then moves by the levels in front of it.
static int picard_stride(const float* err, int B, int p, int i0, const StepCoef* coef, float tau, int L) {
  int s = 1;
  for (; s < p; ++s) {
    int iv = i0 + s;
    if (coef[iv].use_noise == 0.f && iv > 0) iv -= 1;
    const float bound = tau * tau * (coef[iv].sigma * coef[iv].sigma);
    for (int b = 0; b < B; ++b)
      if (!(err[(size_t)s * B + b] / (float)(L * CFD_LAT) <= bound)) return s;
  }
  return s;
}

// The launches of a Picard sweep, once for cfd_sample_parallel and the developer hook cfd_test_picard_sweep: the ring, the sizes, the
// grids, the kernels' argument structs and the choice of the step instance, one function per stage.
struct PicardSweep {
  Ctx* c;
  hipStream_t st;
  PicardStepArgs sa;     // ring, B, L, G, J: set here; eps / s / coef / g / noise / seed / utt0: the caller's, before step()
  int nblk;              // the scan's workgroups per utterance
  PicardSweep(Ctx* c_, hipStream_t st_, const PicardRing& ring, int B, int L, int G, int J) : c(c_), st(st_), nblk((L * (CFD_LAT / 4) + 255) / 256) {
    memset(&sa, 0, sizeof(sa));
    sa.ring = ring; sa.B = B; sa.L = L; sa.G = G; sa.J = J;
  }
  dim3 grid(int levels) const { return dim3((unsigned)((sa.ring.chunk / 8 * levels + 255) / 256)); }   // one thread = 8 elements of a level
  size_t part_bytes() const { return (size_t)sa.J * sa.B * nblk * 4; }
  int fill(int src, int lo, int hi) {   // X(i) = X(src) for the iterations lo .. hi (none: no launch)
    if (hi >= lo) LAUNCH(CFD_PROF_OTHER, picard_fill_kernel<>, grid(hi - lo + 1), dim3(256), st, sa.ring, src, lo, hi);
    return CFD_OK;
  }
  int load(int base, char* sample_sp) {
    LAUNCH(CFD_PROF_OTHER, picard_load_kernel<>, grid(sa.J), dim3(256), st, PicardLoadArgs{sa.ring, sample_sp, sa.B, sa.L, sa.G, base, sa.J});
    return CFD_OK;
  }
  int step(int base, int off) {   // the weighted instance where the combine has a table
    sa.base = base; sa.off = off;
    if (sa.g.wtab) LAUNCH(CFD_PROF_OTHER, picard_step_kernel_weighted, grid(sa.J), dim3(256), st, sa);
    else LAUNCH(CFD_PROF_OTHER, picard_step_kernel<>, grid(sa.J), dim3(256), st, sa);
    return CFD_OK;
  }
  int scan_err(int base, int off, float* part, float* err) {
    LAUNCH(CFD_PROF_OTHER, picard_scan_kernel<>, dim3((unsigned)nblk, (unsigned)sa.B), dim3(256), st,
           PicardScanArgs{sa.s, sa.ring, part, sa.L, base, off, sa.J});
    LAUNCH(CFD_PROF_OTHER, picard_err_kernel<>, dim3((unsigned)((sa.J * sa.B + 255) / 256)), dim3(256), st, part, err, sa.J, sa.B, nblk, sa.J - off);
    return CFD_OK;
  }
};

// ---- parallel-in-time DDPM sampling: Picard sweeps over level batches (cfdenoise.h: cfd_sample_parallel) ---------------------------
extern "C" int cfd_sample_parallel(cfd_handle c, const cfd_sample_args* args, const cfd_parallel_args* par, cfd_parallel_stats* stats,
                                   void* stream) {
  if (!c || !args || !par) return fail(CFD_E_ARG, "null argument");
  if (!par->latents) return fail(CFD_E_ARG, "cfd_sample_parallel: the output latents are NULL");
  if (!(par->tolerance >= 0.f) || !std::isfinite(par->tolerance))
    return fail(CFD_E_ARG, "cfd_sample_parallel: tolerance = %g is not a finite number >= 0", (double)par->tolerance);
  if (par->max_sweeps < 0) return fail(CFD_E_ARG, "cfd_sample_parallel: max_sweeps = %d", par->max_sweeps);
  CHK(level_batch_refusals(c, args, "cfd_sample_parallel", "the window is a DDPM chain's", par->levels_per_batch));
  const cfd_sample_args& s = *args;
  hipStream_t st = (hipStream_t)stream;
  LevelBatch lb;
  std::vector<StepCoef> coef;   // (the stride rule's sigma)
  CHK(level_batch_setup(c, s, "cfd_sample_parallel", par->weights, par->prune, par->levels_per_batch, par->workspace_bytes, st, &lb, &coef));
  const int B = lb.B, L = lb.L, N = lb.N, Ge = lb.Ge, J = lb.J;
  Problem& pb = c->w->pb;
  const long long chunk = (long long)B * L * CFD_LAT;
  // the ring: the caller's trajectory, or J + 1 slots of the handle (the window's p + 1 latents; at the end of the table, where the batch
  // starts in front of the window, the J + 1 latents N - J .. N)
  PicardRing ring{par->trajectory, N + 1, N, chunk};
  if (!ring.x) {
    ring.slots = J + 1;
    CHK(c->run.latents.ensure((size_t)ring.slots * chunk * 4));
    ring.x = c->run.latents.as<float>();
  }
  PicardSweep sw(c, st, ring, B, L, Ge, J);
  DBuf &sbuf = c->pic_s, &part = c->pic_part, &err = c->pic_err;
  CHK(sbuf.ensure((size_t)J * chunk * 4));
  CHK(part.ensure(sw.part_bytes()));
  CHK(err.ensure((size_t)J * B * 4));
  std::vector<float> herr((size_t)J * B);
  if (s.init_latents) HIPCHK(hipMemcpyAsync(ring.at(0), s.init_latents, (size_t)chunk * 4, hipMemcpyDeviceToDevice, st));
  else CHK(enqueue_philox_fill(ring.at(0), B, L * CFD_LAT, (uint64_t)s.seed, 0u, s.first_utterance, 1u, 1.0f, st));
  CHK(sw.fill(0, 1, J));   // every latent of the first window starts from X(0)
  sw.sa.eps = c->w->eps.as<float>(); sw.sa.s = sbuf.as<float>(); sw.sa.coef = c->run.coef.as<StepCoef>(); sw.sa.g = lb.g;
  sw.sa.noise = s.step_noise; sw.sa.seed = s.seed; sw.sa.utt0 = s.first_utterance;
  const int max_sweeps = par->max_sweeps ? par->max_sweeps : N;
  int sweeps = 0;
  for (int i0 = 0; i0 < N;) {
    if (sweeps >= max_sweeps) {
      (void)hipStreamSynchronize(st);
      c->memside_in_forward = false;
      (void)check_saturation(c, "cfd_sample_parallel");
      return fail(CFD_E_STATE, "cfd_sample_parallel: max_sweeps = %d reached with %d of %d levels final (tolerance %g, %d levels per batch)",
                  max_sweeps, i0, N, (double)par->tolerance, J);
    }
    const int base = std::min(i0, N - J), off = i0 - base, p = J - off;   // (J <= N; p = min(J, N - i0))
    pb.lv_i0 = base;
    CHK(sw.load(base, c->w->sample_sp.as<char>()));
    CHK(enqueue_denoise(c, st));
    CHK(sw.step(base, off));
    CHK(sw.scan_err(base, off, part.as<float>(), err.as<float>()));
    HIPCHK(hipMemcpyAsync(herr.data(), err.p, herr.size() * 4, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));   // the one wait of a sweep: the stride is decided on the host
    const int stride = picard_stride(herr.data(), B, p, i0, coef.data(), par->tolerance, L);
    if (stats && stats->strides && sweeps < stats->strides_capacity) stats->strides[sweeps] = stride;
    sweeps += 1;
    // the levels that enter the window start from its last value, X(i0 + p)
    const int i1 = i0 + stride;
    CHK(sw.fill(i0 + p, i0 + p + 1, i1 + std::min(J, N - i1)));
    i0 = i1;
  }
  HIPCHK(hipMemcpyAsync(par->latents, ring.at(N), (size_t)chunk * 4, hipMemcpyDeviceToDevice, st));
  // the per-level projections count into the handle's census: read here, so that a clamped projection fails THIS call
  HIPCHK(hipStreamSynchronize(st));
  c->memside_in_forward = false;
  CHK((check_saturation(c, "cfd_sample_parallel (window levels, memories / their per-level projections)")));
  if (stats) { stats->levels_per_batch = J; stats->chunks_evaluated = Ge; stats->sweeps = sweeps; }
  return CFD_OK;
}

extern "C" int cfd_sample_census(cfd_handle c, cfd_census* out) {
  if (!c || !out) return fail(CFD_E_ARG, "null argument");
  if (!c->acen.valid) return fail(CFD_E_STATE, "no sampling run was opened on this handle");
  memset(out, 0, sizeof(*out));
  out->tau = c->acen.tau;
  out->measured = c->acen.measured ? 1 : 0;
  out->iterations = c->run.pos;
  out->worst_layer = -1;
  if (!c->acen.measured) return CFD_OK;
  HIPCHK(hipSetDevice(c->cfg.device));
  HIPCHK(hipStreamSynchronize(c->run.stream));
  std::vector<unsigned> h((size_t)c->nl * XA_CEN_SLOTS * XA_CEN_STRIDE);
  HIPCHK(hipMemcpy(h.data(), c->acen.buf.p, h.size() * sizeof(unsigned), hipMemcpyDeviceToHost));
  for (int l = 0; l < c->nl; ++l) {
    unsigned pk_bits = 0, over = 0, seen = 0;   // (positive floats order like their bits)
    for (int sl = 0; sl < XA_CEN_SLOTS; ++sl) {
      const unsigned* v = &h[((size_t)l * XA_CEN_SLOTS + sl) * XA_CEN_STRIDE];
      pk_bits = std::max(pk_bits, v[0]);
      over += v[1];
      seen += v[2];
    }
    float pk;
    memcpy(&pk, &pk_bits, 4);
    if (l < CFD_CENSUS_MAX_LAYERS) { out->layer_peak[l] = pk; out->layer_over[l] = over; }
    if (seen > 0 && (out->worst_layer < 0 || pk > out->peak_max)) { out->peak_max = pk; out->worst_layer = l; }
    out->rows_over += over;
    out->rows_seen += seen;
  }
  return CFD_OK;
}

extern "C" int cfd_sample_steps(cfd_handle c, int n) {
  if (!c) return fail(CFD_E_ARG, "null handle");
  if (!c->run.open) return fail(CFD_E_STATE, "no sampling run open");
  if (n < 0 || c->run.pos + n > c->run.iters)
    return fail(CFD_E_ARG, "run has %d of %d iterations done; cannot run %d more", c->run.pos, c->run.iters, n);
  HIPCHK(hipSetDevice(c->cfg.device));
  for (int i = 0; i < n; ++i) HIPCHK(hipGraphLaunch(c->run.graph.exec, c->run.stream));
  c->run.pos += n;
  return CFD_OK;
}

extern "C" int cfd_dyadic_steps(cfd_handle a, cfd_handle b, const cfd_dyadic_proj* pr, int n) {
  if (!a || !pr || a == b) return fail(CFD_E_ARG, "side A's handle, the projection and (two-handle form) a distinct side B handle are needed");
  if (!a->run.open || (b && !b->run.open)) return fail(CFD_E_STATE, "both sides need an open sampling run");
  if (!pr->w1 || !pr->b1 || !pr->w2 || !pr->b2 || !pr->spk_a || !pr->spk_b || !pr->tmp || pr->hidden < 1 || pr->out_dim != CFD_D)
    return fail(CFD_E_ARG, "bad partner projection");
  const cfd_sample_args& sa = a->run.args;
  if (a->run.mode.tie || (b && b->run.mode.tie)) return fail(CFD_E_ARG, "a tied run takes no dyadic steps");
  if (!(sa.dynamic_memory_mask & 1) || (b && !(b->run.args.dynamic_memory_mask & 1)))
    return fail(CFD_E_STATE, "the speaker memory of the run(s) must be declared dynamic");
  if (b && (sa.B != b->run.args.B || sa.L != b->run.args.L || a->cfg.device != b->cfg.device)) return fail(CFD_E_ARG, "the two sides differ in batch, length or device");
  if (!b && sa.B % 2) return fail(CFD_E_ARG, "merged form: the run holds side A's utterances followed by side B's (even batch)");
  if (n < 0 || a->run.pos + n > a->run.iters || (b && b->run.pos + n > b->run.iters))
    return fail(CFD_E_ARG, "run has %d of %d iterations done; cannot run %d more", a->run.pos, a->run.iters, n);
  HIPCHK(hipSetDevice(a->cfg.device));
  hipStream_t st = a->run.stream;
  if (b) {
    // side B's stream may still hold its set-up or an earlier read: everything below is ordered behind it, and side B's later reads
    // behind everything below (events, no host wait)
    HIPCHK(hipEventRecord(b->grad.ev, b->run.stream));
    HIPCHK(hipStreamWaitEvent(st, b->grad.ev, 0));
  }
  const int Bs = b ? sa.B : sa.B / 2;                  // utterances per side
  const long long rows = (long long)Bs * sa.L;
  const dim3 blk(256);
  const long long gy = (rows + 31) / 32;
  if (gy > 65535) return fail(CFD_E_ARG, "too many rows for one launch (%lld)", rows);
  auto project = [&](const float* lat, float* spk) {
    (void)enqueue_linear_act(lat, rows, CFD_LAT, pr->w1, pr->b1, pr->hidden, 1, pr->tmp, st);
    (void)enqueue_linear_act((const float*)pr->tmp, rows, pr->hidden, pr->w2, pr->b2, pr->out_dim, 1, spk, st);
  };
  const float* lat_a = a->run.latents.as<float>();
  const float* lat_b = b ? b->run.latents.as<float>() : lat_a + rows * CFD_LAT;
  for (int i = 0; i < n; ++i) {
    project(lat_b, pr->spk_a);                         // A attends to B's latents as they stand at the start of the iteration ...
    project(lat_a, pr->spk_b);                         // ... and B to A's
    HIPCHK(hipGetLastError());
    HIPCHK(hipGraphLaunch(a->run.graph.exec, st));
    if (b) HIPCHK(hipGraphLaunch(b->run.graph.exec, st));       // same queue, one after the other: no two-queue overlap
  }
  a->run.pos += n;
  if (b) {
    b->run.pos += n;
    HIPCHK(hipEventRecord(a->grad.ev, st));
    HIPCHK(hipStreamWaitEvent(b->run.stream, a->grad.ev, 0));
  }
  return CFD_OK;
}

extern "C" int cfd_sample_position(cfd_handle c) { return (c && c->run.open) ? c->run.pos : -1; }

extern "C" int cfd_sample_read(cfd_handle c, float* out, int close) {
  if (!c || !out) return fail(CFD_E_ARG, "null argument");
  if (!c->run.open) return fail(CFD_E_STATE, "no sampling run open");
  HIPCHK(hipSetDevice(c->cfg.device));
  const size_t lat_bytes = (size_t)c->run.args.B * c->run.args.L * CFD_LAT * 4;
  if (c->run.mode.tie && !c->run.mode.tie_final && c->run.pos == c->run.iters) {   // a finished tied run: the tie copy once more (mid-run reads: as stepped)
    const long long n8 = (long long)c->run.args.B * c->run.args.L * (CFD_LAT / 8);
    hipLaunchKernelGGL(tie_copy_kernel<>, dim3((unsigned)((n8 + 255) / 256)), dim3(256), 0, c->run.stream, c->run.latents.as<float>(),
                       c->run.etie.as<int32_t>(), n8);
    HIPCHK(hipGetLastError());
    c->run.mode.tie_final = true;
  }
  HIPCHK(hipMemcpyAsync(out, c->run.latents.p, lat_bytes, hipMemcpyDeviceToDevice, c->run.stream));
  HIPCHK(hipStreamSynchronize(c->run.stream));
  CHK(settle_deferred_census(c));
  // the census of everything the run's iterations counted (per-step projections of a dynamic memory, the three-launch cross-attention):
  // read on every read of a run whose captured iteration has such launches, BEFORE the run is closed -- a run that fails here stays open
  // and can be inspected or closed by the caller
  if (c->run.counts) CHK(check_saturation(c, "sampling run (the per-step projections of a memory)"));
  if (close) c->run.open = false;
  return CFD_OK;
}

// ---- stand-alone scheduler ops ----------------------------------------------------------------------------
extern "C" int cfd_scheduler_step_pred(cfd_handle c, int scheduler, const float* ac, int T, int n_inf, int t, int clip, float eta,
                                       int set_alpha_to_one, int prediction_type, const float* model_output, const float* noise,
                                       float* sample_inout, size_t numel, float* pred_original_sample, void* stream) {
  if (!c || !ac || !model_output || !sample_inout || t < 0 || t >= T || n_inf < 1) return fail(CFD_E_ARG, "bad argument");
  if (prediction_type != 0 && prediction_type != 1)
    return fail(CFD_E_ARG, "cfd_scheduler_step_pred: prediction_type = %d is not 0 (epsilon) or 1 (sample)", prediction_type);
  if (scheduler == 3 && prediction_type != 0)
    return fail(CFD_E_ARG, "cfd_scheduler_step_pred: DDIM inversion needs prediction_type = 0 (epsilon)");
  if (scheduler != 0 && scheduler != 1 && scheduler != 3)
    return fail(CFD_E_ARG, "cfd_scheduler_step[_pred]: scheduler must be 0 (DDPM), 1 (DDIM) or 3 (DDIM inversion); DPM-Solver++ steps go "
                           "through cfd_dpmsolver_step[_pred]");
  if (scheduler == 3 && (eta != 0.f || clip))
    return fail(CFD_E_ARG, "cfd_scheduler_step[_pred]: DDIM inversion needs eta = 0 and clip_sample = 0 (got %g, %d)", (double)eta, clip);
  HIPCHK(hipSetDevice(c->cfg.device));
  StepCoef k;
  memset(&k, 0, sizeof(k));
  if (scheduler == 0) ddpm_coef(ac, T, n_inf, t, &k);
  else if (scheduler == 3) ddim_inverse_coef(ac, T, n_inf, t, set_alpha_to_one, &k);
  else ddim_coef(ac, T, n_inf, t, eta, set_alpha_to_one, &k);
  if (k.use_noise != 0.f && !noise) return fail(CFD_E_ARG, "this step adds noise: pass the N(0,1) draw");
  const dim3 grid((unsigned)((numel + 255) / 256)), block(256);
  with_pred(prediction_type, [&](auto pred) {
    hipLaunchKernelGGL((sched_step_kernel<0, decltype(pred)::value>), grid, block, 0, (hipStream_t)stream, model_output, noise, sample_inout, numel, k,
                       scheduler, clip, pred_original_sample);
  });
  HIPCHK(hipGetLastError());
  return CFD_OK;
}

extern "C" int cfd_scheduler_step(cfd_handle c, int scheduler, const float* ac, int T, int n_inf, int t, int clip, float eta,
                                  int set_alpha_to_one, const float* model_output, const float* noise, float* sample_inout,
                                  size_t numel, float* pred_original_sample, void* stream) {
  return cfd_scheduler_step_pred(c, scheduler, ac, T, n_inf, t, clip, eta, set_alpha_to_one, 0, model_output, noise, sample_inout, numel,
                                 pred_original_sample, stream);
}

extern "C" int cfd_dpmsolver_step_pred(cfd_handle c, const float* ac, int T, int t, int prev_t, int t_prev_model, int prediction_type,
                                       const float* model_output, const float* m_prev, float* sample_inout, float* x0_out, size_t numel,
                                       void* stream) {
  if (!c || !ac || !model_output || !sample_inout || !x0_out) return fail(CFD_E_ARG, "null argument");
  if (prediction_type != 0 && prediction_type != 1)
    return fail(CFD_E_ARG, "cfd_dpmsolver_step_pred: prediction_type = %d is not 0 (epsilon) or 1 (sample)", prediction_type);
  if (t < 1 || t >= T || prev_t < 0 || prev_t >= t || t_prev_model >= T || (t_prev_model >= 0 && t_prev_model <= t))
    return fail(CFD_E_ARG, "cfd_dpmsolver_step[_pred]: need T > t_prev_model > t > prev_t >= 0 (t_prev_model = -1: first order), t >= 1 "
                           "(got %d, %d, %d, T = %d)", t_prev_model, t, prev_t, T);
  if (t_prev_model >= 0 && !m_prev) return fail(CFD_E_ARG, "a second-order step reads the previous step's x0: pass m_prev");
  HIPCHK(hipSetDevice(c->cfg.device));
  StepCoef k;
  dpmpp_coef(ac, t, prev_t, t_prev_model, &k);
  const dim3 grid((unsigned)((numel + 255) / 256)), block(256);
  with_pred(prediction_type, [&](auto pred) {
    hipLaunchKernelGGL((dpmpp_step_kernel<0, decltype(pred)::value>), grid, block, 0, (hipStream_t)stream, model_output, m_prev, sample_inout, x0_out,
                       numel, k);
  });
  HIPCHK(hipGetLastError());
  return CFD_OK;
}

extern "C" int cfd_dpmsolver_step(cfd_handle c, const float* ac, int T, int t, int prev_t, int t_prev_model, const float* model_output,
                                  const float* m_prev, float* sample_inout, float* x0_out, size_t numel, void* stream) {
  return cfd_dpmsolver_step_pred(c, ac, T, t, prev_t, t_prev_model, 0, model_output, m_prev, sample_inout, x0_out, numel, stream);
}

// ---- developer hook: the stride rule of cfd_sample_parallel, on the host (no handle, no device) --------------------------------------
extern "C" int cfd_test_picard_stride(const float* err, int B, int p, int i0, const float* coef, int N, float tolerance, int L) {
  if (!err || !coef || B < 1 || p < 1 || i0 < 0 || i0 + p > N || L < 1 || !(tolerance >= 0.f)) return fail(CFD_E_ARG, "bad argument");
  return picard_stride(err, B, p, i0, reinterpret_cast<const StepCoef*>(coef), tolerance, L);
}

// ---- developer hook: the kernels of a sweep around the forward, on the caller's predictions (include/cfdenoise_dev.h) ---------------
// The stages of cfd_sample_parallel's own PicardSweep, those the mask names; the partials start as NaN, so that a partial the scan did
// not write shows in err.
extern "C" int cfd_test_picard_sweep(cfd_handle c, const cfd_test_picard_args* t, void* stream) {
  if (!c || !t) return fail(CFD_E_ARG, "null argument");
  const int B = t->B, L = t->L, G = t->G, N = t->N, J = t->J, base = t->base, off = t->off;
  const bool do_fill = t->stages & CFD_PICARD_FILL, do_load = t->stages & CFD_PICARD_LOAD, do_step = t->stages & CFD_PICARD_STEP,
             do_scan = t->stages & CFD_PICARD_SCAN;
  if (!t->stages || (t->stages & ~15)) return fail(CFD_E_ARG, "cfd_test_picard_sweep: stages = %d", t->stages);
  if (!t->ring) return fail(CFD_E_ARG, "cfd_test_picard_sweep: the ring is NULL");
  if (B < 1 || L < 1 || G < 1 || G > 8 || N < 1 || J < 1) return fail(CFD_E_ARG, "cfd_test_picard_sweep: bad B / L / G / N / J");
  if (off < 0 || off >= J) return fail(CFD_E_ARG, "cfd_test_picard_sweep: off = %d is not in [0, J = %d)", off, J);
  if (base < 0 || base + J > N) return fail(CFD_E_ARG, "cfd_test_picard_sweep: the batch %d .. %d leaves the %d iterations", base, base + J - 1, N);
  if (t->slots < J + 1 || t->slots > N + 1) return fail(CFD_E_ARG, "cfd_test_picard_sweep: slots = %d is not in [J + 1, N + 1]", t->slots);
  const long long chunk = (long long)B * L * CFD_LAT, n8 = chunk / 8;
  if (n8 * std::max(J, t->slots) > (1ll << 30)) return fail(CFD_E_ARG, "cfd_test_picard_sweep: too many elements for one launch");
  if (do_fill && (t->fill_src < 0 || t->fill_src > N || t->fill_lo < 0 || t->fill_hi > N || t->fill_hi - t->fill_lo + 1 >= t->slots))
    return fail(CFD_E_ARG, "cfd_test_picard_sweep: fill %d -> %d .. %d", t->fill_src, t->fill_lo, t->fill_hi);
  if (do_load && !t->sample_sp) return fail(CFD_E_ARG, "cfd_test_picard_sweep: sample_sp is NULL");
  if (do_step) {
    if (!t->eps || !t->coef || !t->s) return fail(CFD_E_ARG, "cfd_test_picard_sweep: eps, coef or s is NULL");
    if (t->Gc < 1 || t->Gc > 8) return fail(CFD_E_ARG, "cfd_test_picard_sweep: Gc = %d", t->Gc);
    for (int k = 0; k < t->Gc; ++k)
      if (t->pos[k] < 0 || t->pos[k] >= G) return fail(CFD_E_ARG, "cfd_test_picard_sweep: pos[%d] = %d is not in [0, G = %d)", k, t->pos[k], G);
  }
  if (do_scan && (!t->s || !t->err)) return fail(CFD_E_ARG, "cfd_test_picard_sweep: s or err is NULL");
  HIPCHK(hipSetDevice(c->cfg.device));
  hipStream_t st = (hipStream_t)stream;
  PicardSweep sw(c, st, PicardRing{t->ring, t->slots, N, chunk}, B, L, G, J);
  DBuf coef, part;   // (a return in front of the wait frees them too: hipFree waits for the device)
  if (do_fill) CHK(sw.fill(t->fill_src, t->fill_lo, t->fill_hi));
  if (do_load) CHK(sw.load(base, (char*)t->sample_sp));
  sw.sa.s = t->s;
  if (do_step) {
    CHK(coef.ensure((size_t)N * sizeof(StepCoef)));
    HIPCHK(hipMemcpyAsync(coef.p, t->coef, (size_t)N * sizeof(StepCoef), hipMemcpyHostToDevice, st));
    PicardStepArgs& sa = sw.sa;
    sa.eps = t->eps; sa.coef = coef.as<StepCoef>();
    sa.g.Gc = t->Gc; sa.g.clip = t->clip; sa.g.wtab = t->wtab;
    for (int k = 0; k < 8; ++k) { sa.g.w[k] = t->w[k]; sa.g.pos[k] = k < t->Gc ? t->pos[k] : 0; }
    sa.noise = t->noise; sa.seed = t->seed; sa.utt0 = t->first_utterance;
    CHK(sw.step(base, off));
  }
  if (do_scan) {
    CHK(part.ensure(sw.part_bytes()));
    HIPCHK(hipMemsetAsync(part.p, 0xFF, sw.part_bytes(), st));
    CHK(sw.scan_err(base, off, part.as<float>(), t->err));
  }
  HIPCHK(hipStreamSynchronize(st));
  return CFD_OK;
}

// ---- developer hook: the per-iteration coefficient table a sampling run uploads, on the host (no handle, no device) ----------------
extern "C" int cfd_test_step_coefficients(int kind, const float* ac, int T, int n_inf, const int32_t* timesteps, int N, float eta,
                                          int set_alpha_to_one, float* out) {
  if (!ac || !timesteps || !out || kind < 0 || kind > 3 || T < 1 || N < 1 || n_inf < 1) return fail(CFD_E_ARG, "bad argument");
  std::vector<StepCoef> coef(N);
  CHK(step_coefficients(kind, ac, T, n_inf, timesteps, N, eta, set_alpha_to_one, coef.data()));
  memcpy(out, coef.data(), (size_t)N * sizeof(StepCoef));
  return CFD_OK;
}

extern "C" int cfd_add_noise(cfd_handle c, const float* ac, int t, const float* original, const float* noise, float* out,
                             size_t numel, void* stream) {
  if (!c || !ac || !original || !noise || !out || t < 0) return fail(CFD_E_ARG, "bad argument");
  HIPCHK(hipSetDevice(c->cfg.device));
  const float sa = sqrtf(ac[t]), sb = sqrtf(1.0f - ac[t]);
  hipLaunchKernelGGL(add_noise_kernel<>, dim3((unsigned)((numel + 255) / 256)), dim3(256), 0, (hipStream_t)stream, original, noise, out,
                     numel, sa, sb);
  HIPCHK(hipGetLastError());
  return CFD_OK;
}

int enqueue_philox_fill(float* out, int B, int per_utt, uint64_t seed, uint32_t step, uint32_t utt0, uint32_t stream_id, float scale, hipStream_t st) {
  const long long n = (long long)B * per_utt / 4;
  hipLaunchKernelGGL(philox_fill_kernel<>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, out, B, per_utt, seed, step, utt0, stream_id, scale);
  hipError_t e = hipGetLastError();
  return e == hipSuccess ? CFD_OK : fail(CFD_E_HIP, "philox_fill_kernel launch failed: %s", hipGetErrorString(e));
}

extern "C" int cfd_philox_normal(cfd_handle c, float* out, int B, int per_utt, uint64_t seed, uint32_t step, uint32_t first_utt,
                                 uint32_t stream_id, void* stream) {
  if (!c || !out || B < 1 || per_utt < 4 || per_utt % 4) return fail(CFD_E_ARG, "bad argument");
  HIPCHK(hipSetDevice(c->cfg.device));
  return enqueue_philox_fill(out, B, per_utt, seed, step, first_utt, stream_id, 1.0f, (hipStream_t)stream);
}

extern "C" int cfd_sample_inpaint(cfd_handle c) {
  if (!c) return fail(CFD_E_ARG, "null handle");
  if (!c->run.open) return fail(CFD_E_STATE, "no sampling run open");
  const cfd_sample_args& s = c->run.args;
  // a tied, edit or anchored run: that instance does the tied / kept tokens of this iteration (one thread = 8 elements of any token), then
  // the captured iteration skips its overwrite; the default instance: the preseq tokens, if the run has any
  const bool by_token = c->run.mode.tie || c->run.mode.edit || c->run.mode.anchor;
  if (by_token && c->run.pos >= c->run.iters) return fail(CFD_E_STATE, "cfd_sample_inpaint: the run has no iteration left");
  if (!by_token && (!s.preseq || s.preseq_len < 1)) return CFD_OK;
  HIPCHK(hipSetDevice(c->cfg.device));
  const long long n = by_token ? (long long)s.B * s.L * (CFD_LAT / 8) : (long long)s.B * s.preseq_len * CFD_LAT;
  return with_begin_args(c, [&](auto a) {
    hipLaunchKernelGGL(BeginInst<decltype(a)>::inpaint_now, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, c->run.stream, a,
                       c->w->d_step.as<int>());
    HIPCHK(hipGetLastError());
    return (int)CFD_OK;
  });
}

extern "C" int cfd_sample_write(cfd_handle c, const float* latents) {
  if (!c || !latents) return fail(CFD_E_ARG, "null argument");
  if (!c->run.open) return fail(CFD_E_STATE, "no sampling run open");
  if (c->run.args.scheduler == 3) return fail(CFD_E_ARG, "cfd_sample_write: a DDIM inversion run takes no WEG update (its latents are its own)");
  if (c->run.mode.replay) return fail(CFD_E_ARG, "cfd_sample_write: the replay of a noise space takes no WEG update (its noise was solved for the recorded levels)");
  HIPCHK(hipSetDevice(c->cfg.device));
  const size_t lat_bytes = (size_t)c->run.args.B * c->run.args.L * CFD_LAT * 4;
  HIPCHK(hipMemcpyAsync(c->run.latents.p, latents, lat_bytes, hipMemcpyDeviceToDevice, c->run.stream));
  HIPCHK(hipStreamSynchronize(c->run.stream));
  return CFD_OK;
}

