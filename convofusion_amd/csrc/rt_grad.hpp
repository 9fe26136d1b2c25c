// The row-tile gradient engine: the forward with saved activations (rowtile.hpp) and the reverse sweep (rowtile_bwd.hpp) of small
// problems, and the protocol its callers follow.  Three entry points run on it, each with its own seed of the sweep:
//   cfd_weg_eval (cfd_weg.hip, weg_rt.hpp)        at the text maps, from the word-excitation objective (FOR_WEG); cfd_weg_step is the
//                                                 same caller with a per-row objective and its own update behind the sweep
//   cfd_denoise_vjp / cfd_denoise_vjp_mem         at the forward's output, from the caller's cotangent; _mem adds the gradient at the
//                                                 memories (MemGrad: three launches per layer behind B5 and one at the end) (FOR_VJP)
//   cfd_denoise_guide (guide.hpp)                 at the forward's output, from the key-pose loss (FOR_GUIDE)
// They share a workspace (Ctx::wk[1]: a call runs between two replays of an open sampling run's captured graph), the arena and
// GradState, and reuse nothing of one another.  A call is: check_* (every refusal, nothing touched) -> begin_call -> the caller's
// enqueue (WorkGuard, begin_sequence, launches only) -> finish_call (cfd_weg_eval: its own delivery).
// Included by cfd_grad.hip alone, so that every kernel of rowtile_bwd.hpp is compiled in one unit; what cfd_weg.hip calls has external
// linkage and is declared in cfd_internal.hpp (namespace rtgrad there: WorkGuard, Call, SweepSeed and the caller tags as well).
#pragma once

namespace rtgrad {

// A memory set's signature, appended to `v`: per memory S, the data pointer and the mask pointer.  Part of everything that decides
// whether a call may reuse what the previous one left (Call::sig, prepare's signature, cfd_weg_eval's graph key).
void append_memories(std::vector<long long>& v, const cfd_memory* mem) {
  for (int j = 0; j < CFD_NMEM; ++j) {
    v.push_back(mem[j].S);
    v.push_back((long long)(size_t)mem[j].data);
    v.push_back((long long)(size_t)mem[j].key_padding_mask);
  }
}

// The row-map part of a caller's Call::more: per memory U | row_map | the map's contents as the host sees them.
static void append_row_maps(std::vector<long long>& v, const cfd_memory* mem, const HostMaps& hm) {
  for (int j = 0; j < CFD_NMEM; ++j) {
    v.push_back(mem[j].U);
    v.push_back((long long)(size_t)mem[j].row_map);
    if (mem[j].row_map) v.insert(v.end(), hm.m[j].begin(), hm.m[j].end());
  }
}

static int padded_keys(const cfd_memory* mem) {   // of all five memories together, each padded to 32
  int sp = 0;
  for (int j = 0; j < CFD_NMEM; ++j) sp += (mem[j].S + 31) / 32 * 32;
  return sp;
}

// Why B rows of L tokens against these memories cannot run on the row-tile path -- the limit that is exceeded, in a buffer of the
// calling thread's -- or null when they can.  guide: the caller is cfd_denoise_guide, whose row limit is guide_max_rows (the one
// place where a call's row limit is named; decide_forward_path takes the same figure through PathAsk::max_rows).
const char* ineligible(Ctx* c, long long B, int L, const cfd_memory* mem, bool guide) {
  static thread_local char why[160];
  const int keys = padded_keys(mem);
  const long long max_rows = guide ? c->guide_max_rows : c->rt_max_rows;
  if (!c->rt_on || !c->weg_rt_on) snprintf(why, sizeof(why), "the row-tile path is switched off on this handle (CFD_ROWTILE / CFD_WEG_ROWTILE)");
  else if (L > RT_MAX_L) snprintf(why, sizeof(why), "L = %d exceeds RT_MAX_L = %d tokens per batch row", L, RT_MAX_L);
  else if (B * L > max_rows) snprintf(why, sizeof(why), "Be * L = %lld token rows exceed %s = %lld", B * L, guide ? "guide_max_rows" : "rt_max_rows", max_rows);
  else if (keys > RT_MAX_KEYS) snprintf(why, sizeof(why), "%d padded keys of the five memories together exceed RT_MAX_KEYS = %d", keys, RT_MAX_KEYS);
  else return nullptr;
  return why;
}

// (Re)build the call's problem and arena when the caller, shapes or pointers change.  Host work only (allocations, row maps): never
// captured.  FOR_WEG keeps the text maps (att) for the objective; FOR_VJP and FOR_GUIDE keep none, run the whole network and leave
// d_att zero: the sweep's kernels add it to the text memory's dP as they are.  FOR_GUIDE asks the path decision for its own row limit
// (guide_max_rows, PathAsk::max_rows).  T: the rows of the per-timestep tables.
static int prepare(Ctx* c, const Call& k, int T, hipStream_t st) {
  RtGradState& s = c->grad.rt;
  const int who = k.who, B = k.Be, L = k.L;
  const cfd_memory* mem_in = k.mem;
  const HostMaps* maps = k.maps;
  const int nl = c->nl, spt = padded_keys(mem_in);
  std::vector<long long> sig = {who, B, L, nl, T};
  append_memories(sig, mem_in);
  sig.insert(sig.end(), k.more.begin(), k.more.end());
  if (sig == s.sig) return CFD_OK;
  HIPCHK(hipStreamSynchronize(st));
  s.sig.clear();
  const size_t M = (size_t)B * L, St = (size_t)mem_in[2].S;
  const size_t n_x = M * CFD_D, n_vt = (size_t)B * CFD_D * RT_MAX_L, n_sc = M * spt, n_pre = M * CFD_FF, n_att = (size_t)B * nl * L * St;
  size_t vt_floats = 0, att_floats = 0;   // what the memsets below clear: the buffers with their granule's padding
  CHK(carve(c->grad.rt_ws, 64, [&](ArenaLayout& a) {   // 64 floats: 256-byte granules
    for (int l = 0; l <= nl; ++l)
      for (int k = 0; k < 5; ++k) a.take(s.sv.x[l][k], n_x);
    for (int l = 0; l < nl; ++l) {
      a.take(s.sv.qk[l], M * 2 * CFD_D); a.take(s.sv.vt[l], n_vt); a.take(s.sv.sc[l], n_sc); a.take(s.sv.cst[l], M * 32 * 4); a.take(s.sv.pre[l], n_pre);
    }
    a.take(s.att, n_att); a.take(s.d_att, n_att); a.take(s.fws, (size_t)B * (3 * (size_t)L * St + 3 * St + 64)); a.take(s.dP, n_sc);
    for (int k = 0; k < 3; ++k) a.take(s.G[k], n_x);
    a.take(s.dz, n_x); a.take(s.dy, n_x); a.take(s.dh, n_pre); a.take(s.dO, n_x); a.take(s.dqkv, M * 3 * CFD_D);
    vt_floats = a.rounded(n_vt); att_floats = a.rounded(n_att);
  }));
  for (int l = 0; l < nl; ++l) HIPCHK(hipMemset(s.sv.vt[l], 0, vt_floats * 4));   // keys beyond L stay zero
  s.sv.whole = who != FOR_WEG;
  if (who != FOR_WEG) HIPCHK(hipMemset(s.d_att, 0, att_floats * 4));
  {
    WorkGuard guard(c);
    cfd_memory mem[CFD_NMEM];
    float* att[CFD_NMEM] = {nullptr, nullptr, who == FOR_WEG ? s.att : nullptr, nullptr, nullptr};
    for (int j = 0; j < CFD_NMEM; ++j) mem[j] = mem_in[j];
    PathAsk ask;
    ask.att_out = who == FOR_WEG;
    ask.max_rows = who == FOR_GUIDE ? c->guide_max_rows : 0;
    CHK(setup_problem(c, B, L, mem, maps, att, ask, 0, T));
    if (T > 1) {   // full tables: row t belongs to timestep t
      std::vector<int32_t> iota(T);
      for (int t = 0; t < T; ++t) iota[t] = t;
      HIPCHK(hipMemcpy(c->w->trows.p, iota.data(), (size_t)T * 4, hipMemcpyHostToDevice));
    }
    if (!c->w->pb.path.rt) return fail(CFD_E_STATE, "row-tile evaluation: the problem does not qualify for the row-tile path");
  }
  s.sig = sig;
  return CFD_OK;
}

// What a call does first: the forward's hints lapse, the census an earlier evaluation left is settled, and the handle's own stream --
// capturable, and the one an open run's graph replays on: the two serialise -- starts behind whatever the caller has queued on its
// stream.  (On its own: cfd_weg_eval on the float32 launch sequence, which prepares nothing here.)
int begin_on_own_stream(Ctx* c, hipStream_t caller) {
  c->hint_now = c->hint_same_mem = false;
  CHK(settle_deferred_census(c));
  HIPCHK(hipEventRecord(c->grad.ev, caller));
  HIPCHK(hipStreamWaitEvent(c->own_stream, c->grad.ev, 0));
  return CFD_OK;
}

// The call's timestep, in front of its launch sequence and outside any captured graph: one-row tables (T == 1) are built for it, full
// tables (row t = timestep t) are read at it.
static int set_call_timestep(Ctx* c, int T, int timestep, hipStream_t st) {
  GradState& w = c->grad;
  w.rt.T = T;
  w.t_host = timestep;
  w.dstep_host = T > 1 ? timestep : 0;
  if (T == 1) HIPCHK(hipMemcpyAsync(c->wk[1].trows.p, &w.t_host, 4, hipMemcpyHostToDevice, st));
  HIPCHK(hipMemcpyAsync(c->wk[1].d_step.p, &w.dstep_host, 4, hipMemcpyHostToDevice, st));
  return CFD_OK;
}

// The table rows for Call::mode, wk[1]'s problem and the arena, the call's timestep, its signature and whether that is the one the
// previous call left.  The signature is what the memory-side / time-only launches depend on; with mode != 0 the caller states that
// the memories' CONTENTS are unchanged too, and those launches are skipped: 1 = same timestep as well (a refinement loop at one
// timestep), 2 = the timestep may differ (a guided sampling loop: one call per iteration, same conditioning), served from tables over
// ALL timesteps, built at the first such call (row t = timestep t, one launch per call copies the row).  A caller other than
// cfd_weg_eval appends itself and `more`, so that no caller's signature equals another's.
static int prepare_and_decide(Ctx* c, Call& k, hipStream_t st) {
  GradState& w = c->grad;
  // tables over all timesteps stay while the caller keeps stating that the conditioning is unchanged
  const int T = k.mode == 2 || (k.mode == 1 && w.rt.T > 1) ? c->tsin_rows : 1;
  CHK(prepare(c, k, T, st));
  k.sig = {k.Be, k.L};
  append_memories(k.sig, k.mem);   // (prepare rebuilds the problem when a mask pointer changes: no reuse then)
  k.sig.insert(k.sig.end(), {(long long)(size_t)w.rt_ws.p, -(long long)T});
  if (T == 1) k.sig.push_back(k.timestep);
  if (k.who != FOR_WEG) {
    k.sig.push_back(k.who);
    k.sig.insert(k.sig.end(), k.more.begin(), k.more.end());
  }
  k.reuse = k.mode != 0 && k.sig == w.sig;
  return set_call_timestep(c, T, k.timestep, st);
}

// The one way into a call, behind the caller's check_* (a refusal there touches nothing: the previous call's state survives it).
// The call overwrites wk[1]'s problem and tables and the arena, so a caller other than cfd_weg_eval first drops the captured
// evaluations, whose arguments hold addresses that set-up may move; and whatever becomes of this call, the signature the previous one
// left is gone behind it: a call that fails leaves nothing to reuse (finish_call stores the new one).
int begin_call(Ctx* c, Call& k, hipStream_t caller) {
  hipStream_t st = c->own_stream;
  CHK(begin_on_own_stream(c, caller));
  if (k.who != FOR_WEG)
    for (WegState::Graph& g : c->weg.graph)
      if (g.gx.exec) { HIPCHK(hipStreamSynchronize(st)); g.reset(); }
  const int r = prepare_and_decide(c, k, st);
  c->grad.sig.clear();
  return r;
}

// The counter and shape preamble of a launch sequence, under the caller's WorkGuard.
void begin_sequence(Ctx* c) {
  RtGradState& s = c->grad.rt;
  const Problem& p = c->w->pb;
  s.launches = 0;
  s.stop_gi = -1;
  s.B = p.Be; s.L = p.L; s.Sp_tot = p.Sp_tot; s.St = p.S[2];
  s.focus_large = 0;
}

// The end of a call that returns with its results complete (`r`: what its enqueue returned): its census is read here, so a clamped
// sample or memory fails THIS call.  sig: Call::sig of a call that leaves its memory side for reuse, null of one that keeps nothing.
static int finish_call(Ctx* c, int r, const char* what, const std::vector<long long>* sig = nullptr) {
  HIPCHK(hipStreamSynchronize(c->own_stream));
  CHK(r);
  CHK(check_saturation(c, what));
  if (sig) c->grad.sig = *sig;
  return CFD_OK;
}

template <int PRO, int EPI, int MAXSTEP>
static int bwd_gemm(Ctx* c, hipStream_t st, const RtBwdArgs& a, int N, int ntile) {
  static unsigned long long attr_done = 0;
  CHK(once_per_device(attr_done, c->cfg.device, [&]() -> int {
    HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void*>(&rt_bwd_gemm_kernel<PRO, EPI, MAXSTEP>), hipFuncAttributeMaxDynamicSharedMemorySize,
                               rt_bwd_gemm_lds(MAXSTEP * 32)));
    return CFD_OK;
  }));
  if (a.K != MAXSTEP * 32) return fail(CFD_E_ARG, "backward product: K = %d does not match the kernel instance (%d)", a.K, MAXSTEP * 32);
  LAUNCH_COUNTED(c->grad.rt.launches, (rt_bwd_gemm_kernel<PRO, EPI, MAXSTEP>), dim3(N / 16, ntile), dim3(512), rt_bwd_gemm_lds(a.K), st, a);
  return CFD_OK;
}

// The launches "weg.info" reports for the callees that do not count their own:
//   enqueue_time_tables (cfd_problem.hip): two products of the time embedding + one per time block, two blocks per layer;
//   prepare_static_memside (cfd_problem.hip): per memory mem_center_kernel, the two folded products (enqueue_mem_kv), the two table
//     products (kbtab, vbtab) and mem_scale_table_kernel, + temb_center_kernel + 1.  (The callee also fills a scale plane per memory;
//     the figure is compared between trees and stays what it has always been.)
//   to_split_kernel + enqueue_rows_rt with saved activations (cfd_forward.hip): the embedding + nine launches per layer, less the
//     three of the top layer behind its cross-attention; the whole network (cfd_denoise_vjp) has them and the latent projection.
static int memory_side_launches(int nl) { return (2 + 2 * nl) + (6 * CFD_NMEM + 2); }
static int forward_launches(int nl, bool whole = false) { return whole ? 1 + 1 + 9 * nl + 1 : 1 + 1 + 9 * nl - 3; }

// [time tables + memory side]: what an evaluation that reuses the memory side skips
int enqueue_memory_side(Ctx* c, hipStream_t st) {
  Work* w = c->w;
  w->tt_key.clear();     // (this workspace's timestep-only tables are rebuilt from w->trows, whatever they held: cfd_problem.hip, build_time_tables)
  w->tt_mem_mask = 0;
  CHK(enqueue_time_tables(c, w->pb.T, st));      // one row: the timestep index is in w->trows (copied in front of the launch sequence); full tables: row t = timestep t
  CHK(prepare_static_memside(c, st));
  if (!w->pb.path.rt) return fail(CFD_E_STATE, "row-tile WEG evaluation lost its path");
  c->grad.rt.launches += memory_side_launches(c->nl);
  return CFD_OK;
}

// forward with saved activations (rowtile.hpp) from `latents` [M][128]
int enqueue_forward_saved(Ctx* c, hipStream_t st, const float* latents) {
  RtGradState& s = c->grad.rt;
  Work* w = c->w;
  const long long M = w->pb.M, n = M * (CFD_LAT / 8);
  hipLaunchKernelGGL(to_split_kernel<>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, latents, w->sample_sp.as<char>(), M, CFD_LAT,
                     (long long)CFD_LAT, (long long)CFD_LAT * 4, c->sat_in());
  HIPCHK(hipGetLastError());
  CHK(enqueue_rows_rt(c, st, &s.sv));
  s.launches += forward_launches(c->nl, s.sv.whole);
  return CFD_OK;
}

// What cfd_denoise_vjp_mem adds to the sweep: the gradient at the memories of `want`, d_mem[j] [U_j][S_j][512].
// Per layer, behind B5 (its EMIT instance leaves dS' and P'): T = LayerNorm2(x) . A and G = gn . VV over the span of wanted memories
// (two launches of rt_bwd_gemm_kernel against the float32 folded weights), then the key-side accumulation into the memories' planes
// (rt_xbwd_dn_kernel); behind the last layer one launch takes the planes through the memory LayerNorm (rt_mem_ln_bwd_kernel).
struct MemGrad {
  bool want[CFD_NMEM];
  int j0 = 0, nspan = 0;              // the wanted memories lie in [j0, j0 + nspan)
  float *dSp = nullptr, *Pp = nullptr, *T = nullptr, *G = nullptr, *plane[CFD_NMEM];
  const int *inv_off[CFD_NMEM], *inv_rows[CFD_NMEM];
  float* d_mem[CFD_NMEM];
};

// Float32 copies of the folded A, c and VV, unscaled, by the float64 fold of cfd_finalize_weights (cfd_core.hip) -- made when a
// memory gradient is first asked for, and again after the weights changed.  Host work and set-up launches: never per call.
static int ensure_memw_f32(Ctx* c, hipStream_t st) {
  GradState& w = c->grad;
  if (w.memw_wver == c->wver) return CFD_OK;
  const int nl = c->nl, D = CFD_D;
  const long long LD = (long long)CFD_NMEM * D;
  HIPCHK(hipStreamSynchronize(st));
  CHK(w.memw_a.ensure((size_t)nl * D * LD * 4));
  CHK(w.memw_v.ensure((size_t)nl * D * LD * 4));
  CHK(w.memw_c.ensure((size_t)nl * LD * 4));
  DBuf tmpd;
  CHK(tmpd.ensure((size_t)D * D * 8));
  const dim3 blk(256);
  auto grid1 = [](long long n) { return dim3((unsigned)((n + 255) / 256)); };
  const double cs = std::sqrt(1.0 / (double)D);
  for (int l = 0; l < nl; ++l) {
    const std::string p = "decoder.layers." + std::to_string(l) + ".";
    const float* fw = rawp(c, p + "att_fuser.weight");
    if (!fw) return fail(CFD_E_STATE, "missing tensor '%satt_fuser.weight'", p.c_str());
    for (int j = 0; j < CFD_NMEM; ++j) {
      const std::string a = p + "multihead_attn_" + MEM_NAMES[j];
      const float *ipw = rawp(c, a + ".in_proj_weight"), *ipb = rawp(c, a + ".in_proj_bias"), *ow = rawp(c, a + ".out_proj.weight");
      const float* gam = rawp(c, p + MEM_NAMES[j] + "_norm.weight");
      if (!ipw || !ipb || !ow || !gam) return fail(CFD_E_STATE, "missing tensor of '%s'", a.c_str());
      const float *Wq = ipw, *Wk = ipw + (size_t)D * D, *Wv = ipw + (size_t)2 * D * D, *bq = ipb;
      float* A = w.memw_a.as<float>() + (size_t)l * D * LD + (size_t)j * D;
      float* V = w.memw_v.as<float>() + (size_t)l * D * LD + (size_t)j * D;
      // A[o][i] = cs gamma[i] sum_r Wq[r][o] Wk[r][i];  c[i] = cs gamma[i] sum_r Wk[r][i] bq[r];  VV = Wf_j Wo Wv diag(gamma)
      hipLaunchKernelGGL((fold_mm_kernel<float, float, float>), grid1((long long)D * D), blk, 0, st, Wq, 1LL, (long long)D, Wk, (long long)D, 1LL, A, LD, D, D,
                         D, cs, gam);
      hipLaunchKernelGGL((fold_mv_kernel<float, float, float>), grid1(D), blk, 0, st, Wk, 1LL, (long long)D, bq, (const double*)nullptr,
                         (const float*)nullptr, w.memw_c.as<float>() + ((size_t)l * CFD_NMEM + j) * D, D, D, cs, gam);
      hipLaunchKernelGGL((fold_mm_kernel<float, float, double>), grid1((long long)D * D), blk, 0, st, ow, (long long)D, 1LL, Wv, (long long)D, 1LL,
                         tmpd.as<double>(), (long long)D, D, D, D, 1.0, (const float*)nullptr);
      hipLaunchKernelGGL((fold_mm_kernel<float, double, float>), grid1((long long)D * D), blk, 0, st, fw + (size_t)j * D, (long long)5 * D, 1LL,
                         tmpd.as<double>(), (long long)D, 1LL, V, LD, D, D, D, 1.0, gam);
      HIPCHK(hipGetLastError());
    }
  }
  HIPCHK(hipStreamSynchronize(st));   // (tmpd leaves scope)
  w.memw_wver = c->wver;
  return CFD_OK;
}

// The call's planes and the inverse row maps (host work: allocations and one upload; in front of the launches).
static int prepare_mem_grad(Ctx* c, hipStream_t st, int Be, int L, const cfd_memory* mem, const HostMaps& hm, float* const d_mem[CFD_NMEM], MemGrad& mg) {
  GradState& w = c->grad;
  const size_t M = (size_t)Be * L, spt = (size_t)padded_keys(mem);
  int j1 = -1;
  mg.j0 = CFD_NMEM;
  for (int j = 0; j < CFD_NMEM; ++j) {
    mg.want[j] = d_mem[j] != nullptr;
    mg.d_mem[j] = d_mem[j];
    if (mg.want[j]) { mg.j0 = std::min(mg.j0, j); j1 = j; }
  }
  mg.nspan = j1 - mg.j0 + 1;
  CHK(carve(w.mem_ws, 64, [&](ArenaLayout& a) {
    const size_t n_sp = M * spt, n_t = M * (size_t)mg.nspan * CFD_D;
    a.take(mg.dSp, n_sp); a.take(mg.Pp, n_sp); a.take(mg.T, n_t); a.take(mg.G, n_t);
    for (int j = 0; j < CFD_NMEM; ++j) {
      mg.plane[j] = nullptr;
      if (mg.want[j]) a.take(mg.plane[j], (size_t)mem[j].U * ((mem[j].S + 31) / 32 * 32) * CFD_D);
    }
  }));
  // inverse row maps: per memory [U_j + 1] offsets, then the Be rows by instance (ascending within an instance)
  std::vector<int32_t> inv;
  size_t at[CFD_NMEM];
  for (int j = 0; j < CFD_NMEM; ++j) {
    at[j] = inv.size();
    const int U = mem[j].U;
    std::vector<int32_t> cnt((size_t)U + 1, 0);
    for (int b = 0; b < Be; ++b) ++cnt[(size_t)hm.m[j][b] + 1];
    for (int u = 0; u < U; ++u) cnt[(size_t)u + 1] += cnt[u];
    inv.insert(inv.end(), cnt.begin(), cnt.end());
    for (int u = 0; u < U; ++u)
      for (int b = 0; b < Be; ++b)
        if (hm.m[j][b] == u) inv.push_back(b);
  }
  if (inv.size() * 4 > w.mem_inv.bytes || inv != w.mem_inv_host) {
    HIPCHK(hipStreamSynchronize(st));
    CHK(w.mem_inv.ensure(inv.size() * 4));
    HIPCHK(hipMemcpy(w.mem_inv.p, inv.data(), inv.size() * 4, hipMemcpyHostToDevice));
    w.mem_inv_host = inv;
  }
  for (int j = 0; j < CFD_NMEM; ++j) {
    mg.inv_off[j] = w.mem_inv.as<int>() + at[j];
    mg.inv_rows[j] = mg.inv_off[j] + mem[j].U + 1;
  }
  return CFD_OK;
}

// the three launches of one layer behind its B5: T, G, the key-side accumulation
static int enqueue_mem_grad_layer(Ctx* c, hipStream_t st, const MemGrad& mg, int l, bool first, const RtBwdArgs& base, const float* gn, int ntile) {
  RtGradState& s = c->grad.rt;
  const Problem& p = c->w->pb;
  const LayerW& lw = c->lw[l];
  const long long LD = (long long)CFD_NMEM * CFD_D;
  const int ldt = mg.nspan * CFD_D;
  {   // T = LayerNorm2(x) . A_j for the memories of the span
    RtBwdArgs a = base;
    a.K = CFD_D; a.x = s.sv.x[l][2]; a.gamma = lw.ln2g; a.beta = lw.ln2b;
    a.w = c->grad.memw_a.as<float>() + (size_t)l * CFD_D * LD + (size_t)mg.j0 * CFD_D; a.ldw = LD; a.out = mg.T; a.ldo = ldt;
    CHK((bwd_gemm<RT_BPRO_LNFWD, RT_BEPI_F32, 16>(c, st, a, ldt, ntile)));
  }
  {   // G = gn . VV_j
    RtBwdArgs a = base;
    a.K = CFD_D; a.a = gn;
    a.w = c->grad.memw_v.as<float>() + (size_t)l * CFD_D * LD + (size_t)mg.j0 * CFD_D; a.ldw = LD; a.out = mg.G; a.ldo = ldt;
    CHK((bwd_gemm<RT_BPRO_ROWS, RT_BEPI_F32, 16>(c, st, a, ldt, ntile)));
  }
  RtXDnArgs d;
  memset(&d, 0, sizeof(d));
  d.L = p.L; d.Sp_tot = p.Sp_tot; d.ldt = ldt; d.first = first ? 1 : 0;
  d.dSp = mg.dSp; d.Pp = mg.Pp; d.T = mg.T; d.G = mg.G;
  int nwg = 0;
  for (int j = 0; j < CFD_NMEM; ++j) {
    d.cvec[j] = c->grad.memw_c.as<float>() + ((size_t)l * CFD_NMEM + j) * CFD_D;
    d.plane[j] = mg.plane[j]; d.inv_off[j] = mg.inv_off[j]; d.inv_rows[j] = mg.inv_rows[j];
    d.Sp[j] = p.Sp[j]; d.off[j] = p.off[j]; d.tcol[j] = (j - mg.j0) * CFD_D;
    d.blk0[j] = nwg;
    if (mg.want[j]) nwg += p.U[j] * (p.Sp[j] / 16);
  }
  d.blk0[CFD_NMEM] = nwg;
  LAUNCH_COUNTED(s.launches, rt_xbwd_dn_kernel<>, dim3(nwg), dim3(512), 0, st, d);
  return CFD_OK;
}

// behind the last layer: the planes through the memory LayerNorm into d_mem
static int enqueue_mem_grad_finish(Ctx* c, hipStream_t st, const MemGrad& mg) {
  const Problem& p = c->w->pb;
  RtMemLnArgs a;
  memset(&a, 0, sizeof(a));
  a.cond = rawp(c, "condition_embedding.weight"); a.pe = rawp(c, "mem_pos.pe");
  a.temb = c->w->temb_tab.as<float>();            // (one-row tables: this call's timestep)
  int rows = 0;
  for (int j = 0; j < CFD_NMEM; ++j) {
    a.raw[j] = p.mem[j]; a.plane[j] = mg.plane[j]; a.dmem[j] = mg.d_mem[j]; a.S[j] = p.S[j]; a.Sp[j] = p.Sp[j];
    a.row0[j] = rows;
    if (mg.want[j]) rows += p.U[j] * p.S[j];
  }
  a.row0[CFD_NMEM] = rows;
  LAUNCH_COUNTED(c->grad.rt.launches, rt_mem_ln_bwd_kernel<>, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, st, a);
  return CFD_OK;
}

// reverse sweep (rowtile_bwd.hpp): B1 .. B9 per layer from the top, then the embedding's backward into `grad`.
// mg (cfd_denoise_vjp_mem): B5 is its EMIT instance and three launches per layer follow it (enqueue_mem_grad_layer), one more the
// last layer; `grad` may then be null, which skips the embedding's backward alone.  Without mg the launches are what they always were.
int enqueue_reverse_sweep(Ctx* c, hipStream_t st, const SweepSeed& seed, float* grad, const MemGrad* mg) {
  RtGradState& s = c->grad.rt;
  Work* w = c->w;
  const Problem& p = w->pb;
  const int nl = c->nl, B = s.B, L = s.L, tpr = (L + 15) / 16, ntile = B * tpr;
  s.dy_keys = p.Sp_tot <= 512 ? 512 : RT_MAX_KEYS;
  const auto dy_kernel = mg ? (s.dy_keys == 512 ? rt_xbwd_dy_kernel<512, true> : rt_xbwd_dy_kernel<RT_MAX_KEYS, true>)
                            : (s.dy_keys == 512 ? rt_xbwd_dy_kernel<512> : rt_xbwd_dy_kernel<RT_MAX_KEYS>);
  static unsigned long long attr_done = 0;
  CHK(once_per_device(attr_done, c->cfg.device, [&]() -> int {
    HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void*>(&rt_xbwd_dy_kernel<512>), hipFuncAttributeMaxDynamicSharedMemorySize, rt_xbwd_dy_lds(512)));
    HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void*>(&rt_xbwd_dy_kernel<RT_MAX_KEYS>), hipFuncAttributeMaxDynamicSharedMemorySize,
                               rt_xbwd_dy_lds(RT_MAX_KEYS)));
    HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void*>(&rt_selfattn_bwd_kernel<>), hipFuncAttributeMaxDynamicSharedMemorySize, rt_selfattn_bwd_lds()));
    return CFD_OK;
  }));
  if (mg) {
    static unsigned long long emit_attr_done = 0;
    CHK(once_per_device(emit_attr_done, c->cfg.device, [&]() -> int {
      HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void*>(&rt_xbwd_dy_kernel<512, true>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                 rt_xbwd_dy_lds(512)));
      HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void*>(&rt_xbwd_dy_kernel<RT_MAX_KEYS, true>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                 rt_xbwd_dy_lds(RT_MAX_KEYS)));
      return CFD_OK;
    }));
  }
  RtBwdArgs base;
  memset(&base, 0, sizeof(base));
  base.L = L; base.tpr = tpr;
  RtXBwdArgs xb;
  memset(&xb, 0, sizeof(xb));
  xb.L = L; xb.tpr = tpr; xb.nl = nl; xb.Sp_tot = p.Sp_tot;   // (this step's table rows: Work::now_*, set by the forward)
  xb.rsp = w->p_sp.as<float>(); xb.d_att = s.d_att; xb.dP = s.dP; xb.dy = s.dy;
  if (mg) { xb.dSp = mg->dSp; xb.Pp = mg->Pp; }
  int nkb = 0;
  for (int j = 0; j < CFD_NMEM; ++j) {
    xb.map[j] = p.map[j]; xb.S[j] = p.S[j]; xb.Sp[j] = p.Sp[j]; xb.off[j] = p.off[j];
    xb.blk0[j] = nkb; nkb += p.Sp[j] / 16;
    memcpy(xb.inst[j], p.rt_inst[j], RT_ARG_ROWS);
  }
  xb.blk0[CFD_NMEM] = nkb;
  xb.use_inst = p.rt_use_inst;
  auto Wraw = [&](int l, const char* name) -> const float* { return rawp(c, "decoder.layers." + std::to_string(l) + "." + name); };
  int gi = 0;                 // G[gi] holds the running gradient (valid once have_g)
  bool have_g = false;
  const float* dy1 = nullptr; // gradient at the next layer's norm1 output (the top layer under an output seed: at decoder.norm's)
  if (seed.d_out) {           // d_out . latent_proj.weight
    RtBwdArgs a = base;
    a.K = CFD_LAT; a.a = seed.d_out; a.w = rawp(c, "latent_proj.weight"); a.ldw = CFD_D; a.out = s.dy; a.ldo = CFD_D;
    CHK((bwd_gemm<RT_BPRO_ROWS, RT_BEPI_F32, CFD_LAT / 32>(c, st, a, CFD_D, ntile)));
    dy1 = s.dy;
  }
  // test hook (cfd_debug_weg_stop): leave behind launch B<k> of layer l, remembering where the running gradient is
#define WEG_STOP_AT(k) do { if (s.stop == 16 * l + (k)) { s.stop_gi = have_g ? gi : -1; return CFD_OK; } } while (0)
  for (int l = nl - 1; l >= 0; --l) {
    const LayerW& lw = c->lw[l];
    RtXBwdArgs x5 = xb;
    x5.layer = l; x5.sc = s.sv.sc[l]; x5.cst = s.sv.cst[l];
    for (int j = 0; j < CFD_NMEM; ++j) {
      const size_t rows = (size_t)p.U[j] * p.Sp[j];
      x5.K[j] = w->kall_sp[j].as<char>() + (size_t)l * rows * CFD_D * 4;
      x5.VT[j] = w->vt_all[j].as<char>() + (size_t)l * rows * CFD_D * 4;
      x5.kb[j] = w->now_kb[j] + (size_t)l * CFD_D;
      x5.vb[j] = w->now_vb[j] + (size_t)l * CFD_D;
    }
    if (l < nl - 1 || seed.d_out) {
      {   // B1: through the next layer's norm1 (the top layer: decoder.norm) into this layer's output, then linear2 and the GELU
        RtBwdArgs a = base;
        a.K = CFD_D; a.a = dy1; a.g = have_g ? s.G[gi] : nullptr; a.x = s.sv.x[l + 1][0]; a.gout = s.G[(gi + 1) % 3];
        a.gamma = l < nl - 1 ? c->lw[l + 1].ln1g : rawp(c, "decoder.norm.weight");
        a.w = Wraw(l, "linear2.weight"); a.ldw = CFD_FF; a.out = s.dh; a.ldo = CFD_FF; a.pre = s.sv.pre[l];
        CHK((bwd_gemm<RT_BPRO_LN, RT_BEPI_GELU, 16>(c, st, a, CFD_FF, ntile)));
        gi = (gi + 1) % 3;
        have_g = true;
      }
      WEG_STOP_AT(1);
      {   // B2: linear1
        RtBwdArgs a = base;
        a.K = CFD_FF; a.a = s.dh; a.w = Wraw(l, "linear1.weight"); a.ldw = CFD_D; a.out = s.dy; a.ldo = CFD_D;
        CHK((bwd_gemm<RT_BPRO_ROWS, RT_BEPI_F32, 32>(c, st, a, CFD_D, ntile)));
      }
      WEG_STOP_AT(2);
      {   // B3: norm3, then time block 2's projection
        RtBwdArgs a = base;
        a.K = CFD_D; a.a = s.dy; a.g = s.G[gi]; a.x = s.sv.x[l][4]; a.gamma = lw.ln3g; a.gout = s.G[(gi + 1) % 3];
        a.w = Wraw(l, "time_block2.out_layers.2.weight"); a.ldw = CFD_D; a.out = s.dz; a.ldo = CFD_D;
        CHK((bwd_gemm<RT_BPRO_LN, RT_BEPI_F32, 16>(c, st, a, CFD_D, ntile)));
        gi = (gi + 1) % 3;
      }
      WEG_STOP_AT(3);
      {   // B4: time block 2's SiLU / modulation / norm, then the probabilities' gradient
        RtXBwdArgs a = x5;
        a.dz = s.dz; a.g = s.G[gi]; a.x = s.sv.x[l][3]; a.gamma = lw.tb2g; a.beta = lw.tb2b;
        a.ss = w->now_ss + (size_t)(2 * l + 1) * 2 * CFD_D; a.gout = s.G[(gi + 1) % 3];
        LAUNCH_COUNTED(s.launches, rt_xbwd_dp_kernel<>, dim3(nkb, ntile), dim3(512), rt_xbwd_dp_lds(), st, a);
        gi = (gi + 1) % 3;
      }
      WEG_STOP_AT(4);
    }
    {   // B5: softmax backward and the folded keys
      RtXBwdArgs a = x5;
      a.dp_from_datt = have_g ? 0 : 1;
      LAUNCH_COUNTED_AS(s.launches, "rt_xbwd_dy_kernel", dy_kernel, dim3(CFD_D / 16, ntile), dim3(512), rt_xbwd_dy_lds(p.Sp_tot), st, a);
    }
    WEG_STOP_AT(5);
    if (mg) CHK(enqueue_mem_grad_layer(c, st, *mg, l, l == nl - 1, base, s.G[gi], ntile));   // (G[gi]: the gradient B4 wrote)
    {   // B6: norm2, then time block 1's projection
      RtBwdArgs a = base;
      a.K = CFD_D; a.a = s.dy; a.g = have_g ? s.G[gi] : nullptr; a.x = s.sv.x[l][2]; a.gamma = lw.ln2g; a.gout = s.G[(gi + 1) % 3];
      a.w = Wraw(l, "time_block1.out_layers.2.weight"); a.ldw = CFD_D; a.out = s.dz; a.ldo = CFD_D;
      CHK((bwd_gemm<RT_BPRO_LN, RT_BEPI_F32, 16>(c, st, a, CFD_D, ntile)));
      gi = (gi + 1) % 3;
      have_g = true;
    }
    WEG_STOP_AT(6);
    {   // B7: time block 1, then the attention's output projection
      RtBwdArgs a = base;
      a.K = CFD_D; a.a = s.dz; a.g = s.G[gi]; a.x = s.sv.x[l][1]; a.gamma = lw.tb1g; a.beta = lw.tb1b;
      a.ss = w->now_ss + (size_t)(2 * l) * 2 * CFD_D; a.gout = s.G[(gi + 1) % 3];
      a.w = Wraw(l, "self_attn.out_proj.weight"); a.ldw = CFD_D; a.out = s.dO; a.ldo = CFD_D;
      CHK((bwd_gemm<RT_BPRO_TB, RT_BEPI_F32, 16>(c, st, a, CFD_D, ntile)));
      gi = (gi + 1) % 3;
    }
    WEG_STOP_AT(7);
    {   // B8: attention core
      RtSelfBwdArgs a{s.sv.qk[l], s.sv.vt[l], s.dO, s.dqkv, L, (float)std::sqrt(1.0 / (double)CFD_HD)};
      LAUNCH_COUNTED(s.launches, rt_selfattn_bwd_kernel<>, dim3(CFD_NHEAD, B), dim3(256), rt_selfattn_bwd_lds(), st, a);
    }
    WEG_STOP_AT(8);
    {   // B9: packed in-projection
      RtBwdArgs a = base;
      a.K = 3 * CFD_D; a.a = s.dqkv; a.w = Wraw(l, "self_attn.in_proj_weight"); a.ldw = CFD_D; a.out = s.dy; a.ldo = CFD_D;
      CHK((bwd_gemm<RT_BPRO_ROWS, RT_BEPI_F32, 48>(c, st, a, CFD_D, ntile)));
      dy1 = s.dy;
    }
    WEG_STOP_AT(9);
  }
#undef WEG_STOP_AT
  if (mg) CHK(enqueue_mem_grad_finish(c, st, *mg));
  if (grad || !mg) {   // through layer 0's norm1 and the latent embedding
    RtBwdArgs a = base;
    a.K = CFD_D; a.a = dy1; a.g = s.G[gi]; a.x = s.sv.x[0][0]; a.gamma = c->lw[0].ln1g; a.gout = s.G[(gi + 1) % 3];
    a.w = rawp(c, "latent_embd.weight"); a.ldw = CFD_LAT; a.out = grad; a.ldo = CFD_LAT;
    CHK((bwd_gemm<RT_BPRO_LN, RT_BEPI_F32, 16>(c, st, a, CFD_LAT, ntile)));
    s.stop_gi = (gi + 1) % 3;   // the gradient at the embedding's output
  }
  return CFD_OK;
}

// cfd_denoise_vjp's launches: time tables and memory side, the whole forward with saved activations, the sweep from the output
static int enqueue_vjp(Ctx* c, hipStream_t st, const float* sample, const float* d_out, float* grad, const MemGrad* mg = nullptr) {
  WorkGuard guard(c);
  begin_sequence(c);
  CHK(enqueue_memory_side(c, st));
  CHK(enqueue_forward_saved(c, st, sample));
  return enqueue_reverse_sweep(c, st, SweepSeed{d_out}, grad, mg);
}

}  // namespace rtgrad
