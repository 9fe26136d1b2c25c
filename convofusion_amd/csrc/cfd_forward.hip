// libcfdenoise: the launches of one denoiser forward (tile kernels: enqueue_rows; small problems: enqueue_rows_rt), cfd_forward and the
// per-class profiling hook.  Which of them run, and in which form, is Problem::path (decided in setup_problem, cfd_problem.hip): the
// launch sequences read it and decide nothing themselves.
#include "cfd_internal.hpp"

// ---- the denoiser forward: Denoiser.forward (denoiser.py:173-386) --------------------------------------
// Input: c->w->sample_sp (SP [M][128]); time tables built; output: c->w->eps (fp32 [M][128]).


int enqueue_denoise(Ctx* c, hipStream_t st) {
  CHK(enqueue_memside(c, st));
  if (c->w->pb.path.rt) return enqueue_rows_rt(c, st);
  return enqueue_rows(c, st);
}

// This step's rows of the per-step tables: Work::now_* point at the tables themselves (one table row: cfd_forward, the WEG evaluation;
// per-row timesteps and level batches, whose launches take the step index), or -- a sampling run with one timestep for all rows -- ONE
// launch at the start of the iteration copies row *dstep of every listed table to a fixed place in rt_cur (64-float4 granules, in list
// order) and redirects its `now` to the copy, so that no launch of the iteration has the step index as a dependent scalar load in front
// of its operand loads (a load that misses in every XCD's L2 after the previous iteration's last workgroup has written it: ~1 us on 18
// AdaLN launches and 9 cross-attention prologues per step).  The list: the AdaLN rows, A b / VV b of the memories whose projections
// are made once, the row-tile path's key tables.
struct StepTab { const float** now; int nfloat; };
static std::vector<StepTab> step_tabs(Ctx* c) {
  Work* w = c->w;
  const Problem& p = w->pb;
  const int nl = c->nl;
  std::vector<StepTab> tabs{{&w->now_ss, nl * 4 * CFD_D}};
  for (int j = 0; j < CFD_NMEM; ++j) {
    if ((p.path.static_mask >> j) & 1) { tabs.push_back({&w->now_kb[j], nl * CFD_D + 32}); tabs.push_back({&w->now_vb[j], nl * CFD_D}); }
    if (p.path.rt) tabs.push_back({&w->now_cbt[j], (nl + 1) * p.U[j] * p.Sp[j]});
  }
  return tabs;
}
static size_t step_granules(const StepTab& t) { return (size_t)(t.nfloat / 4 + 63) / 64 * 64; }

size_t step_rows_bytes(Ctx* c) {
  if (!c->w->pb.path.rows_now || c->w->pb.T <= 1) return 0;
  size_t off4 = 0;
  for (const StepTab& t : step_tabs(c)) off4 += step_granules(t);
  return off4 * 16;
}

static int refresh_step_rows(Ctx* c, hipStream_t st) {
  Work* w = c->w;
  w->now_ss = w->ss_tab.as<float>();
  for (int j = 0; j < CFD_NMEM; ++j) { w->now_kb[j] = w->kbtab[j].as<float>(); w->now_vb[j] = w->vbtab[j].as<float>(); w->now_cbt[j] = w->rt_cbt[j].as<float>(); }
  const size_t bytes = step_rows_bytes(c);
  if (!bytes) return CFD_OK;
  const std::vector<StepTab> tabs = step_tabs(c);
  if (tabs.size() > RT_NTAB) return fail(CFD_E_ARG, "%d per-step tables, rt_step_rows_kernel takes %d", (int)tabs.size(), RT_NTAB);
  if (bytes > w->rt_cur.bytes) return fail(CFD_E_STATE, "rt_cur holds %zu bytes, this step's table rows take %zu", w->rt_cur.bytes, bytes);
  RtStepRowsArgs ra;
  memset(&ra, 0, sizeof(ra));
  size_t off4 = 0;
  int nwg = 0;
  for (const StepTab& t : tabs) {
    float* dst = w->rt_cur.as<float>() + off4 * 4;
    ra.src[ra.ntab] = *t.now; ra.dst[ra.ntab] = dst; ra.n4[ra.ntab] = t.nfloat / 4; ra.first[ra.ntab] = nwg;
    nwg += (t.nfloat / 4 + 255) / 256; off4 += step_granules(t); ++ra.ntab;
    *t.now = dst;
  }
  ra.first[ra.ntab] = nwg; ra.d_step = w->d_step.as<int>() + w->pb.path.dstep_slot;
  LAUNCH(CFD_PROF_OTHER, rt_step_rows_kernel<>, dim3(nwg), dim3(256), st, ra);
  return CFD_OK;
}

// The forward for small problems: launches of 16-token x 16-feature workgroups (rowtile.hpp); same buffers, same tap points.
// With `sv` (the row-tile gradient engine, rt_grad.hpp) every residual update goes to a buffer of its own, the self-attention operands, the
// cross-attention scores and the FFN pre-activations of every layer are kept, and the pass ends behind the last layer's
// cross-attention (nothing above it reaches the objective) -- unless sv->whole (cfd_denoise_vjp: the sweep starts at the output).

int enqueue_rows_rt(Ctx* c, hipStream_t st, const RtSave* sv) {
  const Problem& p = c->w->pb;
  const int nl = c->nl, L = p.L, tpr = (L + 15) / 16, ntile = p.Be * tpr;
  const int lds_xpv = rt_xpv_lds(p.Sp_tot, p.Sp_tot <= 512 ? 512 : RT_MAX_KEYS);
#define RT_SET_LDS(kernel, bytes) HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void*>(&kernel), hipFuncAttributeMaxDynamicSharedMemorySize, bytes))
  static unsigned long long attr_done = 0;
  CHK(once_per_device(attr_done, c->cfg.device, [&]() -> int {
    RT_SET_LDS((rt_gemm_kernel<RT_PRO_SP, RT_EPI_EMBED, 256, CFD_LAT / 32, 1>), rt_gemm_lds(RT_PRO_SP, 256, CFD_LAT / 32, 1));
    RT_SET_LDS((rt_gemm_kernel<RT_PRO_LN, RT_EPI_QKV, 512, CFD_D / 32, 3>), rt_gemm_lds(RT_PRO_LN, 512, CFD_D / 32, 3));
    RT_SET_LDS((rt_gemm_kernel<RT_PRO_SP, RT_EPI_RESID, 256, CFD_D / 32, 1>), rt_gemm_lds(RT_PRO_SP, 256, CFD_D / 32, 1));
    RT_SET_LDS((rt_gemm_kernel<RT_PRO_ADALN, RT_EPI_RESID, 512, CFD_D / 32, 1>), rt_gemm_lds(RT_PRO_ADALN, 512, CFD_D / 32, 1));
    RT_SET_LDS((rt_gemm_kernel<RT_PRO_LN, RT_EPI_SPLIT, 512, CFD_D / 32, 2>), rt_gemm_lds(RT_PRO_LN, 512, CFD_D / 32, 2));
    RT_SET_LDS((rt_gemm_kernel<RT_PRO_SP, RT_EPI_RESID, 512, CFD_FF / 32, 1>), rt_gemm_lds(RT_PRO_SP, 512, CFD_FF / 32, 1));
    RT_SET_LDS((rt_gemm_kernel<RT_PRO_LN, RT_EPI_F32, 512, CFD_D / 32, 1>), rt_gemm_lds(RT_PRO_LN, 512, CFD_D / 32, 1));
    RT_SET_LDS((rt_gemm_kernel<RT_PRO_SP, RT_EPI_RESID, 256, CFD_D / 32, 2>), rt_gemm_lds(RT_PRO_SP, 256, CFD_D / 32, 2));
    RT_SET_LDS((rt_gemm_kernel<RT_PRO_ADALN, RT_EPI_RESID, 512, CFD_D / 32, 2>), rt_gemm_lds(RT_PRO_ADALN, 512, CFD_D / 32, 2));
    RT_SET_LDS(rt_xscore_kernel<>, RT_XS_LDS);
    RT_SET_LDS(rt_xpv_kernel<512>, rt_xpv_lds(512, 512));
    RT_SET_LDS(rt_xpv_kernel<RT_MAX_KEYS>, rt_xpv_lds(RT_MAX_KEYS, RT_MAX_KEYS));
    return CFD_OK;
  }));
#undef RT_SET_LDS
  // The residual stream alternates between two buffers: a time block's workgroups read COMPLETE rows (LayerNorm prologue) while the
  // other workgroups of the tile write their 16 features of the sum, so it must not run in place.  x -> (time block 1) -> h ->
  // (cross-attention) -> x -> (time block 2) -> h -> (FFN) -> x; the products whose prologue reads another matrix (out-projection,
  // FFN2) and the cross-attention's second half touch only their own 16 features of the rows and may update in place.
  float* const xw = c->w->x.as<float>();
  float* const hw = c->w->h_sp.as<float>();   // (the tile-kernel path's LayerNorm output: same bytes, unused here)
  auto X = [&](int l, int k) -> float* { return sv ? sv->x[l][k] : ((k == 2 || k == 4) ? hw : xw); };
  CHK(refresh_step_rows(c, st));   // Work::now_*: this step's rows of the per-step tables
  RtGemmArgs base;
  memset(&base, 0, sizeof(base));
  base.L = L; base.tpr = tpr;
  // Two 16-feature blocks per workgroup for the 512 x 512 residual products from two utterances on: half the workgroups, each normalising
  // its 16 rows once for two blocks (one utterance: 0.411 -> 0.421 s per 1000 steps, two: 0.544 -> 0.528, four: 0.882 -> 0.869; same sums
  // in the same order, so bit-identical).  Counted in token tiles: 14 are two utterances of 7 guidance rows at L = 16.
  const int RT_NFB2_MIN_TILES = 14;
  const bool nfb2 = ntile >= RT_NFB2_MIN_TILES && !sv;
#define RT_LAUNCH(cls, PRO, EPI, NT, KT, NFB, nfeat, args)                                                        \
  do {                                                                                                          \
    Bracket _br(c, cls, st);                                                                                    \
    hipLaunchKernelGGL((rt_gemm_kernel<PRO, EPI, NT, KT, NFB>), dim3((nfeat) / (16 * NFB), ntile), dim3(NT), rt_gemm_lds(PRO, NT, KT, NFB), st, args); \
    hipError_t _e = hipGetLastError();                                                                          \
    if (_e != hipSuccess) return fail(CFD_E_HIP, "row-tile launch failed: %s", hipGetErrorString(_e));          \
  } while (0)
  // 1. latent embedding + body/hand embedding + query PE          (denoiser.py:187,316-326)
  {
    RtGemmArgs a = base;
    a.a_sp = c->w->sample_sp.as<char>(); a.w = c->we_sp.as<char>(); a.bias = rawp(c, "latent_embd.bias");
    a.bh = rawp(c, "bh_embedding.weight"); a.qpe = rawp(c, "query_pos.pe"); a.xo = X(0, 0);
    RT_LAUNCH(CFD_PROF_GEMM_TOKEN, RT_PRO_SP, RT_EPI_EMBED, 256, CFD_LAT / 32, 1, CFD_D, a);
  }
  if (c->stop_stage == 1) return CFD_OK;
  auto time_block = [&](const DBuf& w, const float* g, const float* b, const float* bias, int tbidx, const float* xin, float* xout) -> int {
    RtGemmArgs a = base;
    a.x = xin; a.xr = xin; a.xo = xout;
    a.g = g; a.b = b; a.ss = c->w->now_ss + (size_t)tbidx * 2 * CFD_D; a.w = w.as<char>(); a.bias = bias;
    if (nfb2) RT_LAUNCH(CFD_PROF_GEMM_TOKEN, RT_PRO_ADALN, RT_EPI_RESID, 512, CFD_D / 32, 2, CFD_D, a);
    else RT_LAUNCH(CFD_PROF_GEMM_TOKEN, RT_PRO_ADALN, RT_EPI_RESID, 512, CFD_D / 32, 1, CFD_D, a);
    return CFD_OK;
  };
  RtXArgs xa;
  memset(&xa, 0, sizeof(xa));
  xa.L = L; xa.tpr = tpr; xa.nl = nl; xa.Sp_tot = p.Sp_tot; xa.rsp = c->w->p_sp.as<float>();
  int nkb = 0;
  for (int j = 0; j < CFD_NMEM; ++j) {
    xa.map[j] = p.map[j]; xa.rows[j] = p.U[j] * p.Sp[j]; xa.S[j] = p.S[j]; xa.Sp[j] = p.Sp[j]; xa.off[j] = p.off[j];
    xa.cbt[j] = c->w->now_cbt[j]; xa.att[j] = p.att[j]; xa.att_slot[j] = p.att_slot[j];
    memcpy(xa.inst[j], p.rt_inst[j], RT_ARG_ROWS);
    xa.blk0[j] = nkb; nkb += p.Sp[j] / 16;
  }
  xa.blk0[CFD_NMEM] = nkb;
  xa.att_b0 = p.att_nb > 0 ? p.att_b0 : 0;
  xa.att_nb = p.att_nb > 0 ? p.att_nb : p.Be;
  xa.att_step = p.att_nb > 0 ? c->w->d_step.as<int>() : nullptr;
  for (int l = 0; l < nl; ++l) {
    const LayerW& w = c->lw[l];
    char* qk = sv ? sv->qk[l] : c->w->qkv_sp.as<char>();
    char* vt = sv ? sv->vt[l] : c->w->rt_vt.as<char>();
    // ---- a. self attention: x += Wo softmax(q k^T) v                         (cross_attention.py:568-572)
    {
      RtGemmArgs a = base;   // norm1 + q | k | v^T projections
      a.x = X(l, 0);
      a.g = w.ln1g; a.b = w.ln1b; a.w = w.wqkv_rt_sp.as<char>(); a.w2 = w.wqkv_rt_sp.as<char>() + (size_t)2 * CFD_D * CFD_D * 4; a.nfb_qk = 2 * CFD_D / 16;
      a.bias = w.bqk.as<float>(); a.o_sp = qk; a.ld_o = 2 * CFD_D * 4; a.vt = vt; a.w_scaled = 1;   // (the row-tile copies: x CFD_SAW_SCALE)
      RT_LAUNCH(CFD_PROF_GEMM_TOKEN, RT_PRO_LN, RT_EPI_QKV, 512, CFD_D / 32, 3, 3 * CFD_D, a);
    }
    {
      RtSelfArgs a{qk, vt, c->w->o_sp.as<char>(), L, tpr};
      Bracket br(c, CFD_PROF_GEMM_ATTN, st);
      hipLaunchKernelGGL(rt_selfattn_kernel<>, dim3(CFD_NHEAD, ntile), dim3(256), 40960, st, a);
      HIPCHK(hipGetLastError());
    }
    {
      RtGemmArgs a = base;   // out-projection + residual
      a.xr = X(l, 0); a.xo = X(l, 1);
      a.a_sp = c->w->o_sp.as<char>(); a.w = w.wo_rt_sp.as<char>(); a.bias = w.bo2.as<float>(); a.w_scaled = 1;
      if (nfb2) RT_LAUNCH(CFD_PROF_GEMM_TOKEN, RT_PRO_SP, RT_EPI_RESID, 256, CFD_D / 32, 2, CFD_D, a);
      else RT_LAUNCH(CFD_PROF_GEMM_TOKEN, RT_PRO_SP, RT_EPI_RESID, 256, CFD_D / 32, 1, CFD_D, a);
    }
    if (c->stop_stage == 2 + 4 * l) return CFD_OK;
    // ---- b. time block 1                                                        (:575, :426-439)
    CHK(time_block(w.wtb1_sp, w.tb1g, w.tb1b, w.btb1, 2 * l, X(l, 1), X(l, 2)));
    if (c->stop_stage == 3 + 4 * l) {   // (test hook: the tap is read from x)
      if (!sv) HIPCHK(hipMemcpyAsync(xw, hw, (size_t)p.M * CFD_D * 4, hipMemcpyDeviceToDevice, st));
      return CFD_OK;
    }
    // ---- c-e. five cross attentions + fuser, folded                             (:578-652)
    {
      RtXArgs a = xa;
      a.x = X(l, 2); a.xo = X(l, 3);
      a.sc = sv ? sv->sc[l] : c->w->sc.as<float>();
      a.cst = sv ? sv->cst[l] : c->w->rt_cst.as<float>();
      a.ln_g = w.ln2g; a.ln_b = w.ln2b; a.bias = w.cross_bias.as<float>(); a.layer = l;
      for (int j = 0; j < CFD_NMEM; ++j) {
        const size_t rows = (size_t)p.U[j] * p.Sp[j];
        a.K[j] = c->w->kall_sp[j].as<char>() + (size_t)l * rows * CFD_D * 4;
        a.VT[j] = c->w->vt_all[j].as<char>() + (size_t)l * rows * CFD_D * 4;
        a.kb[j] = c->w->now_kb[j] + (size_t)l * CFD_D;
        a.vb[j] = c->w->now_vb[j] + (size_t)l * CFD_D;
      }
      {
        Bracket br(c, CFD_PROF_XATTN, st);
        hipLaunchKernelGGL(rt_xscore_kernel<>, dim3(p.Sp_tot / 32, ntile), dim3(512), RT_XS_LDS, st, a);
        HIPCHK(hipGetLastError());
      }
      {
        Bracket br(c, CFD_PROF_XATTN, st);
        if (p.Sp_tot <= 512) hipLaunchKernelGGL(rt_xpv_kernel<512>, dim3(CFD_D / 16, ntile), dim3(512), lds_xpv, st, a);
        else hipLaunchKernelGGL(rt_xpv_kernel<RT_MAX_KEYS>, dim3(CFD_D / 16, ntile), dim3(512), lds_xpv, st, a);
        HIPCHK(hipGetLastError());
      }
    }
    if (c->stop_stage == 4 + 4 * l) return CFD_OK;
    if (sv && !sv->whole && l == nl - 1) return CFD_OK;
    // ---- f. time block 2                                                        (:655)
    CHK(time_block(w.wtb2_sp, w.tb2g, w.tb2b, w.btb2, 2 * l + 1, X(l, 3), X(l, 4)));
    // ---- g. FFN                                                                 (:659-661)
    {
      RtGemmArgs a = base;   // norm3 + linear1 + GELU
      a.x = X(l, 4);
      a.g = w.ln3g; a.b = w.ln3b; a.w = w.w1_sp.as<char>(); a.bias = w.b1; a.o_sp = c->w->u_sp.as<char>(); a.ld_o = CFD_FF * 4; a.gelu = 1;
      a.pre = sv ? sv->pre[l] : nullptr;
      RT_LAUNCH(CFD_PROF_GEMM_TOKEN, RT_PRO_LN, RT_EPI_SPLIT, 512, CFD_D / 32, 2, CFD_FF, a);
    }
    {
      RtGemmArgs a = base;   // linear2 + residual
      a.xr = X(l, 4); a.xo = X(l + 1, 0);
      a.a_sp = c->w->u_sp.as<char>(); a.w = w.w2_sp.as<char>(); a.bias = w.b2;
      RT_LAUNCH(CFD_PROF_GEMM_TOKEN, RT_PRO_SP, RT_EPI_RESID, 512, CFD_FF / 32, 1, CFD_D, a);
    }
    if (c->stop_stage == 5 + 4 * l) return CFD_OK;
  }
  // 7. final norm + latent projection                                (cross_attention.py:238-239, denoiser.py:382)
  {
    RtGemmArgs a = base;
    a.x = X(nl, 0);
    a.g = rawp(c, "decoder.norm.weight"); a.b = rawp(c, "decoder.norm.bias"); a.w = c->wp_sp.as<char>();
    a.bias = rawp(c, "latent_proj.bias"); a.o_f32 = c->w->eps.as<float>(); a.ldo_f = CFD_LAT;
    RT_LAUNCH(CFD_PROF_GEMM_TOKEN, RT_PRO_LN, RT_EPI_F32, 512, CFD_D / 32, 1, CFD_LAT, a);
  }
#undef RT_LAUNCH
  return CFD_OK;
}

int enqueue_rows(Ctx* c, hipStream_t st) {
  const Problem& p = c->w->pb;
  const int nl = c->nl, L = p.L, Be = p.Be;
  const long long M = p.M;
  const int* dstep = c->w->d_step.as<int>() + p.path.dstep_slot;
  const long long ROWB = CFD_D * 4;  // bytes per SP row of 512
  const dim3 blk(256);
  // one fused kernel per layer for the cross-attention block, or the three launches (path.xattn)
  const bool fused_x = p.path.xattn == XATTN_FUSED;
  // rows that run the replica-independent head of the network (path.share)
  const bool share = p.path.share;
  const int Bs = share ? p.path.share_rows : Be;
  const long long Ms = (long long)Bs * L;
  // 1. latent embedding + body/hand embedding + query PE          (denoiser.py:187,316-326)
  {
    GemmArgs a = gemm_args();
    gemm_x(a, 0, c->we_sp.as<char>(), CFD_D, CFD_LAT, CFD_LAT * 4);
    gemm_y(a, c->w->sample_sp.as<char>(), (int)Ms, CFD_LAT * 4);
    EpiEmbed e{c->w->x.as<float>(), rawp(c, "latent_embd.bias"), rawp(c, "bh_embedding.weight"), rawp(c, "query_pos.pe"), L};
    CHK((run_gemm<MODE_PLAIN>(c, CFD_PROF_GEMM_TOKEN, a, e, 1, 1, st)));
  }
  if (c->stop_stage == 1) return CFD_OK;
  // Work::now_*: this step's rows of the per-step tables; with path.rows_now no launch takes the step index
  CHK(refresh_step_rows(c, st));
  const bool rows_now = p.path.rows_now;
  auto ln = [&](const float* g, const float* b, int adaln, int tbidx, char* out, long long rows) -> int {
    LnArgs a{c->w->x.as<float>(), out, rows, g, b, adaln, c->w->now_ss + (size_t)tbidx * 2 * CFD_D,
             (long long)nl * 2 * 2 * CFD_D, rows_now ? nullptr : dstep, p.tmode, p.tmode == 2 ? L * p.lv_rows : L,
             p.tmode == 2 ? p.lv_i0 : 0};   // (a level batch: table row lv_i0 + level, Problem::lv_rows rows per level)
    LAUNCH(CFD_PROF_ROWS, ln_rows_kernel<>, dim3((unsigned)((rows + 3) / 4)), blk, st, a);
    return CFD_OK;
  };
  auto token_gemm_resid = [&](const DBuf& w, int K, const char* y, const float* bias, long long rows) -> int {
    GemmArgs a = gemm_args();
    gemm_x(a, 0, w.as<char>(), CFD_D, K, (long long)K * 4);
    gemm_y(a, y, (int)rows, (long long)K * 4);
    EpiResid e{c->w->x.as<float>(), 0, bias};
    return run_gemm<MODE_PLAIN>(c, CFD_PROF_GEMM_TOKEN, a, e, 1, 1, st);
  };
  // residual product + the LayerNorm that follows it
  auto token_gemm_resid_ln = [&](const DBuf& w, int K, const char* y, const float* bias, long long rows, const float* g, const float* b,
                                 int adaln, int tbidx) -> int {
    CHK(token_gemm_resid(w, K, y, bias, rows));
    return ln(g, b, adaln, tbidx, c->w->h_sp.as<char>(), rows);
  };
  // The algebraic LayerNorm fold (gemm_sp.hpp EpiLn / EpiResidStat) for mid-size problems at the product shape: norm3, the
  // norm1 of layers 1.. and the decoder's final norm are not launched; the residual product in front of each stores the split pairs of the RAW rows and
  // per-row slot statistics, and the consumer (q | k | v^T in one launch, FFN1, latent_proj) runs on W diag(gamma) and rescales its accumulators.
  // Range: the launches launch_gemm gives the 64 x 64 / 128 x 64 classes anyway (launch_gemm_midsize); above it a ln_rows launch costs less than
  // the producer's wider epilogue (measured at the headline shape: +25.8 us against 14).
  const bool ln_fold = p.path.ln_fold;
  auto token_gemm_resid_stat = [&](const DBuf& w, int K, const char* y, const float* bias, long long rows, char* xs) -> int {
    GemmArgs a = gemm_args();
    gemm_x(a, 0, w.as<char>(), CFD_D, K, (long long)K * 4);
    gemm_y(a, y, (int)rows, (long long)K * 4);
    EpiResidStat e{c->w->x.as<float>(), 0, bias, xs, c->w->ln_stat.as<float>()};
    return run_gemm_midsize<MODE_PLAIN>(c, CFD_PROF_GEMM_TOKEN, a, e, st);
  };
  bool h_raw = false;     // h_sp holds the split pairs of the raw rows + ln_stat their statistics (ln_fold), not norm1(x)
  static unsigned long long attr_done = 0;
  CHK(once_per_device(attr_done, c->cfg.device, [&]() -> int {
    HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void*>(&self_attn_fused_kernel<>), hipFuncAttributeMaxDynamicSharedMemorySize, 65536));
    HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void*>(&xattn_fused_kernel<false, false>), hipFuncAttributeMaxDynamicSharedMemorySize, XA_LDS));
    HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void*>(&xattn_fused_kernel<false, true>), hipFuncAttributeMaxDynamicSharedMemorySize, XA_LDS));
    HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void*>(&xattn_fused_kernel<true, false>), hipFuncAttributeMaxDynamicSharedMemorySize, XA_LDS));
    return CFD_OK;
  }));

  bool h_ready = false;   // h_sp already holds norm1(x) of the layer that starts
  for (int l = 0; l < nl; ++l) {
    const LayerW& w = c->lw[l];
    // rows of sub-layers a and b: layer 0 runs them once per utterance when the batch is G replicas of it
    const int Ba = (l == 0) ? Bs : Be;
    const long long Ma = (long long)Ba * L;
    // ---- a. self attention: x += Wo softmax(q k^T) v                         (cross_attention.py:568-572)
    // (norm1 of layers 1.. is made by the previous layer's last residual product when that ran row-complete: `h_ready`)
    if (!h_ready) CHK(ln(w.ln1g, w.ln1b, 0, 0, c->w->h_sp.as<char>(), Ma));
    h_ready = false;
    bool qkv_one_launch = false;
    {
      // q (pre-scaled), k and v, token-major, in ONE product against [Wq; Wk; Wv] (cfd_finalize_weights): qkv_sp [M][1536], the 12 column
      // tiles of a token panel consecutive on one XCD (gemm_sp_body's block order), so h_sp is fetched once.  The bias covers q | k; its
      // last 512 entries are zeros (the value bias is folded into the out-projection's).
      GemmArgs a = gemm_args();
      gemm_x(a, 0, w.wqkv_sp.as<char>(), 3 * CFD_D, CFD_D, ROWB);
      gemm_y(a, c->w->h_sp.as<char>(), (int)Ma, ROWB);
      EpiSplit e{c->w->qkv_sp.as<char>(), 3 * ROWB, 0, 0, w.bqk.as<float>(), 0, 0};
      if (L == 16) {
        // batch rows of exactly 16 tokens: q | k and v in ONE grouped launch, the value projection stored transposed by the epilogue (EpiQkvT)
        GemmArgs ag = a;
        ag.nslot = 2;
        gemm_x(ag, 0, w.wqkv_sp.as<char>(), 2 * CFD_D, CFD_D, ROWB);
        gemm_x(ag, 1, w.wqkv_sp.as<char>() + 2 * CFD_D * ROWB, CFD_D, CFD_D, ROWB);
        EpiQkvT eg{c->w->qkv_sp.as<char>(), 2 * ROWB, w.bqk.as<float>(), c->w->vts_sp.as<char>(), 1};
        if (h_raw) {   // (layers 1..: the previous layer's second FFN product left raw rows + statistics)
          const float* cd = w.ln_cd.as<float>();
          ag.X[0] = w.wqk_f.as<char>(); ag.X[1] = w.wv_f.as<char>();
          CHK((run_gemm_midsize<MODE_GROUPED>(c, CFD_PROF_GEMM_TOKEN, ag, epi_ln(eg, c->w->ln_stat.as<float>(), cd, cd + 1024, cd + 2048, cd + 2560, 1e-5f), st)));
        } else {
          CHK((run_gemm<MODE_GROUPED>(c, CFD_PROF_GEMM_TOKEN, ag, eg, 1, 1, st)));
        }
        qkv_one_launch = true;
      } else {
        CHK((run_gemm<MODE_PLAIN>(c, CFD_PROF_GEMM_TOKEN, a, e, 1, 1, st)));
      }
    }
    if (qkv_one_launch) {
      // one query tile and one key tile per (row, head): the row-tile path's attention core (4 waves that all compute; V^T in natural key
      // order, which EpiQkvT wrote) instead of the flash kernel's 8-wave workgroup with one busy wave
      RtSelfArgs a{c->w->qkv_sp.as<char>(), c->w->vts_sp.as<char>(), c->w->o_sp.as<char>(), L, 1};
      Bracket br(c, CFD_PROF_GEMM_ATTN, st);
      hipLaunchKernelGGL(rt_selfattn_kernel<>, dim3(CFD_NHEAD, Ba), dim3(256), 40 * 1024, st, a);
      HIPCHK(hipGetLastError());
    } else {
      SelfAttnArgs a{c->w->qkv_sp.as<char>(), c->w->o_sp.as<char>(), 3 * ROWB, L};
      Bracket br(c, CFD_PROF_GEMM_ATTN, st);
      hipLaunchKernelGGL(self_attn_fused_kernel<>, dim3((L + SELF_ATTN_WAVES * 16 - 1) / (SELF_ATTN_WAVES * 16), CFD_NHEAD, Ba), dim3(SELF_ATTN_WAVES * 64), 65536, st, a);
      HIPCHK(hipGetLastError());
    }
    // out-projection + residual, then time block 1's AdaLN + SiLU                 (:572, :575, :426-439)
    CHK(token_gemm_resid_ln(w.wo_sp, CFD_D, c->w->o_sp.as<char>(), w.bo2.as<float>(), Ma, w.tb1g, w.tb1b, 1, 2 * l));
    if (c->stop_stage == 2 + 4 * l) return CFD_OK;
    // ---- b. time block 1
    CHK(token_gemm_resid(w.wtb1_sp, CFD_D, c->w->h_sp.as<char>(), w.btb1, Ma));
    if (c->stop_stage == 3 + 4 * l) return CFD_OK;
    if (Ma != M) {   // every guidance chunk starts its first cross-attention from the same state
      const long long n4 = Ma * (CFD_D / 4);
      LAUNCH(CFD_PROF_ROWS, replicate_rows_kernel<>, dim3((unsigned)((n4 + 255) / 256)), blk, st, reinterpret_cast<float4*>(c->w->x.as<float>()), n4,
             (int)(M / Ma));
    }
    // ---- c-e. five cross attentions + fuser, folded                             (:578-652)
    if (fused_x) {   // LayerNorm2 is part of the kernel's prologue
      XAttnArgs a;
      memset(&a, 0, sizeof(a));
      a.x = c->w->x.as<float>(); a.ln_g = w.ln2g; a.ln_b = w.ln2b; a.bias = w.cross_bias.as<float>(); a.L = L;
      for (int j = 0; j < CFD_NMEM; ++j) {
        const size_t rows = (size_t)p.U[j] * p.Sp[j];
        // (single-fp16 tiles of a long memory, the F16 instance's path.f16_mask: 32 KB per 32 keys = 1 KB per key, tile-major per (layer, instance))
        const bool f16 = (p.path.f16_mask >> j) & 1;
        a.K[j] = f16 ? c->w->k16[j].as<char>() + (size_t)l * rows * 1024 : c->w->kall_sp[j].as<char>() + (size_t)l * rows * ROWB;
        a.cb[j] = c->w->cb[j].as<float>() + (size_t)l * rows;
        a.VT[j] = f16 ? c->w->v16[j].as<char>() + (size_t)l * rows * 1024 : c->w->vt_all[j].as<char>() + (size_t)l * rows * ROWB;
        a.Sp[j] = p.Sp[j];
        const bool stat = (p.path.static_mask >> j) & 1;
        a.rs_off[j] = (unsigned)((size_t)(nl - l) * rows * 4);
        a.kb[j] = stat ? c->w->now_kb[j] + (size_t)l * CFD_D : c->w->zeros512.as<float>();
        a.kb_stride[j] = stat ? nl * CFD_D + 32 : 0;
        a.vb[j] = stat ? c->w->now_vb[j] + (size_t)l * CFD_D : c->w->zeros512.as<float>();
        a.vb_stride[j] = stat ? nl * CFD_D : 0;
      }
      a.d_step = rows_now ? nullptr : dstep;
      a.one_j = -1;
      if (p.xa_one >= 0) {   // (the work lists hold no segments for it: build_xattn_worklist)
        const int j = p.xa_one;
        const size_t rows = (size_t)p.U[j] * p.Sp[j];
        a.one_j = j; a.one_sp = p.Sp[j];
        a.one_va = c->w->xa_one_va.as<float>() + (size_t)l * p.U[j] * CFD_D;
        a.one_rs = c->w->cb[j].as<float>() + (size_t)nl * rows;
      }
      a.wgs = c->w->xa_wgs.as<XaWg>(); a.segs = c->w->xa_segs.as<XaSeg>();
#if XA_STAMP
      CHK(c->w->xa_stamps.ensure((size_t)p.xa_nwg * XA_WAVES * XA_NSTAMP * 8));
      a.stamps = c->w->xa_stamps.as<long long>();
#endif
      Bracket br(c, CFD_PROF_XATTN, st);
      const int inst = p.path.xa_inst;
      if (inst == XA_INST_ATT) a.att = c->w->xa_att_desc.as<XaAtt>() + l;
      if (c->acen.on && inst != XA_INST_ATT) {   // the attention-concentration census of a sampling run (the ATT instance counts nothing)
        a.census = c->acen.buf.as<unsigned>() + (size_t)l * XA_CEN_SLOTS * XA_CEN_STRIDE;
        a.census_tau = c->acen.tau;
        c->acen.hits += 1;
      }
      auto launch_xa = [&](int nwg, const XAttnArgs& xa) {
        if (inst == XA_INST_ATT) hipLaunchKernelGGL((xattn_fused_kernel<true, false>), dim3(nwg), dim3(XA_WAVES * 64), XA_LDS, st, xa);
        else if (inst == XA_INST_F16) hipLaunchKernelGGL((xattn_fused_kernel<false, true>), dim3(nwg), dim3(XA_WAVES * 64), XA_LDS, st, xa);
        else hipLaunchKernelGGL((xattn_fused_kernel<false, false>), dim3(nwg), dim3(XA_WAVES * 64), XA_LDS, st, xa);
      };
      if (l == 0 && share && p.xa0_nwg_a > 0) {   // layer-0 de-duplication (build_xattn_layer0_lists): the longest memory once per distinct (utterance, instance) ...
        XAttnArgs a0 = a;
        a0.wgs = c->w->xa0_wgs_a.as<XaWg>(); a0.segs = c->w->xa0_segs_a.as<XaSeg>(); a0.dd_out = c->w->xa_dedup.as<float>(); a0.stamps = nullptr;
        a0.one_j = -1;   // (the one-key memory belongs to the second launch)
        launch_xa(p.xa0_nwg_a, a0);
        HIPCHK(hipGetLastError());
        // ... then the other memories for every row, which also adds the stored results
        a0.wgs = c->w->xa0_wgs_b.as<XaWg>(); a0.segs = c->w->xa0_segs_b.as<XaSeg>(); a0.dd_out = nullptr; a0.dd_in = c->w->xa_dedup.as<float>();
        a0.one_j = a.one_j;
        launch_xa(p.xa0_nwg_b, a0);
        HIPCHK(hipGetLastError());
        if (c->prof) c->prof_n[CFD_PROF_XATTN] += 1;   // (two launches under one bracket)
      } else {
        launch_xa(p.xa_nwg, a);
        HIPCHK(hipGetLastError());
      }
    } else {
    CHK(ln(w.ln2g, w.ln2b, 0, 0, c->w->h_sp.as<char>(), M));
    // Three-launch path (att_mats wanted): scores against the folded keys of every memory.  Long memories and short
    // (<= 64 keys) memories go to different tile shapes; rows in a shared-memory run of the largest memory use one
    // un-batched product per run.
    const bool runs = p.nruns > 0;
    auto scores_grouped = [&](bool small, int skip_j, const int* brow, int nb) -> int {
      GemmArgs a = gemm_args();
      EpiF32 e;
      memset(&e, 0, sizeof(e));
      int n = 0;
      for (int j = 0; j < CFD_NMEM; ++j) {
        if ((p.Sp[j] <= 64) != small || j == skip_j) continue;
        gemm_x(a, n, c->w->kall_sp[j].as<char>() + (size_t)l * p.U[j] * p.Sp[j] * ROWB, p.Sp[j], CFD_D, ROWB);
        a.xbs[n] = (long long)p.Sp[j] * ROWB; a.xmap[n] = p.map[j];
        e.goff[n] = p.off[j]; e.gbias[n] = c->w->cb[j].as<float>() + (size_t)l * p.U[j] * p.Sp[j]; e.gmap[n] = p.map[j]; e.gstride[n] = p.Sp[j];
        ++n;
      }
      if (!n || nb <= 0) return CFD_OK;
      a.nslot = n; a.brow = brow;
      gemm_y(a, c->w->h_sp.as<char>(), L, ROWB);
      a.ybs = (long long)L * ROWB;
      e.out = c->w->sc.as<float>(); e.ldo = p.Sp_tot; e.obs = (long long)L * p.Sp_tot;
      return run_gemm<MODE_GROUPED>(c, CFD_PROF_GEMM_ATTN, a, e, nb, 1, st);
    };
    CHK(scores_grouped(true, -1, nullptr, Be));   // short memories
    if (!runs) {
      CHK(scores_grouped(false, -1, nullptr, Be));
    } else {
      CHK(scores_grouped(false, -1, c->w->short_rows.as<int>(), p.nshort));
      CHK(scores_grouped(false, p.jbig, c->w->long_rows.as<int>(), p.nlong));
      const int j = p.jbig;
      for (int r = 0; r < p.nruns; ++r) {
        GemmArgs a = gemm_args();
        gemm_x(a, 0, c->w->kall_sp[j].as<char>() + ((size_t)l * p.U[j] + p.run_u[r]) * p.Sp[j] * ROWB, p.Sp[j], CFD_D, ROWB);
        gemm_y(a, c->w->h_sp.as<char>() + (size_t)p.run_row0[r] * L * ROWB, p.run_len[r] * L, ROWB);
        EpiF32 e;
        memset(&e, 0, sizeof(e));
        e.out = c->w->sc.as<float>() + (size_t)p.run_row0[r] * L * p.Sp_tot; e.ldo = p.Sp_tot; e.goff[0] = p.off[j];
        e.gbias[0] = c->w->cb[j].as<float>() + ((size_t)l * p.U[j] + p.run_u[r]) * p.Sp[j]; e.gstride[0] = 0;
        CHK((run_gemm<MODE_PLAIN>(c, CFD_PROF_GEMM_ATTN, a, e, 1, 1, st)));
      }
    }
    {
      SoftmaxArgs a;
      memset(&a, 0, sizeof(a));
      a.sc = c->w->sc.as<float>(); a.P = c->w->p_sp.as<char>(); a.ld = p.Sp_tot; a.rows = M; a.rows_per_b = L; a.nseg = CFD_NMEM;
      for (int j = 0; j < CFD_NMEM; ++j) {
        a.off[j] = p.off[j]; a.S[j] = p.S[j]; a.Sp[j] = p.Sp[j]; a.mask[j] = p.mask[j]; a.has_mask[j] = p.has_mask[j]; a.map[j] = p.map[j]; a.att[j] = p.att[j];
      }
      a.layer = l; a.nl = nl;
      LAUNCH(CFD_PROF_ROWS, softmax_rows_kernel<>, dim3((unsigned)((M + 3) / 4)), blk, st, a);
    }
    // x += sum_j P_j . VV_j(n_j) + folded bias
    auto pv_segk = [&](int skip_j, const int* brow, int nb) -> int {
      if (nb <= 0) return CFD_OK;
      GemmArgs a = gemm_args();
      int n = 0;
      for (int j = 0; j < CFD_NMEM; ++j) {
        if (j == skip_j) continue;
        gemm_x(a, n, c->w->vt_all[j].as<char>() + (size_t)l * p.U[j] * CFD_D * p.Sp[j] * 4, CFD_D, p.Sp[j], (long long)p.Sp[j] * 4);
        a.xbs[n] = (long long)CFD_D * p.Sp[j] * 4; a.xmap[n] = p.map[j];
        a.yk0[n] = p.off[j] / 32;
        ++n;
      }
      a.nslot = n; a.brow = brow;
      gemm_y(a, c->w->p_sp.as<char>(), L, (long long)p.Sp_tot * 4);
      a.ybs = (long long)L * p.Sp_tot * 4;
      EpiResid e{c->w->x.as<float>(), (long long)L * CFD_D, w.cross_bias.as<float>()};
      return run_gemm<MODE_SEGK>(c, CFD_PROF_GEMM_ATTN, a, e, nb, 1, st);
    };
    if (!runs) {
      CHK(pv_segk(-1, nullptr, Be));
    } else {
      CHK(pv_segk(-1, c->w->short_rows.as<int>(), p.nshort));   // short rows: all segments
      CHK(pv_segk(p.jbig, c->w->long_rows.as<int>(), p.nlong));   // long rows: short segments first ...
      const int j = p.jbig;
      for (int r = 0; r < p.nruns; ++r) {   // ... then the shared audio memory, run by run (disjoint rows)
        GemmArgs a = gemm_args();
        gemm_x(a, 0, c->w->vt_all[j].as<char>() + ((size_t)l * p.U[j] + p.run_u[r]) * CFD_D * p.Sp[j] * 4, CFD_D, p.Sp[j], (long long)p.Sp[j] * 4);
        gemm_y(a, c->w->p_sp.as<char>() + (size_t)p.run_row0[r] * L * p.Sp_tot * 4 + (size_t)(p.off[j] / 32) * 128, p.run_len[r] * L, (long long)p.Sp_tot * 4);
        EpiResid e{c->w->x.as<float>() + (size_t)p.run_row0[r] * L * CFD_D, 0, nullptr};
        CHK((run_gemm<MODE_PLAIN>(c, CFD_PROF_GEMM_ATTN, a, e, 1, 1, st)));
      }
    }
    }
    if (c->stop_stage == 4 + 4 * l) return CFD_OK;
    // ---- f. time block 2                                                        (:655)
    CHK(ln(w.tb2g, w.tb2b, 1, 2 * l + 1, c->w->h_sp.as<char>(), M));
    // time block 2's projection + residual, then norm3                           (:655, :659)
    if (ln_fold) CHK(token_gemm_resid_stat(w.wtb2_sp, CFD_D, c->w->h_sp.as<char>(), w.btb2, M, c->w->o_sp.as<char>()));   // (o_sp: free since the out-projection)
    else CHK(token_gemm_resid_ln(w.wtb2_sp, CFD_D, c->w->h_sp.as<char>(), w.btb2, M, w.ln3g, w.ln3b, 0, 0));
    // ---- g. FFN                                                                 (:659-661)
    {
      GemmArgs a = gemm_args();
      gemm_x(a, 0, w.w1_sp.as<char>(), CFD_FF, CFD_D, ROWB);
      gemm_y(a, c->w->h_sp.as<char>(), (int)M, ROWB);
      EpiSplit e{c->w->u_sp.as<char>(), (long long)CFD_FF * 4, 0, 0, w.b1, 1, 0};
      if (ln_fold) {
        const float* cd = w.ln_cd.as<float>();
        a.X[0] = w.w1_f.as<char>(); a.Y = c->w->o_sp.as<char>();
        CHK((run_gemm_midsize<MODE_PLAIN>(c, CFD_PROF_GEMM_TOKEN, a, epi_ln(e, c->w->ln_stat.as<float>(), cd + 3072, cd + 4096, cd + 3072, cd + 4096, 1e-5f), st)));
      } else {
        CHK((run_gemm<MODE_PLAIN>(c, CFD_PROF_GEMM_TOKEN, a, e, 1, 1, st)));
      }
    }
    // second FFN product + residual, then the next layer's norm1 (or the decoder's final norm)   (:661, :568; :238-239)
    {
      const float* ng = l + 1 < nl ? c->lw[l + 1].ln1g : rawp(c, "decoder.norm.weight");
      const float* nb = l + 1 < nl ? c->lw[l + 1].ln1b : rawp(c, "decoder.norm.bias");
      if (c->stop_stage == 5 + 4 * l) return token_gemm_resid(w.w2_sp, CFD_FF, c->w->u_sp.as<char>(), w.b2, M);
      if (ln_fold) { CHK(token_gemm_resid_stat(w.w2_sp, CFD_FF, c->w->u_sp.as<char>(), w.b2, M, c->w->h_sp.as<char>())); h_raw = true; }
      else CHK(token_gemm_resid_ln(w.w2_sp, CFD_FF, c->w->u_sp.as<char>(), w.b2, M, ng, nb, 0, 0));
      h_ready = true;
    }
  }
  // 7. final norm (made above) + latent projection                                (cross_attention.py:238-239, denoiser.py:382)
  {
    GemmArgs a = gemm_args();
    gemm_x(a, 0, c->wp_sp.as<char>(), CFD_LAT, CFD_D, ROWB);
    gemm_y(a, c->w->h_sp.as<char>(), (int)M, ROWB);
    EpiF32 e;
    memset(&e, 0, sizeof(e));
    e.out = c->w->eps.as<float>(); e.ldo = CFD_LAT; e.bias = rawp(c, "latent_proj.bias");
    if (h_raw) {
      const float* cd = c->ln_cd_p.as<float>();
      a.X[0] = c->wp_f.as<char>();
      CHK((run_gemm_midsize<MODE_PLAIN>(c, CFD_PROF_GEMM_TOKEN, a, epi_ln(e, c->w->ln_stat.as<float>(), cd, cd + CFD_LAT, cd, cd + CFD_LAT, 1e-5f), st)));
    } else {
      CHK((run_gemm<MODE_PLAIN>(c, CFD_PROF_GEMM_TOKEN, a, e, 1, 1, st)));
    }
  }
  if (p.path.keeps_maps()) {   // this step's maps: from what the nine cross-attention launches kept, into slot *d_step of the ring
    XaFixArgs f;
    memset(&f, 0, sizeof(f));
    f.att = c->w->xa_att_desc.as<XaAtt>(); f.nl = nl; f.L = L; f.one_j = p.xa_one; f.d_step = c->w->d_step.as<int>();
    for (int j = 0; j < CFD_NMEM; ++j) { f.S[j] = p.S[j]; f.ring[j] = p.att[j]; f.slot[j] = p.att_slot[j]; }
    LAUNCH(CFD_PROF_ROWS, att_fixup_kernel<>, dim3((unsigned)(p.att_nb * L), nl), dim3(256), st, f);
  }
  return CFD_OK;
}

// ---- cfd_forward ---------------------------------------------------------------------------------------
extern "C" int cfd_forward(cfd_handle c, const float* sample, int Be, int L, const int32_t* timesteps, int n_t,
                           const cfd_memory mem[CFD_NUM_MEM], float* out, float* const att[CFD_NUM_MEM], void* stream) {
  if (!c) return fail(CFD_E_ARG, "null argument");
  c->hint_now = c->hint_same_mem;   // the promise covers THIS call only, however it ends
  c->hint_same_mem = false;
  if (!sample || !timesteps || !mem || !out) return fail(CFD_E_ARG, "null argument");
  if (c->run.open) return fail(CFD_E_STATE, "a sampling run is open on this handle");
  HIPCHK(hipSetDevice(c->cfg.device));
  CHK(settle_deferred_census(c));
  if (n_t != 1 && n_t != Be) return fail(CFD_E_ARG, "n_t must be 1 or Be");
  hipStream_t st = (hipStream_t)stream;
  const int tmode = (n_t == 1) ? 0 : 1;
  PathAsk ask;
  for (int j = 0; j < CFD_NMEM; ++j) ask.att_out = ask.att_out || (att && att[j]);
  // (test hook cfd_debug_forward_operands: the single-fp16 tiles of a sampling run's operand policy, asked for as setup_run_problem asks)
  ask.f16 = c->fwd_operands != 0 && tmode == 0 && !ask.att_out;
  CHK(setup_problem(c, Be, L, mem, nullptr, att, ask, tmode, n_t));
  CHK(sat_begin(c, st));
  // tmode 0 reads table row d_step[0] which must be 0 outside a sampling run
  HIPCHK(hipMemsetAsync(c->w->d_step.p, 0, 16, st));
  CHK(build_time_tables(c, timesteps, n_t, st));
  // (the sample is split in front of the once-per-call projections, so that ONE wait reads the census of both)
  CHK(enqueue_to_split(c, CFD_PROF_OTHER, st, sample, c->w->sample_sp.as<char>(), c->w->pb.M, CFD_LAT, (long long)CFD_LAT, (long long)CFD_LAT * 4, c->sat_in()));
  CHK(prepare_static_memside(c, st, c->hint_now && c->w->pb.prev_same));
  if (c->w->pb.path.static_mask) {   // once-per-call projections of the caller's memories: the census is read before they are used
    HIPCHK(hipStreamSynchronize(st));
    CHK(check_saturation(c, "cfd_forward (sample, memories / their projections)"));
  }
  c->memside_in_forward = false;
  CHK(enqueue_denoise(c, st));
  HIPCHK(hipMemcpyAsync(out, c->w->eps.p, (size_t)c->w->pb.M * CFD_LAT * 4, hipMemcpyDeviceToDevice, st));
  if (c->memside_in_forward || !c->w->pb.path.static_mask) {
    // Paths whose memory-side projections run INSIDE the forward (per-row timesteps, att_mats on the tile kernels, the three-launch
    // cross-attention): their census -- and the sample's, which no earlier wait has read on these paths -- is read here,
    // so that a clamped projection fails THIS call instead of the next one (on these paths the call therefore returns with `out` complete).
    HIPCHK(hipStreamSynchronize(st));
    c->memside_in_forward = false;
    CHK(check_saturation(c, "cfd_forward (sample, memories / their per-call projections)"));
  }
  {   // what the next call may reuse (cfd_forward_same_memories): all five memories' timestep-independent projections are in the workspace
    Work* w = c->w;
    const Problem& p = w->pb;
    w->fwd_mem_valid = p.tmode == 0 && p.path.static_mask == (1 << CFD_NMEM) - 1;
    w->fwd_wver = (unsigned long long)c->wver;
    w->fwd_Be = p.Be;
    w->fwd_L = p.L;
    w->fwd_att = ask.att_out;
    for (int j = 0; j < CFD_NMEM; ++j) {
      w->fwd_U[j] = p.U[j]; w->fwd_S[j] = p.S[j]; w->fwd_mask[j] = mem[j].key_padding_mask != nullptr; w->fwd_map[j] = mem[j].row_map != nullptr;
    }
  }
  return CFD_OK;
}

extern "C" int cfd_forward_same_memories(cfd_handle c) {
  if (!c) return fail(CFD_E_ARG, "null handle");
  c->hint_same_mem = true;
  return CFD_OK;
}

extern "C" int cfd_profile_forward(cfd_handle c, float ms[CFD_PROF_NCLASS], int launches[CFD_PROF_NCLASS]) {
  if (!c || !ms || !launches) return fail(CFD_E_ARG, "null argument");
  if (c->w->pb.Be == 0) return fail(CFD_E_STATE, "no problem configured (call cfd_forward or cfd_sample_begin first)");
  HIPCHK(hipSetDevice(c->cfg.device));
  if (c->run.open && c->run.pos >= c->run.iters)
    return fail(CFD_E_STATE, "sampling run is complete; profile before the last iteration");
  hipStream_t st = c->run.open ? c->run.stream : nullptr;
  HIPCHK(hipStreamSynchronize(st));
  for (int k = 0; k < CFD_PROF_NCLASS; ++k) { c->prof_ms[k] = 0.f; c->prof_n[k] = 0; }
  c->prof = true;
  int r = enqueue_denoise(c, st);
  c->prof = false;
  HIPCHK(hipStreamSynchronize(st));
  for (int k = 0; k < CFD_PROF_NCLASS; ++k) { ms[k] = c->prof_ms[k]; launches[k] = c->prof_n[k]; }
  return r;
}

// ---- developer hooks that share this unit's product instances (include/cfdenoise_dev.h) ---------------------
extern "C" int cfd_test_gemm(cfd_handle c, const float* X, const float* Y, float* out, int I, int J, int K, int tile_cfg,
                             void* stream) {
  if (!c || !X || !Y || !out || K % 32 || I % 4 || I < 4 || J < 1) return fail(CFD_E_ARG, "bad argument");
  HIPCHK(hipSetDevice(c->cfg.device));
  hipStream_t st = (hipStream_t)stream;
  DBuf xs, ys;
  CHK(xs.ensure((size_t)I * K * 4));
  CHK(ys.ensure((size_t)J * K * 4));
  CHK(enqueue_to_split(c, CFD_PROF_OTHER, st, X, xs.as<char>(), (long long)I, K, (long long)K,
                     (long long)K * 4, nullptr));
  CHK(enqueue_to_split(c, CFD_PROF_OTHER, st, Y, ys.as<char>(), (long long)J, K, (long long)K,
                     (long long)K * 4, nullptr));
  GemmArgs a = gemm_args();
  gemm_x(a, 0, xs.as<char>(), I, K, (long long)K * 4);
  gemm_y(a, ys.as<char>(), J, (long long)K * 4);
  EpiF32 e;
  memset(&e, 0, sizeof(e));
  e.out = out; e.ldo = I;
  hipError_t err = launch_gemm<MODE_PLAIN, EpiF32>(a, e, 1, 1, st, tile_cfg);
  if (err != hipSuccess) return fail(CFD_E_HIP, "gemm launch failed: %s", hipGetErrorString(err));
  HIPCHK(hipStreamSynchronize(st));
  return CFD_OK;
}

// One launch of the split-pair GEMM with one of the product's epilogues (include/cfdenoise_dev.h).  Only instances the product launches
// are used: the fold's producer and consumers go through launch_gemm_midsize, the other kinds through launch_gemm with any class.
extern "C" int cfd_test_gemm_epi(cfd_handle c, cfd_test_epi_args* t, void* stream) {
  if (!c || !t) return fail(CFD_E_ARG, "null argument");
  const int kind = t->kind, I = t->I, J = t->J, K = t->K;
  if (kind < CFD_EPI_F32 || kind > CFD_EPI_LN_QKVT) return fail(CFD_E_ARG, "unknown epilogue kind %d", kind);
  const bool fold = kind >= CFD_EPI_LN_F32, qkvt = kind == CFD_EPI_QKVT || kind == CFD_EPI_LN_QKVT;
  const bool resid = kind == CFD_EPI_RESID || kind == CFD_EPI_RESID_STAT, split = kind == CFD_EPI_SPLIT || kind == CFD_EPI_LN_SPLIT;
  if (K < 32 || K % 32) return fail(CFD_E_ARG, "K = %d: a positive multiple of 32", K);
  if (J < 1 || I < 4) return fail(CFD_E_ARG, "bad shape I = %d, J = %d", I, J);
  if (!t->X || (!t->Y && !t->y_sp)) return fail(CFD_E_ARG, "null operand");
  if (resid && I != CFD_D) return fail(CFD_E_ARG, "the residual epilogues have rows of %d features (I = %d)", CFD_D, I);
  if (qkvt && I != 3 * CFD_D) return fail(CFD_E_ARG, "q | k | v^T has I = %d (I = %d)", 3 * CFD_D, I);
  if (qkvt && J % 16) return fail(CFD_E_ARG, "q | k | v^T stores batch rows of 16 tokens (J = %d)", J);
  if (split && I % 32) return fail(CFD_E_ARG, "split-pair rows are whole 32-column blocks (I = %d)", I);
  if (I % 4) return fail(CFD_E_ARG, "the epilogues store 4 consecutive features (I = %d)", I);
  if (resid ? !t->x || (kind == CFD_EPI_RESID_STAT && (!t->out || !t->stat)) : !t->out) return fail(CFD_E_ARG, "null output");
  if (qkvt && (!t->out2 || !t->bias)) return fail(CFD_E_ARG, "q | k | v^T needs out2 and the bias");
  if (fold && (!t->gamma || !t->beta || !t->ln_stat)) return fail(CFD_E_ARG, "the fold needs gamma, beta and ln_stat");
  HIPCHK(hipSetDevice(c->cfg.device));
  hipStream_t st = (hipStream_t)stream;
  DBuf xs, ys, wf, cd;
  if (fold) {   // the product's weight side: W' = W diag(gamma) as split pairs, c = W' 1, d = W beta
    CHK(cd.ensure((size_t)2 * I * 4));
    CHK(ln_fold_weight(c, t->X, I, K, t->gamma, t->beta, wf, xs, cd.as<float>(), cd.as<float>() + I));
    HIPCHK(hipStreamSynchronize(nullptr));
  } else {
    CHK(xs.ensure((size_t)I * K * 4));
    CHK(enqueue_to_split(c, CFD_PROF_OTHER, st, t->X, xs.as<char>(), (long long)I, K, (long long)K, (long long)K * 4, nullptr));
  }
  const char* y = reinterpret_cast<const char*>(t->y_sp);
  if (!y) {
    CHK(ys.ensure((size_t)J * K * 4));
    CHK(enqueue_to_split(c, CFD_PROF_OTHER, st, t->Y, ys.as<char>(), (long long)J, K, (long long)K, (long long)K * 4, nullptr));
    y = ys.as<char>();
  }
  GemmArgs a = gemm_args();
  const int I0 = qkvt ? 2 * CFD_D : I;
  gemm_x(a, 0, xs.as<char>(), I0, K, (long long)K * 4);
  if (qkvt) {
    a.nslot = 2;
    gemm_x(a, 1, xs.as<char>() + (size_t)I0 * K * 4, CFD_D, K, (long long)K * 4);
  }
  gemm_y(a, y, J, (long long)K * 4);
  const float* cdp = cd.as<float>();
  auto fold_of = [&](const auto& e) {   // (q | k | v^T: group 1 is the value projection, rows I0.. of the weight)
    const int g1 = qkvt ? I0 : 0;
    return epi_ln(e, t->ln_stat, cdp, cdp + I, cdp + g1, cdp + I + g1, t->ln_eps);
  };
  auto cfg_used = [](int cfg) { return cfg == 1 || cfg == 6 || cfg == 19 || cfg == 20 || cfg == 24 ? cfg : 3; };   // (launch_gemm's default: 3)
  auto plain = [&](const auto& e) -> hipError_t {
    const int cfg = t->tile_cfg ? t->tile_cfg : gemm_auto_cfg<MODE_PLAIN>(a, 1, 1);
    t->tile_cfg_used = cfg_used(cfg);
    return launch_gemm<MODE_PLAIN>(a, e, 1, 1, st, cfg);
  };
  EpiF32 ef;
  memset(&ef, 0, sizeof(ef));
  ef.out = reinterpret_cast<float*>(t->out); ef.ldo = I; ef.bias = t->bias;
  EpiSplit es{reinterpret_cast<char*>(t->out), (long long)I * 4, 0, 0, t->bias, t->gelu, t->perm32};
  EpiQkvT eq{reinterpret_cast<char*>(t->out), (long long)I0 * 4, t->bias, reinterpret_cast<char*>(t->out2), t->natural};
  hipError_t err = hipSuccess;
  switch (kind) {
    case CFD_EPI_F32: err = plain(ef); break;
    case CFD_EPI_SPLIT: err = plain(es); break;
    case CFD_EPI_RESID: err = plain(EpiResid{t->x, 0, t->bias}); break;
    case CFD_EPI_RESID_STAT:
      t->tile_cfg_used = gemm_midsize_cfg<MODE_PLAIN>(a);
      err = launch_gemm_midsize<MODE_PLAIN>(a, EpiResidStat{t->x, 0, t->bias, reinterpret_cast<char*>(t->out), t->stat}, st);
      break;
    case CFD_EPI_QKVT: {
      const int cfg = t->tile_cfg ? t->tile_cfg : gemm_auto_cfg<MODE_GROUPED>(a, 1, 1);
      t->tile_cfg_used = cfg_used(cfg);
      err = launch_gemm<MODE_GROUPED>(a, eq, 1, 1, st, cfg);
      break;
    }
    case CFD_EPI_LN_F32: {
      t->tile_cfg_used = gemm_midsize_cfg<MODE_PLAIN>(a);
      err = launch_gemm_midsize<MODE_PLAIN>(a, fold_of(ef), st);
      break;
    }
    case CFD_EPI_LN_SPLIT: {
      t->tile_cfg_used = gemm_midsize_cfg<MODE_PLAIN>(a);
      err = launch_gemm_midsize<MODE_PLAIN>(a, fold_of(es), st);
      break;
    }
    default: {
      t->tile_cfg_used = gemm_midsize_cfg<MODE_GROUPED>(a);
      err = launch_gemm_midsize<MODE_GROUPED>(a, fold_of(eq), st);
      break;
    }
  }
  if (err != hipSuccess) return fail(CFD_E_HIP, "gemm launch failed: %s", hipGetErrorString(err));
  HIPCHK(hipStreamSynchronize(st));
  return CFD_OK;
}

// Micro-benchmark hook: `iters` launches of the MFMA GEMM (EpiResid epilogue: x[j][i] += D + bias) on device-resident
// SP operands filled from a float32 pattern; returns the average milliseconds per launch (HIP events).
extern "C" int cfd_bench_gemm(cfd_handle c, int I, int J, int K, int tile_cfg, int iters, float* ms_out) {
  if (!c || !ms_out || K % 32 || I % CFD_D || I < CFD_D || J < 1 || iters < 1) return fail(CFD_E_ARG, "bad argument (I must be a multiple of 512)");
  HIPCHK(hipSetDevice(c->cfg.device));
  DBuf xf, yf, xs, ys, out;
  CHK(xf.ensure((size_t)I * K * 4));
  CHK(yf.ensure((size_t)J * K * 4));
  CHK(xs.ensure((size_t)I * K * 4));
  CHK(ys.ensure((size_t)J * K * 4));
  CHK(out.ensure((size_t)J * I * 4));
  HIPCHK(hipMemset(out.p, 0, (size_t)J * I * 4));
  CHK(enqueue_philox_fill(xf.as<float>(), 1, I * K, 1ull, 0u, 0u, 3u, 0.05f, 0));
  CHK(enqueue_philox_fill(yf.as<float>(), 1, (int)((long long)J * K), 2ull, 0u, 0u, 3u, 1.0f, 0));
  if (getenv("CFD_BENCH_ZERO")) {   // power/clock probe: all-zero operands
    HIPCHK(hipMemset(xf.p, 0, (size_t)I * K * 4));
    HIPCHK(hipMemset(yf.p, 0, (size_t)J * K * 4));
  }
  CHK(enqueue_to_split(c, CFD_PROF_OTHER, 0, xf.as<float>(), xs.as<char>(), (long long)I, K, (long long)K, (long long)K * 4, nullptr));
  CHK(enqueue_to_split(c, CFD_PROF_OTHER, 0, yf.as<float>(), ys.as<char>(), (long long)J, K, (long long)K, (long long)K * 4, nullptr));
  GemmArgs a = gemm_args();
  gemm_x(a, 0, xs.as<char>(), I, K, (long long)K * 4);
  gemm_y(a, ys.as<char>(), J, (long long)K * 4);
  EpiResid e{out.as<float>(), 0, nullptr};
  EpiNull en{out.as<float>()};
  EpiF32 ef;
  memset(&ef, 0, sizeof(ef));
  ef.out = out.as<float>(); ef.ldo = I;
  const char* ev = getenv("CFD_BENCH_EPI");
  const int epi_kind = ev ? atoi(ev) : 0;   // 0 residual RMW, 1 no stores, 2 plain fp32 store, 3 split-pair store
  EpiSplit es;
  memset(&es, 0, sizeof(es));
  es.out = out.as<char>(); es.ldo = (long long)I * 4;
  if (epi_kind == 0 && I != CFD_D) return fail(CFD_E_ARG, "the residual epilogue has rows of 512");
  auto go = [&]() -> hipError_t {
    if (epi_kind == 1) return launch_gemm<MODE_PLAIN, EpiNull>(a, en, 1, 1, nullptr, tile_cfg);
    if (epi_kind == 2) return launch_gemm<MODE_PLAIN, EpiF32>(a, ef, 1, 1, nullptr, tile_cfg);
    if (epi_kind == 3) return launch_gemm<MODE_PLAIN, EpiSplit>(a, es, 1, 1, nullptr, tile_cfg);
    return launch_gemm<MODE_PLAIN, EpiResid>(a, e, 1, 1, nullptr, tile_cfg);
  };
  hipError_t err = go();   // warm-up
  if (err != hipSuccess) return fail(CFD_E_HIP, "gemm launch failed: %s", hipGetErrorString(err));
  HIPCHK(hipDeviceSynchronize());
  HIPCHK(hipEventRecord(c->pev[0], nullptr));
  for (int i = 0; i < iters; ++i) (void)go();
  HIPCHK(hipEventRecord(c->pev[1], nullptr));
  HIPCHK(hipEventSynchronize(c->pev[1]));
  float ms = 0.f;
  HIPCHK(hipEventElapsedTime(&ms, c->pev[0], c->pev[1]));
  *ms_out = ms / iters;
  return CFD_OK;
}

