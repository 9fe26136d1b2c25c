// libcfdenoise: how one problem's forward runs -- decided ONCE per problem (setup_problem, cfd_problem.hip) by decide_forward_path below,
// from the handle's developer knobs, the problem's shapes and what the caller asks for, and only read from then on (Problem::path).
// This is the one place where those conditions are written: a new run kind, kernel instance or knob changes this function and its
// table in tests/host/forward_path_test.cpp.  Plain C++: no HIP header, no device code.
#pragma once

enum { FP_NMEM = 5 };                                       // memories of a problem (CFD_NMEM)
enum { XATTN_ROWTILE = 0, XATTN_FUSED = 1, XATTN_THREE = 2 };   // the cross-attention block: rt_xscore / rt_xpv, xattn_fused_kernel, or score products -> softmax -> P.V products
enum { XA_INST_NONE = -1, XA_INST_PAIR = 0, XA_INST_ATT = 1, XA_INST_F16 = 2 };   // xattn_fused_kernel<ATT, F16>; the value "xa.info" reports

// The developer knobs of DESIGN.md section 10 that bear on the path (Ctx), the test hook, and the kernels' own limits
struct PathKnobs {
  bool rt_on = true;              // CFD_ROWTILE
  long long rt_max_rows = 700;    // CFD_ROWTILE_MAX_ROWS
  bool fused_xattn = true;        // CFD_FUSED_XATTN
  int min_wgs = 6;                // CFD_FUSED_XATTN_MIN_WGS
  bool share0 = true;             // CFD_SHARE0
  int ln_fold = -1;               // CFD_LN_FOLD: 0 off, 1 wherever the launches allow it, -1 by shape
  int stop_stage = 0;             // the forward runs under cfd_debug_stop_stage (0: no): every row runs every launch it reaches, every LayerNorm is
                                  // launched; stages 1 .. 3 end it in front of layer 0's cross-attention
  int rt_max_l = 32, rt_max_keys = 1024;   // RT_MAX_L, RT_MAX_KEYS (rowtile.hpp)
  int xa_tiles = 4, f16_min_keys = 128;    // XA_TILES, XA_F16_MIN_KEYS (xattn_fused.hpp)
};

struct PathShape {
  int Be = 0, L = 0;
  int tmode = 0;                  // 0: one timestep for all rows, 1: one per row, 2: a level batch
  int S[FP_NMEM] = {0, 0, 0, 0, 0};
};

// What the caller asks of the problem's forwards
struct PathAsk {
  bool att_out = false;           // every row's attention maps (cfd_forward's att, the WEG evaluation's text maps)
  int ring_row0 = 0, ring_rows = 0;   // a sampling run's attention ring: the batch rows that keep their maps (0 rows: no ring)
  int dynamic_mask = 0;           // bit j: memory j is rewritten between the forwards of a run
  bool f16 = false;               // a non-zero operand policy: single-fp16 key / value tiles of the long memories where the fused kernel allows them
  int chunk_rows = 0;             // the batch is replicas (chunk-major) of these first rows, identical up to the first cross-attention; 0: arbitrary rows
  long long max_rows = 0;         // the caller's own limit on the token rows of the row-tile path, in place of the knob's rt_max_rows (cfd_denoise_guide:
                                  // guide_max_rows -- its backward runs on no other kernels, so the forward's crossover is not its limit); 0: the knob's
};

struct ForwardPath {
  bool rt = false;                // the forward: the row-tile kernels (rowtile.hpp; every memory static) or the tile kernels
  int xattn = XATTN_THREE;
  int xa_inst = XA_INST_NONE;     // the fused kernel's instance; NONE: another cross-attention runs
  bool xa_reached = true;         // the forward gets as far as a cross-attention (no stop stage in front of layer 0's): else "xa.info" reports NONE
  bool xa_list = false;           // the fused kernel's work list is built (knob and length gate; the row-tile path builds it too, unused)
  int f16_mask = 0;               // F16 instance: bit j, memory j is long enough for single-fp16 tiles (its segments carry XA_F16)
  bool share = false;             // layer 0's head -- everything before the first cross-attention -- once per utterance, ...
  int share_rows = 0;             // ... for these first rows, copied to the other chunks
  bool ln_fold = false;           // the algebraic LayerNorm fold of mid-size problems (gemm_sp.hpp EpiLn / EpiResidStat)
  bool rows_now = false;          // the launches get this step's rows of the per-step tables as pointers (rt_cur in a run) instead of a step index
  int dstep_slot = 0;             // the slot of Work::d_step that names the table row: 0 the loop index, 1 the constant 0
  int static_mask = 0;            // bit j: memory j's projections are made once per run / call (prepare_static_memside), not per forward
  bool keeps_maps() const { return xa_inst == XA_INST_ATT; }   // the fused kernel keeps the maps itself (+ att_fixup_kernel)
};

inline ForwardPath decide_forward_path(const PathKnobs& k, const PathShape& s, const PathAsk& a) {
  ForwardPath p;
  const bool stop = k.stop_stage != 0;
  p.xa_reached = !stop || k.stop_stage > 3;
  const long long M = (long long)s.Be * s.L;
  const int all = (1 << FP_NMEM) - 1;
  int sp_tot = 0, long_mask = 0;
  for (int j = 0; j < FP_NMEM; ++j) {
    const int sp = (s.S[j] + 31) / 32 * 32;
    sp_tot += sp;
    if (sp >= k.f16_min_keys) long_mask |= 1 << j;
  }
  // Small problems with one timestep for all rows and no memory rewritten under them: the row-tile kernels
  const long long row_limit = a.max_rows > 0 ? a.max_rows : k.rt_max_rows;
  p.rt = k.rt_on && s.tmode == 0 && s.L <= k.rt_max_l && M <= row_limit && sp_tot <= k.rt_max_keys && !a.dynamic_mask;
  // The fused kernel's work list.  A handful of workgroups cannot hide their serial walk over the key tiles: below min_wgs workgroups of
  // xa_tiles query tiles the three-launch path stays (build_xattn_worklist has the measurements).
  const long long wgs = ((long long)s.Be * ((s.L + 15) / 16) + k.xa_tiles - 1) / k.xa_tiles;
  p.xa_list = k.fused_xattn && wgs >= k.min_wgs;
  // Attention maps: the row-tile cross-attention stores them; on the tile kernels the fused kernel's ATT instance keeps them -- one
  // timestep, every memory static -- and otherwise the three-launch path's softmax writes them
  const bool maps = a.att_out || a.ring_rows > 0;
  const bool att_inst = maps && !p.rt && s.tmode == 0 && p.xa_list && !a.dynamic_mask;
  p.xattn = p.rt ? XATTN_ROWTILE : (p.xa_list && (!maps || att_inst)) ? XATTN_FUSED : XATTN_THREE;
  // Memory-side projections once per run / call: where a kernel that folds the timestep in by itself runs, with one timestep
  p.static_mask = (p.xattn != XATTN_THREE && s.tmode == 0) ? all & ~a.dynamic_mask : 0;
  // Single-fp16 tiles: the fused kernel on projections made once, no maps kept, some memory long enough
  const bool f16 = a.f16 && long_mask && p.xattn == XATTN_FUSED && !att_inst && p.static_mask == all;
  p.xa_inst = p.xattn != XATTN_FUSED ? XA_INST_NONE : att_inst ? XA_INST_ATT : f16 ? XA_INST_F16 : XA_INST_PAIR;
  p.f16_mask = f16 ? long_mask : 0;
  p.share = !p.rt && k.share0 && !stop && a.chunk_rows > 0 && s.Be % a.chunk_rows == 0 && s.Be > a.chunk_rows;
  p.share_rows = p.share ? a.chunk_rows : 0;
  // The fold's range: the launches launch_gemm gives the 64 x 64 / 128 x 64 classes anyway (below: the row-tile path or a handful of
  // workgroups; above: the 128 x 128 class, where a ln_rows launch costs less than the producer's wider epilogue)
  p.ln_fold = !p.rt && k.ln_fold != 0 && s.L == 16 && !stop && (k.ln_fold > 0 || (M >= 512 && M <= 3840));
  p.rows_now = s.tmode == 0;
  p.dstep_slot = s.tmode ? 1 : 0;
  return p;
}
