// libcfdenoise internals shared by the translation units of the library (cfd_core / cfd_problem / cfd_forward / cfd_sample / cfd_blocks / cfd_weg /
// cfd_grad / cfd_dev .hip): the handle, the per-problem workspace, error and launch helpers, and the functions one unit calls in another.
// gfx950 only; no CPU fallback anywhere.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <algorithm>
#include <map>
#include <string>
#include <vector>

#include "../../include/cfdenoise.h"
#include "../../include/cfdenoise_dev.h"
#include "owned.hpp"
#include "forward_path.hpp"
#include "gemm_sp.hpp"
#include "rows.hpp"
#include "attn_fused.hpp"
#include "xattn_fused.hpp"
#include "rowtile.hpp"

static const char* MEM_NAMES[CFD_NMEM] = {"spkemb", "alsn", "tlsn", "apb", "lsnemb"};

struct LayerW {
  DBuf wqkv_sp, bqk, wo_sp, bo2, wtb1_sp, wtb2_sp, w1_sp, w2_sp, cross_bias;
  DBuf wqkv_rt_sp, wo_rt_sp;   // the row-tile path's copies of wqkv_sp and wo_sp: split pairs of CFD_SAW_SCALE x the weights (cfd_common.hpp)
  // the LayerNorm fold's operands (gemm_sp.hpp EpiLn): W' = W diag(gamma) as split pairs for q | k, v and FFN1, and per output feature
  // c = W' 1, d = W beta in ln_cd: [c_qk 1024][d_qk 1024][c_v 512][d_v 512][c_1 1024][d_1 1024]
  DBuf wqk_f, wv_f, w1_f, ln_cd;
  const float *ln1g, *ln1b, *tb1g, *tb1b, *btb1, *ln2g, *ln2b, *tb2g, *tb2b, *btb2, *ln3g, *ln3b, *b1, *b2;
};

// The five row maps of a problem on the host (fetch_row_maps, cfd_problem.hip): memory j's instance of batch row b, range-checked
struct HostMaps {
  std::vector<int> m[CFD_NMEM];
};
static_assert(FP_NMEM == CFD_NMEM, "forward_path.hpp counts the memories itself");

// One problem: shapes, pointers and -- `path` -- how its forward runs.  setup_problem (cfd_problem.hip) fills it, path included
// (decide_forward_path, forward_path.hpp: the only place where the conditions are written, from the knobs, the shapes and what the caller
// asks for); the work lists are built for that path, and every launch sequence only reads it: path.rt picks enqueue_rows_rt or enqueue_rows,
// path.xattn the cross-attention block of enqueue_rows, path.xa_inst the fused kernel's instance ("xa.info"), path.static_mask the
// memories whose projections prepare_static_memside makes once.  Nothing changes the path after setup_problem.
struct Problem {
  ForwardPath path;
  int Be = 0, L = 0;
  long long M = 0;
  int U[CFD_NMEM], S[CFD_NMEM], Sp[CFD_NMEM], off[CFD_NMEM], Sp_tot = 0;
  const float* mem[CFD_NMEM];
  const int* map[CFD_NMEM];
  const uint8_t* mask[CFD_NMEM];
  int has_mask[CFD_NMEM];
  float* att[CFD_NMEM];
  // attention ring of a sampling run (cfd_sample_args::att_ring): only the batch rows [att_b0, att_b0 + att_nb) write their maps, into
  // slot *d_step of att[j] (att_slot[j] floats per slot), as rows 0 .. att_nb - 1 of that slot.  att_nb == 0: att[j] is one [Be][nl][L][S_j] block.
  // (path.keeps_maps(): the fused cross-attention kernel's ATT instance + att_fixup_kernel write them; every row's for cfd_forward's att)
  int att_b0 = 0, att_nb = 0;
  bool prev_same = false;       // setup_problem: the workspace still holds the previous cfd_forward's projections of memories of these shapes
  long long att_slot[CFD_NMEM] = {0, 0, 0, 0, 0};
  int tmode = 0;  // 0: all rows share the timestep of table row *d_step ; 1: row b uses table row b ; 2: a level batch (below)
  // Level batch (cfd_ddpm_invert, tmode 2): the batch is J levels of lv_rows rows each, level-major; every row of level lv uses table row
  // lv_i0 + lv, and memory j's U[j] = J * lv_U[j] instances are the caller's lv_U[j] distinct memories once per level (instance
  // lv * lv_U[j] + u: memory u at level lv's timestep), reached through level row maps.
  int lv_rows = 0, lv_i0 = 0, lv_U[CFD_NMEM] = {0, 0, 0, 0, 0};
  // (path.share, sampling loop only: the batch is G replicas (chunk-major) of the same B latent rows, so everything before the first
  //  cross-attention -- embedding, layer 0's self-attention and first time block -- is identical for the G replicas of an utterance; it is
  //  computed for the first path.share_rows = B rows and copied to the other chunks.)
  int T = 1;      // rows in the temb tables
  // Rows that share one memory of the LARGEST memory type in long consecutive runs (the guidance batch repeats
  // the unconditional audio memory for 5 of its 7 chunks): their attention against that memory is one big
  // un-batched product per run instead of a 196-row product per batch row.
  int jbig = -1, nruns = 0, nlong = 0, nshort = 0;
  int run_row0[8], run_len[8], run_u[8];
  // fused cross-attention (xattn_fused.hpp): workgroups of the work list, 0 = the list was not built
  int xa_nwg = 0;
  int xa0_nwg_a = 0, xa0_nwg_b = 0;   // layer-0 de-duplication lists (build_xattn_layer0_lists); 0: one launch
  bool xa_flush = false;               // some work list flushes the accumulator between two online memories (XA_FLUSH)
  int xa_one = -1;                     // the one-key memory the fused cross-attention adds as a vector (xattn_fused.hpp, XAttnArgs::one_j), or -1
  int xa_tpw = 0, xa_n16 = 0, xa_nseg = 0;   // of the work list (build_xattn_worklist): the most query tiles, XA_F16 segments and segments of a workgroup ("xa.info")
  // (path.static_mask: memories whose folded projections are computed once for the run from the centred static part of the memory,
  //  prepare_static_memside; per step they only get their per-key scale and bias, mem_scale_all_kernel)
  int rt_use_inst = 0;                              // the row maps fit the kernel arguments (<= RT_ARG_ROWS rows, instances < 256)
  unsigned char rt_inst[CFD_NMEM][RT_ARG_ROWS];
};

struct RtSave {
  float* x[CFD_MAX_LAYERS + 1][5];   // [l][0] layer input, [1] after self-attention, [2] after time block 1, [3] after cross-attention, [4] after time block 2
  char* qk[CFD_MAX_LAYERS];
  char* vt[CFD_MAX_LAYERS];
  float* sc[CFD_MAX_LAYERS];    // e_s of the cross-attention (rowtile.hpp: rt_xscore_kernel) ...
  float* cst[CFD_MAX_LAYERS];   // ... and its cell statistics
  float* pre[CFD_MAX_LAYERS];
  bool whole = false;           // run the WHOLE network (cfd_denoise_vjp: the sweep is seeded at the output); false: stop behind the top layer's cross-attention
};

// The row-tile gradient engine (rt_grad.hpp: forward with saved activations and reverse sweep): the arena of saved activations and
// gradient buffers
struct RtGradState {
  std::vector<long long> sig;   // the caller (cfd_weg_eval / cfd_denoise_vjp / cfd_denoise_guide), shapes and pointers the arena and the problem of wk[1] were prepared for
  RtSave sv;
  float *att = nullptr, *d_att = nullptr, *fws = nullptr, *dP = nullptr, *G[3] = {nullptr, nullptr, nullptr}, *dz = nullptr, *dy = nullptr,
        *dh = nullptr, *dO = nullptr, *dqkv = nullptr;
  int launches = 0;
  int T = 1;                    // rows of wk[1]'s per-timestep tables: 1 (this call's timestep) or every timestep (reuse_memory_side == 2)
  // test hook (cfd_debug_weg_stop): leave the reverse sweep after launch 16 l + k (k = 1 .. 9: B1 .. B9 of layer l; 16 * 0 + 10: the embedding's
  // backward); 0 = run everything.  stop_gi: which of G[0..2] held the running gradient when enqueue returned (-1: none written yet)
  int stop = 0, stop_gi = -1;
  int B = 0, L = 0, Sp_tot = 0, St = 0;   // the shapes of the last launch sequence (rtgrad::begin_sequence; cfd_debug_read sizes its buffers by them)
  int dy_keys = 0, focus_large = 0;       // the rt_xbwd_dy_kernel instance (512 / RT_MAX_KEYS) and the objective kernel (1: weg_focus_kernel) it launched
};

// What the engine's callers -- cfd_weg_eval (cfd_weg.hip), cfd_denoise_vjp(_mem) and cfd_denoise_guide (cfd_grad.hip) -- keep on the
// handle from one call to the next.  They share wk[1], the arena and this state; what one of them left is never reused by another.
struct GradState {
  DBuf rt_ws;                   // the arena
  RtGradState rt;
  int t_host = 0;               // the call's timestep, copied to wk[1].trows in front of every launch sequence (one-row tables)
  int dstep_host = 0;           // ... and the table row it selects, copied to wk[1].d_step (0 for one-row tables, the timestep for full tables)
  // What the memory-side / time-only part of the last call depended on: caller, shapes, memory pointers, arena, table rows (and the
  // timestep of one-row tables).  rtgrad::begin_call compares and clears it, a call that succeeded stores it (rtgrad::finish_call;
  // cfd_weg_eval in its run()): a call that fails leaves nothing to reuse.
  std::vector<long long> sig;
  void invalidate() { sig.clear(); }   // cfd_load_tensor: the next call reuses no memory-side result (WegState keeps nothing that depends on a weight's values)
  // cfd_denoise_vjp_mem (rt_grad.hpp, MemGrad): float32 copies of the folded A | VV ([nl][512][5 x 512] each, memory j's columns at
  // 512 j) and c ([nl][5][512]), unscaled, from the float64 fold -- 2 x nl x 512 x 2560 x 4 B = 94 MB at nine layers -- built by the
  // first call that asks for a memory gradient (memw_wver: the weights' generation they were folded from) and freed with the handle;
  // the call's planes (dS', P', T, G, dn' per memory) and inverse row maps.
  DBuf memw_a, memw_v, memw_c, mem_ws, mem_inv;
  long long memw_wver = -1;
  std::vector<int32_t> mem_inv_host;
  DBuf guide_ws;                // cfd_denoise_guide (guide.hpp): the replicated input, the seeded cotangent, the per-chunk gradients, the direct term, the loss partials
  hipEvent_t ev = nullptr;      // cross-stream hand-over of the three callers, and of cfd_dyadic_steps (destroyed with the handle)
};

// What cfd_weg_eval alone (cfd_weg.hip) keeps on the handle from one evaluation to the next.
struct WegState {
  DBuf ws, tok;   // the float32 launch sequence's activation arena; the focus-token tables
  // cfd_weg_eval replays its launches (~400 of the float32 launch sequence, ~160 on the row-tile path) as a hipGraph.  A graph holds
  // its kernels' arguments BY VALUE, so everything the caller passes per call -- latents in, losses / max_att / grad out, the
  // timestep's sinusoid row -- goes through fixed staging buffers (io); round 1's attempt captured the caller's own pointers, which
  // are fresh torch tensors on every call, and so replayed against stale addresses ("wrong gradients when interleaved with the
  // sampling graph").  One graph per variant (full evaluation / memory-side results reused), keyed by everything else the launches
  // depend on; a key is run eagerly once (function attributes, warm-up) and captured on its second use.
  DBuf io;
  struct Graph {
    std::vector<long long> key;
    int uses = 0;
    GraphExec gx;
    void reset(const std::vector<long long>& new_key = {}) { *this = Graph{new_key}; }   // drop the graph; start counting the uses of `new_key`
  };
  Graph graph[2];               // [0] full evaluation, [1] memory-side results reused
  long long tok_version = 0;    // counts the uploads of the focus-token tables (part of a graph's key)
  std::vector<int32_t> tok_host;
  // cfd_weg_step (eager, no staging): room for x~ | g~ | the rows' steps, and the steps as the host handed them to the copy.  Its tables
  // share `tok` (offsets | indices | last_rows) and tok_host, so either call notices what the other left there.
  DBuf rows;
  std::vector<float> step_host;
};

// One problem's device workspace: what the launches of a forward touch.  setup_problem sizes it at its end, from the problem's path
// (buffers only grow: what an earlier problem's path needed stays); prepare_static_memside adds the once-per-run projections.
//   every path                      x, h_sp, o_sp, u_sp, eps, sample_sp, qkv_sp, n_sp / kall_sp / cb / vt_all, temb_tab / h1_tab / ss_tab / trows
//   path.xattn == XATTN_THREE       sc, p_sp (scores, probabilities)
//   path.rt                         sc, p_sp (e_s, the keys' scales), rt_cst, rt_vt
//   tile kernels at L == 16         vts_sp
//   path.ln_fold                    ln_stat
//   path.rows_now in a run (T > 1)  rt_cur
struct Work {
  Problem pb;
  // qkv_sp: SP rows of q | k | v (1536 columns) on the tile kernels at L != 16; q | k (1024 columns) for batch rows of 16 tokens and on the
  // row-tile path, whose V^T per batch row lives in vts_sp / rt_vt
  DBuf x, h_sp, qkv_sp, vts_sp, o_sp, u_sp, sc, p_sp, eps, sample_sp;
  DBuf ln_stat;                 // LayerNorm fold: per row 16 slots of (mean, M2) written by the producing residual product (EpiResidStat)
  DBuf n_sp[CFD_NMEM], kall_sp[CFD_NMEM], cb[CFD_NMEM], vt_all[CFD_NMEM];
  DBuf temb_tab, h1_tab, ss_tab, trows, iota, long_rows, short_rows, zero_mask;
  // timestep-independent memory-side projections (rows.hpp mem_center_kernel): per memory the dot products c_l . a_s (ca), |a_s|^2 (asq)
  // and, per table row t, A_l b_t / c_l . b_t (kbtab) and VV_l b_t (vbtab); b_t = centred timestep embedding.
  DBuf ca[CFD_NMEM], asq[CFD_NMEM], kbtab[CFD_NMEM], vbtab[CFD_NMEM], b_tab, b_sp, bsq, zeros512;
  DBuf xa_wgs, xa_segs, xa_stamps, xa0_wgs_a, xa0_segs_a, xa0_wgs_b, xa0_segs_b, xa_dedup, xa_one_va, xa_att_raw, xa_att_mc, xa_att_fin, xa_att_desc;
  DBuf d_step;  // [0] = loop index, [1] = constant 0, [2] = "this iteration's in-painting overwrite is done" (cfd_sample_inpaint)
  // the timestep-independent memory-side projections the last cfd_forward left in this workspace (cfd_forward_same_memories): valid only
  // from the end of a cfd_forward that made (or reused) all five until the next setup_problem on this workspace
  bool fwd_mem_valid = false;
  int fwd_U[CFD_NMEM] = {0, 0, 0, 0, 0}, fwd_S[CFD_NMEM] = {0, 0, 0, 0, 0}, fwd_Be = 0, fwd_L = 0;
  bool fwd_att = false;
  bool fwd_mask[CFD_NMEM] = {false, false, false, false, false}, fwd_map[CFD_NMEM] = {false, false, false, false, false};
  unsigned long long fwd_wver = 0;
  DBuf rt_vt, rt_cbt[CFD_NMEM];   // row-tile path: V^T of the self-attention, per-step key tables
  DBuf rt_cst;                    // row-tile path: the cross-attention's cell statistics, float4 [M][Sp_tot / 32] (rowtile.hpp, RtXArgs::cst)
  DBuf k16[CFD_NMEM], v16[CFD_NMEM];   // single-fp16 key / value tiles of the static memories (xa_pack16_kernel), for the memories of path.f16_mask
  DBuf rt_cur;                    // sampling run with one timestep for all rows: this step's rows of every per-step table (refresh_step_rows)
  // What the timestep-only tables of this workspace were built from: the table rows' timesteps and the weights' generation.  temb / AdaLN
  // rows (20 launches) and, per memory, A_l b_t / VV_l b_t (kbtab / vbtab: two products each) depend on nothing else, so a run that
  // finds them built for its own timestep list skips them (the rollout opens eleven 1000-step runs per sample, unbounded_synthesis.py:285-468).
  std::vector<int32_t> tt_key;
  long long tt_wver = -1;
  int tt_mem_mask = 0;            // bit j: kbtab[j] / vbtab[j] (and b_tab / b_sp / bsq) hold the products for tt_key
  // Where the launches of the current problem find this step's AdaLN rows, A b / VV b vectors and row-tile key tables (the tables
  // themselves, or their rows' copies in rt_cur); set by refresh_step_rows at the start of a launch sequence, read by both sequences and
  // the reverse sweep (rt_grad.hpp)
  const float* now_ss = nullptr;
  const float* now_kb[CFD_NMEM] = {nullptr, nullptr, nullptr, nullptr, nullptr};
  const float* now_vb[CFD_NMEM] = {nullptr, nullptr, nullptr, nullptr, nullptr};
  const float* now_cbt[CFD_NMEM] = {nullptr, nullptr, nullptr, nullptr, nullptr};
};

// The kind of the open sampling run: which instances of begin_step_kernel / inpaint_now_kernel / cfg_step_kernel it launches
// (cfd_sample.hip: with_begin_args, enqueue_loop_iteration).  sample_begin starts every run from RunMode{}: a new field needs no reset;
// it is filled from its BeginExt field in init_latents_and_kind (the comment on BeginExt lists every place a new run kind touches).
struct RunMode {
  // Weighted run (cfd_sample_begin_weighted): the guidance weights come from SampleRun::wtab instead of cfd_sample_args::guidance_weight.
  bool weighted = false;
  // Edit run (cfd_sample_begin_edit): the run starts at iteration k0 of the full table (d_step[0] starts there; SampleRun::pos and iters
  // count executed iterations).  edit: the edit instances of begin_step_kernel / inpaint_now_kernel overwrite the tokens of ekeep
  // [B][L] with coef[i].sa * esrc + coef[i].sb * enoise.
  int k0 = 0;
  bool edit = false;
  // DDIM inversion run (scheduler kind 3) with a trajectory (cfd_sample_begin_invert): the caller's ring [iterations + 1][B][L][128]; the
  // trajectory instance of cfg_step_kernel stores the latents after iteration i into slot i + 1.
  float* traj = nullptr;
  // Anchored run (cfd_sample_begin_anchored): the anchored instances of begin_step_kernel / inpaint_now_kernel set the tokens of ekeep
  // to anchor_ring[anchor_n - i] (the caller's ring, read in place).
  bool anchor = false;
  const float* anchor_ring = nullptr;
  int anchor_n = 0;
  // Tied run (cfd_sample_begin_tied): the tied instances of begin_step_kernel / inpaint_now_kernel copy token etie[b][l] (-1: none) of
  // the run's own latents into token (b, l) at the start of every iteration, next to the edit instance's kept tokens; tie_final: the
  // copy after the last iteration (tie_copy_kernel, enqueued by the first cfd_sample_read that finds the run finished) has been done.
  bool tie = false;
  bool tie_final = false;
  // Replay of a recorded DDPM noise space (cfd_sample_begin_replay): the anchored instances over the caller's trajectory (anchor,
  // anchor_ring, anchor_n as above), the run's step noise = the caller's noise ring (args.step_noise), and a start at iteration k0.
  bool replay = false;
};

// The open sampling run (cfd_sample.hip): what sample_begin sets up, the captured iteration replays on and cfd_sample_read / _end
// settle.  While no run is open the level-batch calls (cfd_ddpm_invert, cfd_sample_parallel) use args, coef, wtab and latents as
// their scratch; their own buffers (lv_*, pic_*) are the handle's.
struct SampleRun {
  bool open = false;
  int pos = 0, iters = 0;            // executed iterations; loop iterations of the open run (= length of the timestep table)
  hipStream_t stream = nullptr;
  bool counts = false;               // the captured iteration contains launches that count into the saturation census (per-step projections)
  cfd_sample_args args;              // the run's copy of the caller's arguments: G = the evaluated chunks, no host pointers
  GraphExec graph;                   // the captured iteration
  DBuf latents, coef, inoise;
  DBuf hist;   // DPM-Solver++ runs (scheduler kind 2): [B][L][128] the previous iteration's x0 (CfgStepArgs::hist)
  // Internal chunk order of a sampling run: chunk k of the caller's chunk-major batch lives at rows
  // chunk_pos[k] * B.  Chunks whose rows all use ONE shared copy of the largest memory (the unconditional audio
  // memory: 5 of the 7 guidance chunks, not adjacent in the reference's order) are moved next to each other, so
  // their attention against it is one un-batched product instead of one per contiguous run.  Every per-row result
  // is unchanged (rows are independent); the guidance combine reads chunk k at its position.
  int chunk_pos[8];
  DBuf perm_map[CFD_NMEM];
  // The open run's mode and the buffers its instances read.  Weighted run: wtab [iterations][B][8] (indexed by the caller's chunk order);
  // wpos[k] is the row position of chunk k, or chunk 0's for a chunk the run does not evaluate.  esrc / enoise [B][L][128]: an edit's source
  // latents and the run's initial noise; ekeep [B][L]: the kept tokens of an edit, tied or anchored run; etie [B][L]: the tie table.
  RunMode mode;
  int wpos[8];
  DBuf wtab, esrc, enoise, ekeep, etie;
};

// Attention-concentration census of the last sampling run (cfd_sample_args::census_tau, cfd_sample_census; xattn_fused.hpp, XAttnArgs::census):
// buf is u32 [nl][XA_CEN_SLOTS][XA_CEN_STRIDE] per run, zeroed by cfd_sample_begin behind the warm-up iteration.  on: only while cfd_sample_begin
// enqueues the run's iteration (the captured graph keeps the pointers); hits: fused cross-attention launches that got a census slot.
struct AttnCensus {
  DBuf buf;
  bool on = false, valid = false, measured = false;
  int hits = 0;
  float tau = 0.f;
};

struct cfd_handle_s {
  cfd_config cfg;
  int nl = 0;
  bool finalized = false;
  std::map<std::string, DBuf> raw;
  std::map<std::string, size_t> raw_numel;
  // prepared weights
  DBuf we_sp, wp_sp, we_all, be_all;
  DBuf wp_f, ln_cd_p;           // the final norm folded into latent_proj: W' as split pairs; [c 128][d 128]
  DBuf wk_all_sp[CFD_NMEM], wv_all_sp[CFD_NMEM];
  std::vector<LayerW> lw;
  int qpe_rows = 0, mpe_rows = 0;
  // timestep sinusoid table
  DBuf tsin;
  int tsin_rows = 0;
  // workspaces (struct Work): wk[0] belongs to cfd_forward / the sampling run (its captured graph holds these pointers), wk[1] to the
  // row-tile gradient engine (GradState), which runs between two replays of an open run and must not disturb it; `w` is the one in use
  Work wk[2];
  Work* w = &wk[0];
  long long wver = 0;     // generation of the prepared weights (cfd_finalize_weights)
  int setup_launches = 0; // launches the last cfd_sample_begin spent on timestep-only tables (0: served from the cache); test / bench read-out
  // saturation census of THIS handle (cfd_common.hpp): sat[CFD_SAT_MEM] weights / memories / their projections, sat[CFD_SAT_IN] the
  // sample / latents handed to an entry point.  Zeroed at the entry of the calls that count, read at their end.
  DBuf sat;
  bool memside_in_forward = false;   // the last enqueue_denoise ran memory-side projections itself (not hoisted): census still open
  AttnCensus acen;
  unsigned int* sat_mem() const { return sat.as<unsigned int>() + CFD_SAT_MEM; }
  unsigned int* sat_in() const { return sat.as<unsigned int>() + CFD_SAT_IN; }
  int fwd_operands = 0;         // test hook (cfd_debug_forward_operands): 15 = cfd_forward asks setup_problem for single-fp16 tiles as a run would; 0 = pairs
  bool hint_same_mem = false;   // cfd_forward_same_memories: the promise for the NEXT cfd_forward ...
  bool hint_now = false;        // ... taken (and cleared) at that call's very first line, before anything can fail: a call that returns early
                                // must not leave the promise standing for the call after it
  bool census_pending = false;  // a cfd_weg_eval without loss_host left its census unread (it does not wait): settled by the next entry point
  // Developer knobs, read from the environment once per handle (cfd_create).  Each forces a path the library
  // also takes by itself for some shape or call; the parity tests use them as baselines.
  //   CFD_ROWTILE=0               no row-tile path (rowtile.hpp) for small problems: the tile kernels everywhere.  The row-tile path is
  //                               chosen by shape: at most rt_max_rows token rows of at most RT_MAX_L tokens per batch row, one timestep
  //                               for all rows, no dynamic memories
  //   CFD_ROWTILE_MAX_ROWS=<n>    moves that threshold
  //   CFD_GUIDE_MAX_ROWS=<n>      the token rows (Be * L) cfd_denoise_guide takes: its own limit, in place of rt_max_rows (PathAsk::max_rows)
  //   CFD_WEG_ROWTILE=0           cfd_weg_eval keeps the float32 launch sequence of weg_eval.hpp instead of the row-tile one (weg_rt.hpp, rt_grad.hpp)
  //   CFD_WEG_GRAPH=0             cfd_weg_eval always runs eagerly (WegState::graph)
  //   CFD_FUSED_XATTN=0           the three-launch cross-attention (score products -> softmax_rows_kernel -> P.V products) everywhere
  //                               instead of the fused kernel (xattn_fused.hpp)
  //   CFD_FUSED_XATTN_MIN_WGS=<n> the fewest workgroups a work list needs for the fused kernel
  //   CFD_L0_DEDUP=0              layer 0's cross-attention as one launch over all rows (build_xattn_layer0_lists)
  //   CFD_SHARE0=0                the pre-cross-attention part of layer 0 for every guidance replica (ForwardPath::share)
  //   CFD_PERMUTE=0               a sampling run keeps the caller's chunk order (chunk_pos)
  //   CFD_LN_FOLD=0 / 1           the algebraic LayerNorm fold of mid-size problems (cfd_forward.hip) off / wherever the launches allow
  //                               it; unset (-1): by shape
  //   CFD_XA_OPERANDS=0 / 15      overrides cfd_sample_args.operand_policy (the fused cross-attention's tile formats); unset: -1
  bool rt_on = true, weg_rt_on = true, weg_graph_on = true, fused_xattn = true, l0_dedup = true, share0 = true, permute = true;
  long long rt_max_rows = 700;    // measured crossover at the product shape (L = 16), seconds per 1000 steps, row-tile vs tile kernels (profiles/r05_rowtile_crossover.log:
                                  // the short cross-attention work lists of round 5 made the tile kernels faster): 5 utterances 1.04 / 1.22, 6: 1.18 / 1.24, 7: 1.34 / 1.23
  long long guide_max_rows = 4096;   // cfd_denoise_guide: the arena of saved activations is ~0.19 MB per token row at nine layers
  int fused_xattn_min_wgs = 6, ln_fold = -1, xa_operands = -1;
  // what decide_forward_path (forward_path.hpp) reads of the handle
  PathKnobs path_knobs() const {
    PathKnobs k;
    k.rt_on = rt_on; k.rt_max_rows = rt_max_rows; k.fused_xattn = fused_xattn; k.min_wgs = fused_xattn_min_wgs; k.share0 = share0;
    k.ln_fold = ln_fold; k.stop_stage = stop_stage;
    k.rt_max_l = RT_MAX_L; k.rt_max_keys = RT_MAX_KEYS; k.xa_tiles = XA_TILES; k.f16_min_keys = XA_F16_MIN_KEYS;
    return k;
  }
  GradState grad;              // the row-tile gradient engine's state between two calls (rt_grad.hpp)
  WegState weg;                // cfd_weg_eval's own state between two evaluations (cfd_weg.hip)
  // cfd_vae_decode / cfd_vae_decode_vjp / cfd_vae_decode_sweep (cfd_blocks.hip, vae_dec.hpp): the calls' own workspace; the shape of the
  // forward it holds; for cfd_debug_read ("vae.*"), where the last saving forward and its sweep left their taps (g null: none, the last
  // forward was forward-only); and the kept forward's ticket (0: none is kept; `dropped_by` then names the call that dropped the last one)
  struct VaeVjpState {
    DBuf ws;
    float *g = nullptr, *dzl = nullptr, *x0 = nullptr;
    int bs = 0, fp = 0, nl = 0, launches = 0, fwd_launches = 0, nframes = 0, n_chunks = 0;
    long long rows = 0;
    uint64_t ticket = 0, serial = 0;
    const char* dropped_by = nullptr;
    bool grew = false;            // ... and had to grow the workspace
  } vae;
  // cfd_t5_encode (cfd_text.hip, t5_enc.hpp): the call's workspace, sized from (n_seq, T) -- per token row x | h | q k v | ctx | f --, the
  // launches of the last call (0: it was refused; big_launches: those of its products that ran as 128 x 128 blocks), where it left the
  // residual stream and the last block's h, q | k | v, ctx and f (cfd_debug_read "t5.x", "t5.h", "t5.qkv", "t5.ctx", "t5.f"), and the
  // handle's device's compute units (what the products' block shape is chosen by)
  struct T5State {
    DBuf ws;
    float *x = nullptr, *h = nullptr, *qkv = nullptr, *ctx = nullptr, *f = nullptr;
    long long rows = 0;
    int launches = 0, big_launches = 0, n_cu = 0;
  } t5;
  // cfd_audio_encode / cfd_audio_power (cfd_audio.hip, audio_fe.hpp): the call's workspace -- per waveform the chunk maxima, peak and largest
  // Mel power, the Mel powers [n_wave][T][n_mels], and where the call needs them the dB rows and the MLP's two hidden layers --, the
  // launches of the last call (0: it was refused), its frames per waveform and its output rows.  cfd_audio_onsets (onset_fe.hpp) carves
  // the same buffer: peaks, Mel powers, frame energies, two onset slots of T frames per waveform and the counts
  struct AudioState {
    DBuf ws;
    long long frames = 0, rows = 0;
    int launches = 0;
  } audio;
  // cfd_audio_encoder_vjp (cfd_audio.hip, audio_enc_bwd.hpp): the call's workspace -- h1, h2, dz2, dz1 per row and, where the rows are
  // more than one segment, a plane of the six parameter gradients per segment --, the launches of the last call (0: it was refused),
  // its rows and its segments
  struct AudioEncVjpState {
    DBuf ws;
    long long rows = 0;
    int launches = 0, segments = 0;
  } audio_enc;
  // cfd_motion_eval / cfd_motion_diversity (cfd_metrics.hip, metrics_eval.hpp): the call's workspace -- the processed motions and embeddings
  // where the caller takes none, the embedding net's activations for 128 sequences, the diversity's block sums --, the launches of the last
  // call (0: it was refused) and its sequences
  struct MetricsState {
    DBuf ws;
    long long rows = 0;
    int launches = 0;
  } metrics;
  // profiling
  bool prof = false;
  hipEvent_t pev[2] = {nullptr, nullptr};
  float prof_ms[CFD_PROF_NCLASS];
  int prof_n[CFD_PROF_NCLASS];
  int stop_stage = 0;  // test hook: leave enqueue_denoise after this tap point (0 = run everything)
  hipStream_t own_stream = nullptr;  // non-blocking stream the captured loop iteration replays on
  SampleRun run;                     // the sampling run (one at a time)
  DBuf lv_map[CFD_NMEM], lv_mask[CFD_NMEM];   // level batches: the level row maps and the key-padding masks once per level
  DBuf pic_s, pic_part, pic_err;              // cfd_sample_parallel: the levels' steps [J][B][L][128], the error partials and sums
  // (cfd_destroy has waited for the device.)  The graphs go first, then the stream they replay on and the events; every buffer frees itself.
  ~cfd_handle_s() {
    run.graph.reset();
    for (WegState::Graph& g : weg.graph) g.reset();
    if (grad.ev) (void)hipEventDestroy(grad.ev);
    if (own_stream) (void)hipStreamDestroy(own_stream);
    for (hipEvent_t e : pev) if (e) (void)hipEventDestroy(e);
  }
};
typedef cfd_handle_s Ctx;

// Saturation census (cfd_common.hpp) of this handle.  sat_begin zeroes the two counters in stream order at the entry of a call that
// counts; check_saturation reads them (the caller has waited for the stream) and clears them, so an error is reported by the call
// whose launches counted it and never leaks into the next call or another handle.
static inline int sat_begin(Ctx* c, hipStream_t st) {
  HIPCHK(hipMemsetAsync(c->sat.p, 0, 8, st));
  return CFD_OK;
}
static inline int check_saturation(Ctx* c, const char* what) {
  unsigned int n[2] = {0, 0};
  HIPCHK(hipMemcpy(n, c->sat.p, 8, hipMemcpyDeviceToHost));
  if (n[0] == 0 && n[1] == 0) return CFD_OK;
  HIPCHK(hipMemset(c->sat.p, 0, 8));
  if (n[CFD_SAT_MEM])
    return fail(CFD_E_RANGE, "%s: %u groups of values exceed +-65504, the range of the fp16 split-pair operands (weights, centred memories and their "
                             "folded key / value projections must stay inside it); rescale the conditioning input", what, n[CFD_SAT_MEM]);
  return fail(CFD_E_RANGE, "%s: %u groups of values of the sample / latents exceed +-65504, the range of the fp16 split-pair operands", what, n[CFD_SAT_IN]);
}

// A cfd_weg_eval that does not wait (loss_host == NULL) cannot read its own census.  The next entry point of the handle does, before it
// zeroes or reads the counters for its own launches: nothing is dropped and nothing is blamed on the wrong call.
static inline int settle_deferred_census(Ctx* c) {
  if (!c->census_pending) return CFD_OK;
  c->census_pending = false;
  HIPCHK(hipStreamSynchronize(c->own_stream));
  return check_saturation(c, "an earlier cfd_weg_eval (latents, memories / their projections)");
}

static inline const float* rawp(Ctx* c, const std::string& name) {
  auto it = c->raw.find(name);
  return it == c->raw.end() ? nullptr : it->second.as<float>();
}

// Work done once per device (function attributes): `done` holds one bit per device ordinal -- a process may hold handles on several
// GPUs -- and the bit is set when `fn` has succeeded.
template <class Fn>
static inline int once_per_device(unsigned long long& done, int device, Fn&& fn) {
  const unsigned long long bit = 1ull << (device & 63);
  if (done & bit) return CFD_OK;
  CHK(fn());
  done |= bit;
  return CFD_OK;
}

// ---- profiling brackets ---------------------------------------------------------------------------
struct Bracket {
  Ctx* c;
  int cls;
  hipStream_t st;
  Bracket(Ctx* c_, int cls_, hipStream_t st_) : c(c_), cls(cls_), st(st_) {
    if (c->prof) (void)hipEventRecord(c->pev[0], st);
  }
  ~Bracket() {
    if (c->prof) {
      (void)hipEventRecord(c->pev[1], st);
      (void)hipEventSynchronize(c->pev[1]);
      float ms = 0.f;
      (void)hipEventElapsedTime(&ms, c->pev[0], c->pev[1]);
      c->prof_ms[cls] += ms;
      c->prof_n[cls] += 1;
    }
  }
};

template <int MODE, class Epi>
static int run_gemm(Ctx* c, int cls, const GemmArgs& a, const Epi& e, int nb, int nz, hipStream_t st, int cfg = 0) {
  Bracket br(c, cls, st);
  hipError_t err = launch_gemm<MODE, Epi>(a, e, nb, nz, st, cfg);
  if (err != hipSuccess) return fail(CFD_E_HIP, "gemm launch failed: %s", hipGetErrorString(err));
  return CFD_OK;
}

template <int MODE, class Epi>
static int run_gemm_midsize(Ctx* c, int cls, const GemmArgs& a, const Epi& e, hipStream_t st) {
  Bracket br(c, cls, st);
  hipError_t err = launch_gemm_midsize<MODE, Epi>(a, e, st);
  if (err != hipSuccess) return fail(CFD_E_HIP, "gemm launch failed: %s", hipGetErrorString(err));
  return CFD_OK;
}

static inline GemmArgs gemm_args() {
  GemmArgs a;
  memset(&a, 0, sizeof(a));
  a.nslot = 1;
  return a;
}
// Operand slot n of X: I rows of K columns (split pairs, row pitch ldx bytes), every row valid; the Y operand: J rows, likewise.
static inline void gemm_x(GemmArgs& a, int n, const char* X, int I, int K, long long ldx) {
  a.X[n] = X; a.ldx[n] = ldx; a.I[n] = I; a.Iclamp[n] = I; a.kt[n] = K / 32;
}
static inline void gemm_y(GemmArgs& a, const char* Y, int J, long long ldy) {
  a.Y = Y; a.ldy = ldy; a.J = J; a.Jclamp = J;
}

#define LAUNCH(cls, kernel, grid, block, st, ...) LAUNCH_AS(cls, #kernel, kernel, grid, block, st, __VA_ARGS__)
// (name: what a failed launch is called in the error -- for a kernel chosen through a template, whose expression names no instance)
#define LAUNCH_AS(cls, name, kernel, grid, block, st, ...)                                     \
  do {                                                                                         \
    Bracket _br(c, cls, st);                                                                   \
    hipLaunchKernelGGL(kernel, grid, block, 0, st, __VA_ARGS__);                               \
    hipError_t _e = hipGetLastError();                                                         \
    if (_e != hipSuccess) return fail(CFD_E_HIP, "%s launch failed: %s", name, hipGetErrorString(_e)); \
  } while (0)

// The launch of a unit that reports its launches ("audio.info", "audio_enc_vjp.info", "t5.info", "metrics.info", "vae.info", "weg.info"): launch with dynamic
// LDS bytes, check at once -- a failure names the kernel and returns before anything behind it is enqueued --, then count into `count`.
// A launch written with it cannot be left out of its unit's figure.  (No profiling Bracket: these units have no profile class.)
#define LAUNCH_COUNTED(count, kernel, grid, block, lds, st, ...) LAUNCH_COUNTED_AS(count, #kernel, kernel, grid, block, lds, st, __VA_ARGS__)
#define LAUNCH_COUNTED_AS(count, name, kernel, grid, block, lds, st, ...)                      \
  do {                                                                                         \
    hipLaunchKernelGGL(kernel, grid, block, lds, st, __VA_ARGS__);                             \
    hipError_t _e = hipGetLastError();                                                         \
    if (_e != hipSuccess) return fail(CFD_E_HIP, "%s launch failed: %s", name, hipGetErrorString(_e)); \
    ++(count);                                                                                 \
  } while (0)

// ---- small kernels of the host code itself (templates: each unit instantiates what it launches) -----------
template <int CFD_KI = 0>
__global__ void scale_copy_kernel(const float* in, float* out, long long n, float s) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) out[i] = in[i] * s;
}
template <int CFD_KI = 0>
__global__ void d2f_kernel(const double* in, float* out, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) out[i] = (float)in[i];
}
template <int CFD_KI = 0>
__global__ void f2d_kernel(const float* in, double* out, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) out[i] = (double)in[i];
}

// x[g][:] = x[0][:] for g = 1 .. G-1 (n4 float4 per replica): hands the shared pre-cross-attention state of layer 0
// to every guidance chunk
template <int CFD_KI = 0>
__global__ void replicate_rows_kernel(float4* x, long long n4, int G) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n4) return;
  const float4 v = x[i];
  for (int g = 1; g < G; ++g) x[(long long)g * n4 + i] = v;
}

// x~ of a tied run, replicated (cfd_denoise_guide: once per guidance chunk; cfd_weg_step: once): row c * n_tok / L + b of `xin` is
// x~[b], x with every tied token replaced by its source's value (tie == null: x itself).  One thread per float4 of the total4 written;
// a tie entry outside [0, n_tok) counts as free, so no table makes the kernel read out of bounds.
template <int = 0>
__global__ void guide_replicate_kernel(const float* __restrict__ x, const int32_t* __restrict__ tie, float* __restrict__ xin, long long n_tok,
                                       long long total4) {
  const long long i = blockIdx.x * 256LL + threadIdx.x;
  if (i >= total4) return;
  const long long tok = (i >> 5) % n_tok;
  long long src = tok;
  if (tie) {
    const int v = tie[tok];
    if (v >= 0 && v < n_tok) src = v;
  }
  reinterpret_cast<float4*>(xin)[i] = reinterpret_cast<const float4*>(x)[src * (CFD_LAT / 4) + (i & 31)];
}

template <int CFD_KI = 0>
__global__ void fill_f32_kernel(float* p, long long n, float v) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) p[i] = v;
}


// PRED: what `eps` holds (cfd_scheduler_step_pred: 0 the noise, 1 the clean latent -- rows.hpp, step_x0_of / step_eps_of)
template <int CFD_KI = 0, int PRED = 0>
__global__ void sched_step_kernel(const float* eps, const float* noise, float* x, size_t n, StepCoef c, int kind, int clip, float* x0_out) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const float e = eps[i], xv = x[i];
  const float x0 = step_x0_of<PRED>(c, clip, xv, e);
  if (x0_out) x0_out[i] = x0;
  float prev = (kind == 0) ? c.c0 * x0 + c.cx * xv : c.c0 * x0 + c.cx * step_eps_of<PRED>(c, xv, e);
  if (c.use_noise != 0.f) prev = prev + c.sigma * noise[i];
  x[i] = prev;
}
// DPM-Solver++ (2M) step on its own (cfd_dpmsolver_step): x0_out = this step's data prediction (the caller's history for the next step),
// x = the update; m_prev (the previous step's x0) is read by order-2 steps only.  PRED 1: the model output is the data prediction.
template <int CFD_KI = 0, int PRED = 0>
__global__ void dpmpp_step_kernel(const float* eps, const float* m_prev, float* x, float* x0_out, size_t n, StepCoef c) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const float xv = x[i];
  const float x0 = step_x0_of<PRED>(c, 0, xv, eps[i]);   // (no clip_sample in this scheduler)
  const float m1 = c.order == 2.0f ? m_prev[i] : 0.f;
  x0_out[i] = x0;
  x[i] = dpmpp_prev(c, xv, x0, m1);
}
template <int CFD_KI = 0>
__global__ void add_noise_kernel(const float* x0, const float* noise, float* out, size_t n, float sa, float sb) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) out[i] = sa * x0[i] + sb * noise[i];
}

// ---- functions one translation unit calls in another ---------------------------------------------------
// cfd_core.hip
int to_sp(Ctx* c, const float* src, long long R, int K, DBuf& dst, long long dst_rows = -1);
// float32 [R][K] (row pitch ld_src floats) -> split pairs (row pitch ld_dst bytes); `sat`: the census counter of the values' class, or null
int enqueue_to_split(Ctx* c, int cls, hipStream_t st, const float* src, char* dst, long long R, int K, long long ld_src, long long ld_dst, unsigned int* sat);
// the LayerNorm fold's weight side (cfd_core.hip, null stream): dst_sp = split(W diag(gamma)) [R][K], cvec = W' 1, dvec = W beta; tmp: scratch
int ln_fold_weight(Ctx* c, const float* W, int R, int K, const float* gamma, const float* beta, DBuf& tmp, DBuf& dst_sp, float* cvec, float* dvec);
// cfd_problem.hip: work lists, problem set-up, timestep tables, memory-side projections
// the memories' row maps on the host, `rows` entries each (rows_name: what the caller calls that count, for the message): the one place that
// downloads a row map.  A memory without a map gets the identity and must have one instance per row; every entry is checked against U.
int fetch_row_maps(const cfd_memory mem[CFD_NMEM], int rows, const char* rows_name, HostMaps& hm);
// What setup_problem, cfd_weg_eval and cfd_denoise_vjp(_mem) refuse alike, before anything is touched: weights and timestep table in
// place, B rows of an even L >= 2 tokens within the query PE, every memory present, within the memory PE and with one instance per row
// where it has no row map.  CALL_TIMESTEP: `timestep` is the call's one timestep and must lie in the table; CALL_ROW_MAPS: memories may
// come with row maps (without the flag one is refused, so that U == B for every memory).
enum { CALL_TIMESTEP = 1, CALL_ROW_MAPS = 2 };
int check_latent_call(Ctx* c, int B, int L, const cfd_memory mem[CFD_NMEM], int flags, int timestep = 0);
// maps: the host copy of mem[].row_map where the caller has it already (null: fetched here, unless cfd_forward keeps the previous call's lists);
// att: attention outputs [Be][nl][L][S_j] or null; ask: what else the caller asks of the forwards (forward_path.hpp)
int setup_problem(Ctx* c, int Be, int L, const cfd_memory mem[CFD_NMEM], const HostMaps* maps, float* const att[CFD_NMEM], const PathAsk& ask,
                  int tmode, int T);
int build_time_tables(Ctx* c, const int32_t* trows_host, int T, hipStream_t st);
int enqueue_time_tables(Ctx* c, int T, hipStream_t st);
int prepare_static_memside(Ctx* c, hipStream_t st, bool reuse = false);
int enqueue_memside(Ctx* c, hipStream_t st);
// cfd_forward.hip: the launches of one denoiser forward
int enqueue_rows(Ctx* c, hipStream_t st);
int enqueue_rows_rt(Ctx* c, hipStream_t st, const RtSave* sv = nullptr);
int enqueue_denoise(Ctx* c, hipStream_t st);
size_t step_rows_bytes(Ctx* c);   // what refresh_step_rows needs of Work::rt_cur for the current problem (0: its forwards refresh nothing)
// cfd_grad.hip (rt_grad.hpp): what cfd_weg.hip calls of the row-tile gradient engine, and the types those calls take
namespace rtgrad {
// Who prepared wk[1] and the arena: the three callers share both, and what one of them left is never reused by another.
enum { FOR_WEG = 0, FOR_VJP = 1, FOR_GUIDE = 2 };
struct WorkGuard {   // the launches of a call address Ctx::wk[1]; everything else of the handle keeps wk[0]
  Ctx* c;
  explicit WorkGuard(Ctx* c_) : c(c_) { c->w = &c->wk[1]; }
  ~WorkGuard() { c->w = &c->wk[0]; }
};
struct Call {   // one call on the engine, as begin_call takes it
  int who;                        // FOR_*
  int Be, L;                      // Be rows of L tokens
  const cfd_memory* mem;
  const HostMaps* maps;           // the host copy of the row maps, or null (no memory has one)
  std::vector<long long> more;    // what else of the caller's arguments the problem depends on (instance counts, row maps, guidance chunks)
  int mode;                       // reuse_memory_side: 0 / 1 / 2
  int timestep;
  // left by begin_call
  bool reuse = false;             // the memory side of the previous call stands: skip those launches
  std::vector<long long> sig;     // what finish_call stores for the next call to compare
};
// Where the reverse sweep starts.  d_out == null (cfd_weg_eval): at the text maps -- the top layer's B5 takes d_att alone, nothing above
// its cross-attention reaches the objective.  d_out (cfd_denoise_vjp, cfd_denoise_guide): the cotangent at the forward's output
// [M][128] -- one product through latent_proj, then the top layer's B1 .. B4 like every other layer's, with decoder.norm where a lower
// layer has the next layer's norm1 (and d_att all zero: the objective contributes nothing).
struct SweepSeed {
  const float* d_out = nullptr;
};
struct MemGrad;
void append_memories(std::vector<long long>& v, const cfd_memory* mem);   // S | data | key_padding_mask of each memory: the memories' part of every signature
const char* ineligible(Ctx* c, long long B, int L, const cfd_memory* mem, bool guide = false);
int begin_on_own_stream(Ctx* c, hipStream_t caller);
int begin_call(Ctx* c, Call& k, hipStream_t caller);
void begin_sequence(Ctx* c);
int enqueue_memory_side(Ctx* c, hipStream_t st);
int enqueue_forward_saved(Ctx* c, hipStream_t st, const float* latents);
int enqueue_reverse_sweep(Ctx* c, hipStream_t st, const SweepSeed& seed, float* grad, const MemGrad* mg = nullptr);
}  // namespace rtgrad
// cfd_sample.hip
int enqueue_philox_fill(float* out, int B, int per_utt, uint64_t seed, uint32_t step, uint32_t utt0, uint32_t stream_id, float scale, hipStream_t st);
// cfd_blocks.hip
int enqueue_linear_act(const float* x, long long n_rows, int K, const float* W, const float* b, int N, int act, float* out, hipStream_t st);
int vae_debug_buffer(Ctx* c, const char* what, float** p, size_t* n);   // the taps of the last cfd_vae_decode_vjp (cfd_debug_read "vae.*")
// The fused decode's call path, for cfd_denoise_guide_pose (cfd_grad.hip, guide.hpp), which decodes between its forward and its sweep:
// the limits of `p` (`who` names the caller in the message); the forward of `p` on the handle's VAE workspace (save: kept for the sweep;
// whatever forward the handle kept is dropped, and `who` is what a stale ticket's message names); the sweep over that forward.
constexpr int GUIDE_NFEATS = 189;   // the decoder's output features as guide.hpp indexes them (cfd_blocks.hip asserts VE_NFEATS is this)
int vae_decode_check(const char* who, const cfd_vae_decode_args* p);
int vae_decode_forward(Ctx* c, const char* who, const cfd_vae_decode_args* p, float* feats, bool save, bool copy_w, hipStream_t st);
int vae_decode_sweep(Ctx* c, const float* w, const float* d_feats, float* d_z, hipStream_t st);
