/* libcfdenoise -- developer / test hooks (NOT part of the drop-in boundary: nothing in the reference corresponds to them).
 * Used by tests/ (kernel-level parity, stage-wise taps), tools/ (micro-benchmarks) and nothing in convofusion_amd's product path.
 * The product boundary is include/cfdenoise.h. */
#ifndef CFDENOISE_DEV_H
#define CFDENOISE_DEV_H
#include "cfdenoise.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Test hook: D[j][i] = sum_k X[i][k] Y[j][k] through the split-pair (fp16 hi/lo, 3 MFMAs per product) kernel.
 * X dev float32 [I][K], Y dev float32 [J][K], out dev float32 [J][I]; K % 32 == 0, I % 4 == 0.
 * tile_cfg: 0 = chosen from the shape; 1 = 128x128 (2-stage), 6 = 128x112 (2-stage), 19 = 64x64 (3-stage), 20 = 32x128 (3-stage),
 * 24 = 128x64 (3-stage), any other value = 128x16 (2-stage) (csrc/gemm_sp.hpp: launch_gemm). */
int cfd_test_gemm(cfd_handle h, const float* X, const float* Y, float* out, int I, int J, int K, int tile_cfg,
                  void* stream);

/* Test hook: one launch of the split-pair GEMM D[j][i] = sum_k X[i][k] Y[j][k] with one of the product's epilogues (csrc/gemm_sp.hpp).
 * The float32 operands are split as cfd_test_gemm splits them; split-pair outputs are returned as stored (per row and 32-column block:
 * 64 bytes of hi, then 64 bytes of lo), not decoded.  Synchronizes before returning. */
enum {
  CFD_EPI_F32 = 0,         /* out f32 [J][I] = D + bias                                                                         */
  CFD_EPI_SPLIT = 1,       /* out SP [J][I] = split(act(D + bias)); act = GELU if gelu; perm32: the P-fragment column order     */
  CFD_EPI_RESID = 2,       /* x f32 [J][512] += D + bias                                                                        */
  CFD_EPI_RESID_STAT = 3,  /* EPI_RESID + out SP [J][512] = split(x_new) + stat f32 [J][16][2] = (mean, M2) per 32-column slot  */
  CFD_EPI_QKVT = 4,        /* grouped, I = 1536: rows 0..1023 of X -> out SP [J][1024] = split(D + bias); rows 1024..1535 ->
                              out2 SP [J/16][512][32] = the value projection transposed (key order: natural, else 4q+r -> 8q+r) */
  CFD_EPI_LN_F32 = 5,      /* the LayerNorm fold: D taken as X LN(y; gamma, beta), then EPI_F32                                */
  CFD_EPI_LN_SPLIT = 6,    /* the fold, then EPI_SPLIT                                                                          */
  CFD_EPI_LN_QKVT = 7      /* the fold (per group), then EPI_QKVT                                                               */
};
typedef struct cfd_test_epi_args {
  int kind;                /* CFD_EPI_*                                                                                         */
  int I, J, K;             /* K % 32 == 0; EPI_RESID*: I = 512; EPI_*QKVT: I = 1536, J % 16 == 0; split-pair outputs: I % 32 == 0;
                              EPI_*F32: I % 4 == 0                                                                              */
  int tile_cfg;            /* F32 / SPLIT / RESID / QKVT: the launch_gemm class (as cfd_test_gemm; 0 = the product's choice).
                              RESID_STAT and the LN kinds ignore it: they go through launch_gemm_midsize, as in the product      */
  int gelu, perm32, natural;
  const float* X;          /* dev f32 [I][K]; LN kinds: W before the fold (the hook folds gamma / beta into it)                */
  const float* Y;          /* dev f32 [J][K] (ignored if y_sp is set)                                                           */
  const void* y_sp;        /* optional dev SP [J][K]: the column operand as stored, e.g. a RESID_STAT launch's out              */
  const float* bias;       /* dev f32 [I] or null (EPI_*QKVT: required, [1024])                                                 */
  const float* gamma;      /* LN kinds: dev f32 [K]                                                                             */
  const float* beta;       /* LN kinds: dev f32 [K]                                                                             */
  const float* ln_stat;    /* LN kinds: dev f32 [J][16][2] per-row slot statistics (as RESID_STAT writes them)                  */
  float ln_eps;
  float* x;                /* EPI_RESID*: dev f32 [J][512], updated in place                                                    */
  void* out;               /* dev: see the kinds                                                                                */
  void* out2;              /* EPI_*QKVT: dev SP [J/16][512][32]                                                                 */
  float* stat;             /* EPI_RESID_STAT: dev f32 [J][16][2]                                                                */
  int tile_cfg_used;       /* out: the class launched (1, 3, 6, 19, 20 or 24)                                                   */
} cfd_test_epi_args;
/* Fails with CFD_E_ARG, before any launch, where an argument breaks the constraints above. */
int cfd_test_gemm_epi(cfd_handle h, cfd_test_epi_args* args, void* stream);

/* Test hooks: stop the forward pipeline after tap point `stage` (0 = off; 1 = after the latent embedding;
 * 2+4l / 3+4l / 4+4l / 5+4l = layer l after self-attention / time block 1 / cross-attention / the layer),
 * and read an internal float32 buffer ("x" residual stream [M][512], "temb", "ss", "eps", "sc": the scores of
 * the three-launch and row-tile cross-attention, which only those paths allocate).
 *   "xa.info"  [7]  the cross-attention of the last cfd_forward: the xattn_fused_kernel instance its layers launched (0: split pairs,
 *                   1: ATT, keeps the maps, 2: F16, single-fp16 tiles; -1: none -- the three-launch path, the row-tile path, or a stop
 *                   stage in front of the first block), then of its work list: workgroups (0: no list), the most query tiles of a
 *                   workgroup (1, 2 or 4), the most single-fp16 segments (n16) and the most segments (nseg) of a workgroup, whether a
 *                   list flushes the accumulator between two online memories (0 / 1), and the one-key memory added as a vector (-1: none) */
int cfd_debug_stop_stage(cfd_handle h, int stage);
/* Test hook: the operand policy of the handle's cfd_forward calls (a sampling run has cfd_sample_args.operand_policy; nothing else reads
 * this).  policy = 0 (the default): split pairs, the launch sequence and every kernel are what they are without the hook.  policy = 15:
 * cfd_forward asks for the single-fp16 key / value tiles of its long memories exactly as cfd_sample_begin does, so the fused cross-attention
 * runs its F16 instance (csrc/xattn_fused.hpp) on tiles xa_pack16_kernel packs in that call -- under the product's own conditions: one
 * timestep for all rows, no attention maps wanted, every memory's projections made once per call on the tile kernels (no row-tile path),
 * a non-empty fused work list, some memory of at least 128 padded keys.  Where one fails the forward silently runs split pairs, as a
 * sampling run would: read "xa.info".  Any other value: CFD_E_ARG; CFD_E_STATE while a sampling run is open.  A change of the value drops
 * what cfd_forward_same_memories would let the next call reuse (the work lists carry the tile format). */
int cfd_debug_forward_operands(cfd_handle h, int policy);
/* Micro-benchmark: average ms of `iters` launches of the [J x K] x [512 x K]^T residual GEMM (I must be 512). */
int cfd_bench_gemm(cfd_handle h, int I, int J, int K, int tile_cfg, int iters, float* ms_out);
/* cfd_debug_read also reads the taps the last cfd_vae_decode_vjp left in the handle's VAE workspace (float32; fp = nframes rounded up to
 * 16, token rows ((stack * bs + b) * fp + f); rows of 16-frame tiles wholly beyond a sequence's length read 0 in "vae.g.*" and are not
 * written in "vae.x.*"):
 *   "vae.g.<l>"   [2 * bs * fp][128]   the running gradient at layer l's output, as it enters the layer's backward
 *   "vae.dz.<l>"  [2][bs][16][128]     layer l's memory-side contribution to d_z (rows >= n_chunks: no meaning)
 *   "vae.x.<l>"   [2 * bs * fp][128]   the forward's stream at layer l's input; l = num_layers: the last layer's output
 *   "vae.info"    2 floats: the launches of the call, fp
 * ... and what the last cfd_t5_encode left on the handle:
 *   "t5.info"     4 floats: the launches of the call (5 per block + 1; 0: it was refused), its token rows n_seq * T, the workspace's bytes,
 *                 and how many of its products ran as 128 x 128 blocks (the others: 64 x 64; the bits are the same)
 *   "t5.x"        [n_seq * T][768]     the residual stream behind the last block, in front of the final norm
 *   "t5.h"        [n_seq * T][768]     the last block's stream behind its attention: h = x + ctx Wo^T
 *   "t5.qkv"      [n_seq * T][2304]    the last block's q | k | v rows
 *   "t5.ctx"      [n_seq * T][768]     the last block's attention output, heads side by side
 *   "t5.f"        [n_seq * T][3072]    the last block's feed-forward intermediate relu(rms(h) g2 Wi^T)
 * ... and the last cfd_audio_encode / cfd_audio_power:
 *   "audio.info"  4 floats: the launches of the call (0: it was refused), the frames per waveform 1 + n_samples / hop, the output rows
 *                 n_wave * max(n_win, 1), the workspace's bytes */
int cfd_debug_read(cfd_handle h, const char* what, float* dst_dev, size_t numel);

/* Test hook: stop the reverse sweep of a row-tile cfd_weg_eval (csrc/weg_rt.hpp, csrc/rowtile_bwd.hpp) behind one launch.
 * stop = 0: off.  stop = 16 l + k, k = 1 .. 9: behind launch B<k> of layer l (the top layer has no B1 .. B4); stop = 10: behind the
 * embedding's backward, the last launch.  Anything else: CFD_E_ARG.  CFD_E_STATE on a handle that has the row-tile evaluation off.
 * With a stop set, cfd_weg_eval
 *   - fails with CFD_E_STATE before any launch where its arguments are not eligible for the row-tile path;
 *   - enqueues its launches eagerly -- no capture, no replay, and the call does not count as a use of its graph key -- leaves the
 *     sweep behind the named launch, synchronizes, and delivers neither losses, max_att, grad nor *loss_host;
 *   - remembers which of its three rotating buffers holds the running gradient ("weg.g").
 * With stop = 0 the launch sequence and the graph keys are what they are without the hook.
 *
 * cfd_debug_read then reads the buffers of the evaluation's workspace, all float32 with the M = B * L token rows (b, t) -> b * L + t
 * dense (tiles are ragged in the kernels, not in memory):
 *   "weg.g"          [M][512]   the running gradient at the residual stream: behind B1 at the layer's output (= the next layer's
 *                               input), B3 after time block 2, B4 after the cross-attention, B6 after time block 1, B7 after the
 *                               self-attention, the embedding's backward at the embedding's output; CFD_E_STATE before the top
 *                               layer's B6 has written the first one.  "weg.g0" .. "weg.g2": the three buffers themselves
 *   "weg.dh"         [M][1024]  B1: gradient at the FFN pre-activation
 *   "weg.dy"         [M][512]   B2 / B5 / B9: gradient at the norm3 / norm2 / norm1 output
 *   "weg.dz"         [M][512]   B3 / B6: gradient at the SiLU output of time block 2 / 1 (the input of its last linear layer)
 *   "weg.dO"         [M][512]   B7: gradient at the self-attention core's output, before out_proj
 *   "weg.dqkv"       [M][1536]  B8: dq | dk | dv at the packed in-projection's output (dq at the UNSCALED query), heads side by side
 *   "weg.dP"         [M][Sp_tot] B4: gradient at the cross-attention probabilities.  Memory j owns the columns off_j .. off_j + Sp_j - 1,
 *                               Sp_j = S_j rounded up to 32, off_j = Sp_0 + .. + Sp_(j-1), Sp_tot = their sum; in B4's grid that is
 *                               16-key blocks in memory order.  Folded formulation: per (row, memory) the values differ from the
 *                               unfolded gradient by one constant (the value bias), which the softmax backward removes.  Columns
 *                               S_j .. Sp_j - 1 and masked keys hold finite values that B5 multiplies with probability 0
 *   "weg.x.<l>.<k>"  [M][512]   the saved residual stream: layer l's input (k = 0), after self-attention (1), time block 1 (2),
 *                               cross-attention (3), time block 2 (4).  The saved forward ends at the last layer's cross-attention:
 *                               points behind it are not written
 *   "weg.att" / "weg.d_att" [B][layers][L][S_tlsn]  the listener-text probabilities and the objective's gradient at them
 *   "weg.info"       [5]        launches of the last evaluation, Sp_tot, the rt_xbwd_dy_kernel instance (512 / 1024 keys), the objective
 *                               kernel (0: weg_focus_small_kernel, 1: weg_focus_kernel), the index of the buffer behind "weg.g" (-1: none)
 * cfd_debug_weg_fill sets the gradient buffers (g0 .. g2, dh, dy, dz, dO, dqkv, dP) to `value`, e.g. a NaN: what a stopped sweep has
 * not written yet must still hold it.  Needs a completed row-tile evaluation (the workspace exists from then on). */
int cfd_debug_weg_stop(cfd_handle h, int stop);
int cfd_debug_weg_fill(cfd_handle h, float value);
/* Test hook: ONE launch of a focus kernel as cfd_weg_step launches it -- cfd_weg_focus's arguments, except that the focus tables are
 * HOST (they are checked against every row's slice and staged by the hook), plus
 *   last_rows  HOST [B] or NULL: every row its own slice [1, last_rows[b]) (each checked: 3 <= last_rows[b] <= last); `last` is the
 *              widest slice, which sizes the workspace blocks and decides the small kernel's eligibility.  NULL: the one slice [1, last)
 *   per_row    1: d_att = d losses[b] / d att[b];  0: d mean_b losses[b] / d att (cfd_weg_focus's scale)
 *   small      1: weg_focus_small_kernel (CFD_E_ARG unless L * (last - 1) <= 1024, nt_max <= 64, L <= 64);  0: weg_focus_kernel
 * workspace dev >= B * (3 * L * (last - 1) + 3 * nt_max) floats (unused by the small kernel, still required).  With last_rows NULL and
 * per_row 0 both kernels return cfd_weg_focus's bits.  The call waits for the launch. */
int cfd_test_weg_focus_rows(cfd_handle h, const float* att, int B, int NL, int L, int S, const int32_t* tok_off, const int32_t* tok_idx,
                            const int32_t* last_rows, int last, int nt_max, const float kernel3[3], int per_row, int small, float* workspace,
                            float* losses, float* max_att, float* d_att, void* stream);
/* Test hook: the FFT stage of cfd_audio_encode alone -- the same device function (csrc/audio_fe.hpp) on the same frames, without
 * normalisation: power [n_wave][1 + n_samples / hop][n_fft / 2 + 1] = |rfft(window * frame)|^2.  wave, twiddle, window as in
 * cfd_audio_args; the same refusals for n_fft, hop, n_wave and n_samples.  One launch. */
int cfd_audio_power(cfd_handle h, const float* wave, int n_wave, long long n_samples, int n_fft, int hop, const float* twiddle,
                    const float* window, float* power, void* stream);
/* Test hook (no handle): the device buffers the library holds in this process, over all handles and calls -- how many, and their bytes as asked
 * for.  Every buffer belongs to a handle or to one call: a reading is back at an earlier one once the handles created since are destroyed. */
int cfd_debug_live_buffers(long long* count, long long* bytes);
/* Test hook: the bytes of the handle's VAE decode workspace as allocated (it only ever grows): after a forward-only cfd_vae_decode on a
 * fresh handle, the forward-only layout's bytes (include/cfdenoise.h states them per row); after a saving forward, the VJP layout's. */
int cfd_debug_vae_workspace(cfd_handle h, long long* bytes);
/* Test hook (no handle, no device): the per-iteration coefficient rows a sampling run of scheduler `kind` (cfd_sample_args.scheduler)
 * over the HOST timestep table timesteps[0..N) uploads -- out HOST float32 [N][8], per row: sigma_t, alpha_t, c0, cx, sigma, use_noise,
 * order, 1/r0 (csrc/rows.hpp StepCoef; kind 2: c0 = sigma_prev / sigma_t, cx = alpha_prev (exp(-h) - 1)).  alphas_cumprod HOST
 * float32 [T]; n_inf: the count given to set_timesteps (DDPM / DDIM stride).  Fails with CFD_E_ARG where cfd_sample_begin would. */
int cfd_test_step_coefficients(int kind, const float* alphas_cumprod, int T, int n_inf, const int32_t* timesteps, int N, float eta,
                               int set_alpha_to_one, float* out);
/* Test hook (no handle, no device): the stride cfd_sample_parallel takes after a sweep.  err HOST float32 [p][B] (row k: the squared change
 * of X(i0 + k); row 0 is not read), coef HOST float32 [N][8] rows as cfd_test_step_coefficients writes them (sigma and use_noise are read),
 * the window i0 .. i0 + p - 1 inside the N iterations.  Returns the stride in [1, p], or CFD_E_ARG. */
int cfd_test_picard_stride(const float* err, int B, int p, int i0, const float* coef, int N, float tolerance, int L);

/* Test hook: the kernels of a cfd_sample_parallel sweep around the forward, on the caller's predictions -- the product's own kernel
 * instances with the grids and blocks the call itself launches them with; no weights, no run.  X(i), the latent entering iteration i,
 * is slot (N - i) % slots of the ring (slots = N + 1: a caller's trajectory; slots = J + 1: the call's own ring).  The batch is the J
 * levels base .. base + J - 1, its first `off` levels final already.  The stages of `stages` run in the order of the bits. */
enum {
  CFD_PICARD_FILL = 1,     /* X(i) = X(fill_src) for i = fill_lo .. fill_hi (fill_hi < fill_lo: no launch, as the call skips it)        */
  CFD_PICARD_LOAD = 2,     /* sample_sp row ((lv * G + g) * B + b) * L + l = split(X(base + lv)[b][l]), every g < G                      */
  CFD_PICARD_STEP = 4,     /* s[lv] = the DDPM step of X(base + lv) under the combined prediction, lv >= off (others not written)       */
  CFD_PICARD_SCAN = 8      /* X(i0 + k) = fl(s + fl(Xn - X)) for k = 1 .. J - off (i0 = base + off), in place; err[k][b] = the squared
                              change of X(i0 + k) for 1 <= k <= min(J - off, J - 1), 0 in every other row                               */
};
typedef struct {
  int stages;              /* CFD_PICARD_* bits                                                                                         */
  int B;
  int L;
  int G;                   /* the evaluated chunks of a level                                                                           */
  int N;
  int slots;               /* J + 1 <= slots <= N + 1                                                                                   */
  int base;
  int off;                 /* 0 <= off < J                                                                                              */
  int J;                   /* base + J <= N                                                                                             */
  float* ring;             /* dev f32 [slots][B][L][128], updated in place (FILL, SCAN)                                                 */
  int fill_src;            /* FILL: iterations in [0, N]                                                                                */
  int fill_lo;
  int fill_hi;
  void* sample_sp;         /* LOAD out: dev SP [J * G * B * L][128], as stored (cfd_test_gemm_epi: per row and 32-column block 64 bytes
                              of hi, then 64 bytes of lo)                                                                               */
  const float* eps;        /* STEP: dev f32 [J][G][B][L][128]                                                                           */
  const float* coef;       /* STEP: HOST f32 [N][8], rows as cfd_test_step_coefficients writes them (uploaded by the hook)              */
  int Gc;                  /* STEP: the chunks of the combine, 1 <= Gc <= 8                                                             */
  int pos[8];              /* STEP: chunk k < Gc of the combine is evaluated chunk pos[k] < G                                           */
  float w[8];              /* STEP: guidance weights (read without a weight table)                                                      */
  int clip;
  const float* wtab;       /* STEP: optional dev f32 [N][B][8]: the weighted kernel instance                                            */
  const float* noise;      /* STEP: dev f32 [N][B][L][128], or NULL: Philox stream 0 with step index i under seed / first_utterance     */
  unsigned long long seed;
  unsigned int first_utterance;
  float* s;                /* STEP out, SCAN in: dev f32 [J][B][L][128]                                                                 */
  float* err;              /* SCAN out: dev f32 [J][B]                                                                                  */
} cfd_test_picard_args;
/* Fails with CFD_E_ARG, before any launch, on a null pointer a requested stage needs or a size outside the constraints above.
 * Synchronizes before returning. */
int cfd_test_picard_sweep(cfd_handle h, const cfd_test_picard_args* args, void* stream);

#ifdef __cplusplus
}
#endif
#endif
