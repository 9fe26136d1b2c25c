/* libcfdenoise -- C ABI of the MI355X-native ConvoFusion denoising loop.
 *
 * The reference (m-hamza-mughal/convofusion) is pure Python/PyTorch and has no FFI; its plug point
 * for this path is `instantiate_from_config` on a dotted class path (convofusion/config.py:16-31,
 * configs/modules/denoiser.yaml:2, configs/modules/scheduler.yaml:2).  This header is the boundary a
 * replacement binds underneath that plug point: plain pointers and sizes, no torch types.  Each
 * entry point names the reference interface it replaces.  All `dev` pointers are device (HBM)
 * pointers, e.g. `tensor.data_ptr()`; the caller owns every buffer it passes.  A handle may be used
 * from one host thread at a time.  Every function returns 0 on success or a negative CFD_E_* code;
 * cfd_last_error() then describes the failure (the reference raises Python exceptions instead:
 * TypeError / ValueError / torch shape errors, denoiser.py:113,123,171,280).
 */
#ifndef CFDENOISE_H
#define CFDENOISE_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CFD_OK 0
#define CFD_E_ARG (-1)      /* bad argument / unsupported configuration (reference: TypeError/ValueError) */
#define CFD_E_SHAPE (-2)    /* shape the reference also rejects: odd L, L/2 or S beyond the PE buffers */
#define CFD_E_STATE (-3)    /* call order (weights not finalized, no sampling run open, ...) */
#define CFD_E_HIP (-4)      /* HIP runtime error */
#define CFD_E_RANGE (-5)    /* a weight, a centred memory row or a folded key / value projection of one exceeds +-65504, the range of the fp16
                               split-pair operands: the engine would clamp it silently (the reference is float32 and has no such limit);
                               rescale the offending conditioning input */

#define CFD_NUM_MEM 5       /* memory tuple order: spkemb, alsn, tlsn, apb, lsnemb (denoiser.py:220) */

typedef struct cfd_handle_s* cfd_handle;

/* Replaces Denoiser.__init__ (convofusion/models/architectures/denoiser.py:18-171) for the shipped
 * configuration (configs/modules/denoiser.yaml): condition text+audio, arch trans_dec, pre-norm, gelu,
 * sine PEs.  Dimensions other than the ones below are rejected with CFD_E_ARG. */
typedef struct {
  int latent_dim;        /* 128  (latent_dim[-1]) */
  int text_encoded_dim;  /* 512 */
  int ff_size;           /* 1024 */
  int num_layers;        /* 9 (1..16 accepted) */
  int num_heads;         /* 4 */
  int device;            /* HIP device ordinal */
} cfd_config;

int cfd_create(const cfd_config* cfg, cfd_handle* out);
void cfd_destroy(cfd_handle h);
const char* cfd_last_error(void);
/* Hash of the sources this library was built from (convofusion_amd/build.py: source_hash).  The ctypes binding compares
 * it with the sources on disk before the first call: a library left over from other sources -- e.g. after an update that
 * changed a struct of this header -- is rebuilt or refused instead of mis-reading its arguments. */
const char* cfd_source_hash(void);

/* Replaces nn.Module.load_state_dict for the `denoiser.*` entries of the checkpoint
 * (layout: SURVEY.md section 8b; test.py:109-111 -> base.py:106-123).  `name` is the key without the
 * `denoiser.` prefix, e.g. "decoder.layers.0.self_attn.in_proj_weight"; `data` is float32, `numel`
 * elements, on the host (is_device = 0) or the device (1).  Buffers `query_pos.pe` / `mem_pos.pe`
 * may be longer than the checkpoint's 1024 rows (closed-form sine table extended by the caller). */
int cfd_load_tensor(cfd_handle h, const char* name, const float* data, size_t numel, int is_device);

/* After the last cfd_load_tensor: checks that every tensor is present, folds and re-lays-out the
 * weights on the device (float64 folding, then split-pair GEMM operands: two fp16 halves hi + lo per value). */
int cfd_finalize_weights(cfd_handle h);

/* Sinusoid rows of the timestep embedding for integer timesteps 0..n_rows-1
 * (get_timestep_embedding, convofusion/models/architectures/tools/embeddings.py:245-285, computed by
 * the caller exactly as the reference does: [cos | sin] halves, 512 floats per row), host float32. */
int cfd_set_timestep_table(cfd_handle h, const float* rows, int n_rows);

/* One memory of the conditioning tuple.  `data` [U][S][512] float32 (dev) holds the U DISTINCT
 * memories; `row_map` (dev int32 [Be], or NULL meaning U == Be, identity) says which one each
 * effective-batch row uses -- the 7-way guidance batch repeats each utterance's memory and one shared
 * unconditional memory (convofusion.py:909-929), which the memory-side projections exploit.
 * `key_padding_mask` [U][S] uint8 (dev, 1 = ignore key; nn.MultiheadAttention key_padding_mask,
 * cross_attention.py:587-626) or NULL. */
typedef struct {
  const float* data;
  const int32_t* row_map;
  const uint8_t* key_padding_mask;
  int U;
  int S;
} cfd_memory;

/* Replaces Denoiser.forward (denoiser.py:173-386).
 *   sample      dev [Be][L][128]
 *   timesteps   HOST int32, n_t == 1 (one timestep for every row, the sampler's case) or n_t == Be
 *   mem[5]      conditioning tuple
 *   out         dev [Be][L][128]   predicted noise
 *   att[5]      dev [Be][num_layers][L][S_j] attention probabilities (cross_attention.py:227-234), or
 *               NULL pointers to skip materialising them
 * Enqueued on `stream` (a hipStream_t, may be NULL = default stream); no host sync inside. */
int cfd_forward(cfd_handle h, const float* sample, int Be, int L, const int32_t* timesteps, int n_t,
                const cfd_memory mem[CFD_NUM_MEM], float* out, float* const att[CFD_NUM_MEM], void* stream);

/* The caller's promise for the NEXT cfd_forward on this handle: its memories (data, key-padding masks, row maps, shapes) are bit-identical
 * to those of the previous cfd_forward.  That call then reuses their timestep-independent projections (the folded keys / values of all
 * layers: most of a call's work when the reference's own Python loop calls the denoiser once per iteration with an un-de-duplicated 7 x B
 * conditioning batch, convofusion.py:499-513).  Ignored -- the projections are made -- whenever the handle cannot honour it: anything else
 * ran on the handle in between (a sampling run, a WEG evaluation, a forward with per-row timesteps), other shapes, weights reloaded. */
int cfd_forward_same_memories(cfd_handle h);

/* Replaces Convofusion._diffusion_reverse (convofusion/models/modeltype/convofusion.py:391-549) and
 * its in-painting copy diffusion_reverse_forecast (unbounded_synthesis.py:28-187), together with the
 * diffusers-0.14.0 scheduler calls inside them (set_timesteps / step / add_noise). */
typedef struct {
  int B;                      /* utterances */
  int L;                      /* latent tokens (16 in the product; must be even) */
  int G;                      /* guidance chunks: 7 (clf_guidance_drops + 1, convofusion.py:60) or 1 */
  float guidance_weight[8];   /* weight of chunk k >= 1 in  e_0 + sum_k w_k (e_k - e_0)
                                 reference: {-, 7.5, 7.5, 7.5, 7.5, 7.5, 0}  (convofusion.py:529-541) */
  int scheduler;              /* 0 = DDPMScheduler (fixed_small), 1 = DDIMScheduler, 2 = DPMSolverMultistepScheduler in diffusers 0.14.0's
                                 default configuration (dpmsolver++, solver_order 2, midpoint, lower_order_final; no noise): needs
                                 `timesteps` and clip_sample == 0; eta, set_alpha_to_one and steps_offset are ignored.  The run keeps
                                 its own x0 history ([B][L][128] float32, allocated by cfd_sample_begin).
                                 3 = deterministic DDIM inversion (prompt-to-prompt's next_step): runs the DDIM step backwards, from
                                 clean latents towards noise.  Needs `timesteps`, strictly increasing in [0, T) (the DDIM table
                                 reversed), eta == 0 and clip_sample == 0 (a clipped x0 is not invertible).  Iteration i at t:
                                 eps = the combine evaluated at t; a_cur = abar[t - T // N] (t - T // N < 0: 1 with set_alpha_to_one,
                                 else abar[0]), a_nxt = abar[t]; x0 = (x - sqrt(1 - a_cur) eps) / sqrt(a_cur),
                                 x = sqrt(a_nxt) x0 + sqrt(1 - a_nxt) eps -- kind 1's step with these coefficients.  CFD_E_ARG with
                                 preseq, a dynamic memory, an edit (cfd_sample_begin_edit / _anchored) or a WEG update
                                 (cfd_sample_write). */
  int num_train_timesteps;    /* 1000 */
  int num_inference_steps;    /* scheduler.set_timesteps(N) */
  int clip_sample;            /* configs/modules/scheduler.yaml:11 */
  float eta;                  /* DDIM only */
  int set_alpha_to_one;       /* DDIM only */
  int steps_offset;           /* DDIM only */
  const float* alphas_cumprod;/* HOST float32 [num_train_timesteps] (the scheduler's table) */
  const float* init_latents;  /* dev [B][L][128] N(0,1) draws (scaled by init_noise_sigma = 1), or NULL:
                                 drawn on the device, Philox stream 1 */
  const float* step_noise;    /* dev [iterations][B][L][128] or NULL: Philox stream 0 */
  uint64_t seed;              /* Philox key */
  uint32_t first_utterance;   /* global id of utterance 0 (shards draw independent sub-streams) */
  const float* preseq;        /* dev [B][preseq_len][128] previous-window latents to in-paint, or NULL */
  int preseq_len;
  cfd_memory mem[CFD_NUM_MEM];/* Be = G*B rows */
  int skip_zero_weight_chunks;/* != 0: trailing guidance chunks whose weight is exactly 0 are not evaluated.  The
                                 reference computes the full-conditioning chunk and multiplies it by
                                 guidance_scale * 0 (convofusion.py:538); its forward only feeds the per-step
                                 attention maps, which the fused loop does not keep.  Results are identical. */
  int dynamic_memory_mask;    /* bit j set: the CONTENTS of memory j may be rewritten by the caller between iterations of the
                                 run (the dyadic rollout's partner projection); its projections are then made in every
                                 iteration.  0 (the reference loop: memories are constants of a run, convofusion.py:391-549):
                                 the timestep-independent part of every memory's projections is computed once at
                                 cfd_sample_begin and the memories are not read again. */
  const int32_t* timesteps;   /* HOST int32 [num_timesteps]: the loop's timestep sequence `scheduler.timesteps` (convofusion.py:423),
                                 or NULL: (arange(N) * (T // N))[::-1] (+ steps_offset for DDIM), N = num_inference_steps.  The step
                                 formulas keep `prev_t = t - T // N` either way.  Needed for DDPM counts that do not divide T, where
                                 diffusers 0.14.0's table arange(0, T, T // N)[::-1] has MORE than N entries (unpinned, see
                                 convofusion_amd/scheduler.py); the run then has num_timesteps iterations.
                                 Scheduler 2 (DPM-Solver++) REQUIRES the table -- np.linspace(0, T - 1, N + 1).round()[::-1][:-1], built by
                                 the scheduler (numpy rounds halves to even; the library never rebuilds it) -- strictly decreasing and in
                                 [1, T); each step goes to the next entry (to 0 after the last), and its second-order term uses the
                                 previous entry. */
  int num_timesteps;
  int prediction_type;        /* what the denoiser predicts (the schedulers' prediction_type; TRAIN.ABLATION.PREDICT_EPSILON of the
                                 reference, convofusion.py:101-103): 0 = the noise ("epsilon"; ctypes' zero-initialised default), 1 = the
                                 clean latent ("sample").  With 1 the guidance combine `out` is read as x0 (clipped to [-1, 1] with
                                 clip_sample): scheduler 0 steps ddpm_mu(x0, x) + sigma z, scheduler 2 takes it as its data prediction,
                                 scheduler 1 steps c0 x0 + cx eps_hat (+ sigma z) with eps_hat = (x - sqrt(abar_t) out) / sqrt(1 - abar_t)
                                 from the UNCLIPPED output (the form of later diffusers releases; 0.14.0's DDIM is unpinned here).  Any
                                 other value is CFD_E_ARG.  1 is refused (CFD_E_ARG) by scheduler 3, cfd_sample_begin_anchored,
                                 cfd_sample_begin_replay, cfd_ddpm_invert and cfd_sample_parallel.  The field sits in what was 4 bytes of
                                 padding in front of att_ring: no other field moves and the struct's size is unchanged. */
  float* att_ring[CFD_NUM_MEM];/* all NULL, or five dev buffers [iterations][B][num_layers][L][S_j] float32: the captured iteration
                                 stores the attention probabilities of the LAST guidance chunk (full conditioning) of iteration i into
                                 slot i -- the reference's per-iteration dict attention_matrices[t] = att_mats of the last chunk
                                 (convofusion.py:517-523, dumped as att_<t>.npy by base.py:243-259).  Small problems (the row-tile
                                 path) store them from their second cross-attention launch, all others from the fused
                                 cross-attention kernel's softmax (+ one small launch per iteration): 2 - 5 % of the run time.
                                 Needs skip_zero_weight_chunks == 0 and no dynamic memory (such a run has no fused cross-attention:
                                 cfd_sample_begin fails with CFD_E_SHAPE and the caller takes the maps with one cfd_forward per
                                 iteration).  The ring's size is the caller's business: iterations x B x layers x L x keys. */
  int operand_policy;         /* Operand format of the fused cross-attention's key / value tiles of the LONG memories (>= 128 padded keys: the
                                 audio memory) in THIS run (csrc/xattn_fused.hpp, F16):
                                 0 = fp16 split pairs everywhere (3 MFMAs per product, ~2^-22 operand error: what cfd_forward always uses);
                                 non-zero in bits 0 - 3 (15 by convention) = plain fp16 attention against the long memories: their folded
                                 keys and values as single-fp16 tiles (half those tiles' L2 -> LDS traffic), the queries and probabilities
                                 of those products as one fp16 as well (1 MFMA per product instead of 3).  Partial combinations were
                                 measured and are dominated.
                                 Short memories (the text / speaker / activity memories: few keys, little averaging of the rounding) always
                                 keep pairs.  The reference is float32 throughout (cross_attention.py:593-652); which runs tolerate the format
                                 is measured per scheduler in DESIGN.md section 2 -- convofusion_amd.sampler.OPERAND_POLICY holds the default
                                 per scheduler kind.  Ignored (pairs) on the row-tile path, with att_ring, and with a dynamic memory. */
  float census_tau;           /* > 0: the run keeps an attention-concentration census of its long memories (cfd_sample_census): the fused
                                 cross-attention kernel counts, per layer, the largest probability of every query row against a long memory
                                 (>= 128 padded keys) and how many rows have one above census_tau.  0 (ctypes' zero-initialised default): off,
                                 nothing is counted.  The field sits in what was the tail padding of this struct: its size is unchanged. */
} cfd_sample_args;

/* Opens a sampling run: builds the per-step coefficient and timestep-embedding tables, draws / copies
 * the initial latents and captures ONE loop iteration (replicate -> denoiser -> guidance -> scheduler
 * step) as a hipGraph on `stream`. */
int cfd_sample_begin(cfd_handle h, const cfd_sample_args* args, void* stream);
/* cfd_sample_begin with per-modality guidance weights that may change over the schedule and differ per utterance (the reference's
 * w_c, convofusion.py:527-541, "kept 1 as a standard").  `weights`: HOST float32 [iterations][B][8], copied once; entry [i][b][k] is the
 * whole factor of chunk k >= 1 for utterance b in iteration i -- guidance_scale * w_c as the reference would compute it -- and [i][b][0]
 * is ignored.  The combine is the default run's term for term: e_0 + ((((w_1 (e_1 - e_0) + w_2 (e_2 - e_0)) + ...) + w_6 (e_6 - e_0)).
 * args->guidance_weight and args->skip_zero_weight_chunks are ignored; args->G must be 7.  A NULL table or a non-finite entry:
 * CFD_E_ARG.  prune != 0: every chunk k >= 1 whose weight is exactly 0 in all iterations and for all utterances is not evaluated (its
 * term is a zero that leaves the float32 sum unchanged): the memories' row maps are compacted to the evaluated chunks in stream order
 * (a memory without a row map gets the identity map), so the denoiser runs G_eval * B rows; the full-conditioning chunk is kept when the
 * run has att_ring (its maps come from it).  *chunks_evaluated (may be NULL) receives G_eval. */
int cfd_sample_begin_weighted(cfd_handle h, const cfd_sample_args* args, const float* weights, int prune, int* chunks_evaluated,
                              void* stream);
/* Motion editing (token-masked in-painting, img2img strength).  The 16 loop tokens are 8 time chunks x {body, hands}: token 2c + p is
 * 16-frame chunk c, part p (convofusion.py:1028), so one [B][L] mask selects time spans, body parts or both. */
typedef struct {
  const float* source;        /* dev [B][L][128] float32: the latents to edit (e.g. the VAE encoder's posterior mean in loop layout).
                                 Copied at begin: the run does not read it afterwards.  NULL: CFD_E_ARG. */
  const uint8_t* keep;        /* dev [B][L] uint8, each 0 or 1 (another value: CFD_E_ARG), or NULL (= all 0).  At the start of every
                                 executed iteration i the tokens with keep = 1 are set to sa_i * source + sb_i * eps -- the reference
                                 rollout's add_noise (unbounded_synthesis.py:70-76) with the mask in place of `l < preseq_len`; sa_i /
                                 sb_i = sqrt(abar_t), sqrt(1 - abar_t) of iteration i's timestep; each product and the sum rounded to
                                 float32 on its own.  eps = the run's initial N(0,1) draw (init_latents, or Philox stream 1), kept for the
                                 whole run and never rewritten.  cfd_sample_inpaint does this overwrite ahead of the captured iteration. */
  int first_iteration;        /* k0 in [0, iterations): the run executes iterations k0 .. iterations - 1 of the full timestep table
                                 (img2img strength: k0 = iterations - min(int(iterations * strength), iterations)).  k0 > 0: every token
                                 starts at sa_k0 * source + sb_k0 * eps; k0 = 0: the initial latents are eps unchanged.  Iteration i keeps
                                 its full-table index everywhere: step coefficients, Philox step-noise index i, step_noise row i,
                                 the weight table's row i.  DPM-Solver++: the first executed step is first order (no history yet) and
                                 lower_order_final follows the full table's length, as diffusers 0.14.0 decides them.
                                 cfd_sample_position and cfd_sample_steps count executed iterations (iterations - k0 in all); att_ring
                                 slot j holds executed iteration k0 + j, so the ring needs iterations - k0 slots. */
} cfd_edit_args;
/* cfd_sample_begin / cfd_sample_begin_weighted (weights != NULL, with `prune` and `chunks_evaluated` as there; weights == NULL: the
 * default combine with args->guidance_weight, `prune` ignored and *chunks_evaluated = the evaluated chunks) for an edit run.  CFD_E_ARG:
 * e == NULL, e->source == NULL, e->first_iteration outside [0, iterations), a keep value other than 0 / 1, args->preseq together with
 * an edit.  With first_iteration = 0 and keep all 0 / NULL the run computes what cfd_sample_begin(_weighted) computes, bit for bit. */
int cfd_sample_begin_edit(cfd_handle h, const cfd_sample_args* args, const cfd_edit_args* e, const float* weights, int prune,
                          int* chunks_evaluated, void* stream);
/* Tied tokens: a token of the run that takes its value from another token of the same run in every iteration.  Long-form synthesis runs
 * the half-overlapping 128-frame windows of an utterance as rows of one batch at the same noise level and ties the first half of window w
 * to the second half of window w - 1 (the synchronous form of the reference rollout's preseq in-painting). */
typedef struct {
  const int32_t* tie;         /* dev [B][L] int32: -1 (a free token) or the flat index b' * L + l' of the token's source in the same run.
                                 At the start of every iteration, before the replication into the denoiser's input,
                                 latents[b][l] = latents[b'][l'] -- the source as the previous iteration's scheduler step left it (at
                                 iteration 0: its initial noise) -- and once more after the last iteration, so that cfd_sample_read of a
                                 finished run returns every tied token bit-identical to its source; a read before that returns the
                                 latents as the scheduler step left them.  cfd_sample_inpaint does the copy (and an edit's overwrite)
                                 ahead of the captured iteration.  A source must be free: not tied itself (no chains, no cycles, no
                                 self-tie) and not kept by the edit, so no launch reads a token it writes.  Copied at begin (and checked
                                 on the host copy): the run does not read the caller's table afterwards. */
} cfd_tie_args;
/* cfd_sample_begin_edit (edit != NULL: its kept tokens next to the tied ones; first_iteration must be 0) or cfd_sample_begin /
 * cfd_sample_begin_weighted (edit == NULL: no kept token, no source needed) for a tied run; weights / prune / chunks_evaluated as in
 * cfd_sample_begin_edit.  Schedulers 0, 1 and 2, with or without att_ring, either operand policy.  With a table of -1 throughout the run
 * computes what the same call without ties computes, bit for bit.  CFD_E_ARG, with the first offending (b, l) in cfd_last_error: an entry
 * outside [-1, B * L), a token tied to itself, a source that is itself tied, a source that is kept, a token both kept and tied; also a NULL
 * tie or table, a NULL edit source, first_iteration != 0 (no strength), scheduler 3 (DDIM inversion), preseq, dynamic memories (dyadic
 * runs; cfd_dyadic_steps refuses a tied run as well).  An anchored run has no tied form. */
int cfd_sample_begin_tied(cfd_handle h, const cfd_sample_args* args, const cfd_edit_args* edit, const cfd_tie_args* tie,
                          const float* weights, int prune, int* chunks_evaluated, void* stream);
/* DDIM inversion with its trajectory: cfd_sample_begin / cfd_sample_begin_weighted (weights != NULL, with `prune` and `chunks_evaluated`
 * as there; weights == NULL: the default combine, *chunks_evaluated = the evaluated chunks) for a scheduler-3 run that also records
 * `trajectory`: dev float32 [iterations + 1][B][L][128], owned by the caller and written by the run.  Slot 0 receives the initial
 * latents (the source) at begin; the captured iteration's scheduler step stores the latents after iteration i into slot i + 1 (no extra
 * launch).  CFD_E_ARG: trajectory == NULL, args->scheduler != 3, and every kind-3 refusal. */
int cfd_sample_begin_invert(cfd_handle h, const cfd_sample_args* args, float* trajectory, const float* weights, int prune,
                            int* chunks_evaluated, void* stream);
/* Re-conditioning over a recorded inversion trajectory (cfd_sample_begin_invert). */
typedef struct {
  const float* trajectory;    /* dev float32 [steps + 1][B][L][128]: the ring of an inversion run.  Read, not copied: it must stay
                                 unchanged until the run is closed. */
  int steps;                  /* iterations of that inversion; must equal this run's iterations */
  int B, L;                   /* the ring's utterances and tokens; must equal args->B / args->L */
  const uint8_t* keep;        /* dev [B][L] uint8, each 0 or 1, or NULL (= all 0): at the start of iteration i the tokens with keep = 1
                                 are set to trajectory[steps - i] -- the inverted latents at the level iteration i starts from. */
} cfd_anchor_args;
/* An anchored DDIM run: args->scheduler == 1, eta == 0, clip_sample == 0, no preseq.  Weights / prune / chunks_evaluated as in
 * cfd_sample_begin_edit.  With keep all 0 / NULL the run computes what cfd_sample_begin(_weighted) computes, bit for bit.  CFD_E_ARG:
 * a NULL argument or trajectory, another scheduler, eta != 0, clip_sample != 0, preseq, steps / B / L other than the run's, a keep
 * value other than 0 / 1. */
int cfd_sample_begin_anchored(cfd_handle h, const cfd_sample_args* args, const cfd_anchor_args* a, const float* weights, int prune,
                              int* chunks_evaluated, void* stream);
/* Edit-friendly DDPM inversion (Huberman-Spiegelglas et al., CVPR 2024): the noise space of a DDPM run that reproduces `source`.  For
 * every iteration i of the DDPM table (timestep t_i, N entries) an INDEPENDENT level x_i = fl(fl(sa_i * source) + fl(sb_i * eps_i)) is
 * drawn, the guided prediction is evaluated at every level under the run's conditioning, and the DDPM step is solved for its noise:
 *   z_i = (x_{i+1} - mu_i(x_i, eps_hat_i)) / sigma_i        (x_N = source; z_i = 0 exactly where the step adds none: t_i = 0)
 * with mu_i = c0 * x0 + cx * x_i, x0 = clip((x_i - sb * eps_hat) / sa), evaluated as the DDPM loop's step evaluates them.  The N
 * evaluations do not depend on each other: they run as ceil(N / J) denoiser forwards of J levels each (J * G_eval * B * L token rows with
 * per-level timesteps), enqueued on `stream` with no host synchronisation between them; the memory-side work of a forward is done once
 * per (level, distinct memory instance) -- the rows of a level reach their instance through the run's row maps. */
typedef struct {
  const float* source;        /* dev [B][L][128] float32 */
  const float* weights;       /* HOST float32 [N][B][8] or NULL, with `prune`: as in cfd_sample_begin_weighted (NULL: args->guidance_weight
                                 and args->skip_zero_weight_chunks) */
  int prune;
  const float* level_noise;   /* dev [N][B][L][128] eps_i, or NULL: Philox stream 2, step index i, utterance first_utterance + b (a draw
                                 per level, independent of the others and of streams 0 / 1) */
  float* trajectory;          /* out, dev [N + 1][B][L][128]: slot 0 the source, slot N - i the level x_i ENTERING iteration i (slot N the
                                 noisiest) -- the convention of cfd_sample_begin_invert's ring */
  float* noise;               /* out, dev [N][B][L][128]: row i = z_i, the step noise of iteration i */
  int levels_per_batch;       /* J; 0: chosen from workspace_bytes */
  size_t workspace_bytes;     /* budget of the level batch's workspace (0: 4 GiB); J is the largest count the library's estimate of a level's
                                 workspace fits into it, at least 1 */
} cfd_ddpm_invert_args;
/* `args`: the cfd_sample_args of the DDPM run (scheduler 0, its timestep table, memories with row maps, clip_sample honoured;
 * init_latents / step_noise / att_ring unused).  *chunks_evaluated / *levels_per_batch_used (may be NULL) receive G_eval and J.
 * CFD_E_ARG: a scheduler other than 0, preseq, a dynamic memory, att_ring, a NULL source / trajectory / noise, a weight table with a
 * non-finite entry.  CFD_E_STATE: a sampling run is open on the handle. */
int cfd_ddpm_invert(cfd_handle h, const cfd_sample_args* args, const cfd_ddpm_invert_args* inv, int* chunks_evaluated,
                    int* levels_per_batch_used, void* stream);
/* Parallel-in-time DDPM sampling (ParaDiGMS, Shih et al., NeurIPS 2023): Picard sweeps over a sliding window of J consecutive latents of
 * the DDPM chain.  X(i) is the current estimate of the latent ENTERING iteration i; the window is iterations i0 .. i0 + p - 1,
 * p = min(J, N - i0); X(i0) is final.  One sweep evaluates the guided prediction at every X(j) of the window in ONE level-batched forward
 * (the batch of cfd_ddpm_invert), takes the DDPM step s_j = mu_j(X(j), eps_hat_j) [+ sigma_j z_j] of every level, and re-propagates
 *   Xn(i0) = X(i0),   Xn(j + 1) = fl(s_j + fl(Xn(j) - X(j)))
 * serially per element.  A level whose predecessor did not change receives exactly s_j, and X(i0 + 1) is exact after every sweep: at
 * tolerance 0 the call computes the sequential chain, in at most N sweeps.  After a sweep the host reads, per window position
 * k = 1 .. p - 1 and utterance b, e[k][b] = sum_{l,d} (Xn(i0 + k) - X(i0 + k))^2 (reduced in a fixed order, no float atomics: two calls
 * on the same inputs take the same strides and return the same bits) and slides the window by the largest stride s in [1, p] with
 *   e[k][b] / (L * 128) <= tolerance^2 * v(i0 + k)   for every 1 <= k < s and every b
 * where v(i) = sigma_i^2 of iteration i's step (an iteration that adds no noise takes the value of the iteration before it).  The
 * levels that enter the window start from the last window value.  One host synchronisation per sweep. */
typedef struct {
  const float* weights;       /* HOST float32 [N][B][8] or NULL, with `prune`: as in cfd_ddpm_invert_args */
  int prune;
  float tolerance;            /* tau >= 0 (0: the sequential chain) */
  int levels_per_batch;       /* J; 0: chosen from workspace_bytes as cfd_ddpm_invert chooses it */
  size_t workspace_bytes;     /* as in cfd_ddpm_invert_args (0: 4 GiB) */
  int max_sweeps;             /* 0: N (always enough); a run that needs more fails with CFD_E_STATE */
  float* latents;             /* out, dev [B][L][128] */
  float* trajectory;          /* out or NULL, dev [N + 1][B][L][128]: slot N - i the latent entering iteration i, slot 0 the result (the
                                 ring convention of cfd_sample_begin_invert / cfd_ddpm_invert).  The call works in place in it; a slot is
                                 never written again once its latent is final.  NULL: the call keeps J + 1 slots of its own. */
} cfd_parallel_args;
typedef struct {
  int levels_per_batch;       /* J as used */
  int chunks_evaluated;       /* G_eval */
  int sweeps;                 /* level-batched forwards executed */
  int* strides;               /* HOST int32 [strides_capacity] or NULL: the advance of sweep k (they sum to N); sweeps beyond the
                                 capacity are not recorded */
  int strides_capacity;
} cfd_parallel_stats;
/* `args`: the cfd_sample_args of the DDPM run (scheduler 0; clip_sample, timesteps, the memories with their row maps, guidance_weight /
 * skip_zero_weight_chunks, seed and first_utterance honoured; init_latents / step_noise as in cfd_sample_begin -- NULL: Philox stream 1
 * and stream 0 with step index i, the draws of the captured loop with the same seed).  `stats` may be NULL; its `strides` / capacity are
 * inputs.  A self-contained call: it opens no run.  Operands are split pairs.  CFD_E_ARG: a scheduler other than 0, preseq, a dynamic
 * memory, att_ring, a negative or non-finite tolerance, a negative levels_per_batch or max_sweeps, a NULL `latents`.  CFD_E_STATE: a
 * sampling run is open on the handle; max_sweeps reached before the last level was final. */
int cfd_sample_parallel(cfd_handle h, const cfd_sample_args* args, const cfd_parallel_args* par, cfd_parallel_stats* stats, void* stream);
/* Replay of a recorded noise space (cfd_ddpm_invert). */
typedef struct {
  const float* trajectory;    /* dev [steps + 1][B][L][128]; read in place until the run is closed */
  const float* noise;         /* dev [steps][B][L][128]; read in place: iteration i takes noise[i] as its step noise */
  int steps;                  /* iterations of the inversion; must equal this run's iterations */
  int B;                      /* must equal args->B */
  int L;                      /* must equal args->L */
  const uint8_t* keep;        /* dev [B][L] uint8 0 / 1 or NULL (= all 0): at the start of iteration i the tokens with keep = 1 are set
                                 to trajectory[steps - i] */
  int first_iteration;        /* k0 in [0, steps): the paper's T_skip.  The run starts from trajectory[steps - k0] and executes iterations
                                 k0 .. steps - 1; counting (cfd_sample_position, weight-table row, att_ring slot) as in cfd_edit_args */
} cfd_replay_args;
/* A DDPM run (args->scheduler == 0) over a recorded noise space; args->init_latents / step_noise are ignored (they come from the rings).
 * Weights / prune / chunks_evaluated as in cfd_sample_begin_edit.  With keep all 0 / NULL and first_iteration = 0 the run computes what
 * cfd_sample_begin(_weighted) with init_latents = trajectory[steps] and step_noise = noise computes, bit for bit.  CFD_E_ARG: a NULL
 * argument, trajectory or noise, another scheduler, steps / B / L other than the run's, first_iteration outside [0, steps), preseq, a
 * dynamic memory, a keep value other than 0 / 1.  A replay has no tied form, and cfd_sample_write (a WEG update) refuses it. */
int cfd_sample_begin_replay(cfd_handle h, const cfd_sample_args* args, const cfd_replay_args* r, const float* weights, int prune,
                            int* chunks_evaluated, void* stream);
/* Replays the captured iteration `n` more times (asynchronously on the run's stream). */
int cfd_sample_steps(cfd_handle h, int n);
/* Number of iterations executed so far in the open run. */
int cfd_sample_position(cfd_handle h);

/* Dyadic reactive path (BASELINE.json configs[4]; the partner projection is the reference's TextAudioMotionFuser.latent_proj,
 * condfuser.py:22-27: Linear 128->128, GELU, Linear 128->out_dim, GELU): `n` lock-step iterations of two open sampling runs.
 * Each iteration enqueues, on ONE stream (side A's) and with no host synchronisation, the projection of side B's current latents
 * into side A's conditional speaker-memory rows `spk_a` [B][L][512], the projection of side A's latents into `spk_b`, side A's
 * captured iteration and side B's captured iteration.  Both runs must have been opened with the speaker memory declared dynamic
 * (cfd_sample_args.dynamic_memory_mask bit 0) and `spk_*` pointing into the memories they captured.  All pointers are device
 * pointers; `tmp` holds B * L * hidden floats.
 * Merged form (side_b == NULL), for two sides that share the denoiser's weights: ONE run of 2 B utterances -- side A's followed by
 * side B's -- whose conditional speaker rows [0, B) are `spk_a` and [B, 2 B) are `spk_b`; an iteration is the two projections and one
 * captured iteration of the double batch. */
typedef struct {
  const float* w1;  /* [hidden][latent_dim] */
  const float* b1;  /* [hidden] */
  const float* w2;  /* [out_dim][hidden] */
  const float* b2;  /* [out_dim] */
  int hidden, out_dim;
  float* spk_a;
  float* spk_b;
  float* tmp;
} cfd_dyadic_proj;
int cfd_dyadic_steps(cfd_handle side_a, cfd_handle side_b, const cfd_dyadic_proj* proj, int n);
/* Copies the current latents to `out` (dev [B][L][128]); with close != 0 also ends the run. */
int cfd_sample_read(cfd_handle h, float* out, int close);

/* Attention-concentration census of the last sampling run opened on the handle (open or closed), over its iterations so far.  Each
 * (query row, long memory) pair the fused cross-attention kernel evaluates contributes the row's largest probability max_s p_s.
 * Layer 0 evaluates the long memory once per distinct (utterance, memory instance) pair and counts those rows once.  Waits for the run's
 * stream.  measured = 0: nothing of the run could count -- census_tau was 0, or the run has no fused non-ATT cross-attention launch (the
 * row-tile path, the three-launch path, a dynamic memory, att_ring); such runs use split pairs whatever the operand policy. */
#define CFD_CENSUS_MAX_LAYERS 16
typedef struct {
  float tau;                                  /* cfd_sample_args.census_tau of the run */
  int measured;
  int iterations;                             /* iterations the census covers */
  int worst_layer;                            /* layer with the largest peak (-1: none counted) */
  float peak_max;                             /* largest peak probability over layers, rows and iterations (0: none counted) */
  uint32_t rows_over;                         /* (row, long memory) pairs with a peak > tau, all layers and iterations */
  uint32_t rows_seen;                         /* live (row, long memory) pairs counted */
  float layer_peak[CFD_CENSUS_MAX_LAYERS];    /* per layer (layers beyond num_layers: 0) */
  uint32_t layer_over[CFD_CENSUS_MAX_LAYERS];
} cfd_census;
int cfd_sample_census(cfd_handle h, cfd_census* out);

/* Stand-alone scheduler ops on device tensors (diffusers 0.14.0 `scheduler.step(...).prev_sample` and
 * `add_noise`), for callers that drive their own loop (unbounded_synthesis.py:75,181).  cfd_scheduler_step takes scheduler 0 (DDPM),
 * 1 (DDIM) or 3 (DDIM inversion: `t` is the level the step moves to; eta and clip_sample must be 0) and refuses any other kind with
 * CFD_E_ARG: DPM-Solver++ keeps a history and has its own entry, cfd_dpmsolver_step. */
int cfd_scheduler_step(cfd_handle h, int scheduler, const float* alphas_cumprod, int num_train_timesteps,
                       int num_inference_steps, int t, int clip_sample, float eta, int set_alpha_to_one,
                       const float* model_output, const float* noise, float* sample_inout, size_t numel,
                       float* pred_original_sample /* dev [numel] or NULL: the (clipped) x0 estimate the step forms,
                       SchedulerOutput.pred_original_sample (read at convofusion.py:619) */,
                       void* stream);
/* Stand-alone DPM-Solver++ (2M) step (diffusers 0.14.0 DPMSolverMultistepScheduler.step, default configuration) on device tensors, for
 * callers that drive their own loop; the caller keeps the history.  x0_out (dev [numel]) receives this step's data prediction
 * x0 = (x - sigma_t eps) / alpha_t -- the m_prev of the next step -- and sample_inout the update from t to prev_t (0 after the last
 * table entry).  t_prev_model: the timestep of the previous step (whose x0 is m_prev) for a second-order step, -1 for a first-order
 * step (m_prev may then be NULL).  alphas_cumprod is HOST float32 [num_train_timesteps].  Shares its coefficients with the
 * sampling loop's scheduler kind 2. */
int cfd_dpmsolver_step(cfd_handle h, const float* alphas_cumprod, int num_train_timesteps, int t, int prev_t, int t_prev_model,
                       const float* model_output, const float* m_prev, float* sample_inout, float* x0_out, size_t numel, void* stream);
/* cfd_scheduler_step / cfd_dpmsolver_step with the model's prediction type (cfd_sample_args.prediction_type: 0 = epsilon, what the two
 * calls above pass; 1 = sample: model_output is x0 -- pred_original_sample / x0_out is then the (clipped) model output; any other value
 * and 1 with scheduler 3 are CFD_E_ARG). */
int cfd_scheduler_step_pred(cfd_handle h, int scheduler, const float* alphas_cumprod, int num_train_timesteps, int num_inference_steps,
                            int t, int clip_sample, float eta, int set_alpha_to_one, int prediction_type, const float* model_output,
                            const float* noise, float* sample_inout, size_t numel, float* pred_original_sample, void* stream);
int cfd_dpmsolver_step_pred(cfd_handle h, const float* alphas_cumprod, int num_train_timesteps, int t, int prev_t, int t_prev_model,
                            int prediction_type, const float* model_output, const float* m_prev, float* sample_inout, float* x0_out,
                            size_t numel, void* stream);
int cfd_add_noise(cfd_handle h, const float* alphas_cumprod_host, int t, const float* original,
                  const float* noise, float* out, size_t numel, void* stream);

/* Conditioning producers on device tensors: out[r][n] = act(b[n] + sum_k x[r][k] W[n][k]), float32 -- one
 * nn.Linear (+ activation) of the small MLPs that make the memories: AudioConvEncoder.main / .out_net
 * (convofusion/models/architectures/audioenc.py:12-21,33-34: Linear, LeakyReLU(0.1), Linear, LeakyReLU(0.1), Linear;
 * dropout is the identity at inference) and TextAudioMotionFuser.latent_proj (condfuser.py:22-27: Linear, GELU,
 * Linear, GELU), which the dyadic path applies to the partner's current latents every step (BASELINE config 5).
 *   x dev [n_rows][K], W dev [N][K] (nn.Linear.weight), b dev [N] or NULL, out dev [n_rows][N]
 *   act: 0 none, 1 nn.GELU() (erf form), 2 nn.LeakyReLU(0.1) */
int cfd_linear_act(cfd_handle h, const float* x, long long n_rows, int K, const float* W, const float* b, int N, int act,
                   float* out, void* stream);

/* float32 building blocks of the small transformer that follows the loop -- ConvoFusionVae.decode
 * (convofusion/models/architectures/vae.py:268-372: two SkipTransformerDecoders of d_model 128, 2 heads, 5 pre-norm layers,
 * cross_attention.py:66-125,311-395) -- used by convofusion_amd/vae.py together with cfd_linear_act:
 *   cfd_layer_norm  nn.LayerNorm over the last dimension (D <= 2048)
 *   cfd_mha         the attention core of nn.MultiheadAttention on already projected q / k / v, sequence-major
 *                   [L][bs][E] rows, key_padding_mask dev uint8 [bs][Lk] (1 = ignore) or NULL; head_dim <= 64, Lk <= 1024
 *   cfd_add         x += y (residual connection)
 *   cfd_zero_rows   rows with keep[row] == 0 are zeroed (vae.py:358 `output[~mask.T] = 0`) */
int cfd_layer_norm(cfd_handle h, const float* x, long long rows, int D, const float* gamma, const float* beta, float eps,
                   float* out, void* stream);
int cfd_mha(cfd_handle h, const float* q, const float* k, const float* v, int Lq, int Lk, int bs, int E, int H,
            const uint8_t* key_padding_mask, float* out, void* stream);
int cfd_add(cfd_handle h, float* x, const float* y, size_t numel, void* stream);
int cfd_zero_rows(cfd_handle h, float* x, const uint8_t* keep, long long rows, int D, void* stream);

/* Replaces ConvoFusionVae.encode (convofusion/models/architectures/vae.py:162-266: SkipTransformerEncoder cross_attention.py:18-64 of
 * pre-norm TransformerEncoderLayers :288-300) up to the distribution's parameters, in ONE launch for both encoder stacks
 * (csrc/vae_enc.hpp): the chunking into 16-frame sequences with frame 0's root x / z subtracted (:176-187), the skeleton embeddings,
 * the 2 global motion tokens + query_pos_encoder.pe, the key-padding mask of `lengths`, both SkipTransformerEncoders, the final norm,
 * and the first 2 tokens of each stack.  Exact float32 throughout.  std / the rsample stay with the caller (vae.py:256-258).
 *   wpack       dev float32: the packed encoder weights of both stacks, layout in csrc/vae_enc.hpp (built by convofusion_amd/vae.py)
 *   d_model, num_heads, ff_size, num_layers, latent_size: must be 128, 2, 1024, odd <= 9, 1 (CFD_E_ARG otherwise)
 *   features    dev float32 rows (b * nframes + f) of >= 189 values, row_stride floats apart (vae.py:164, [bs, nframes, 189])
 *   nframes     a positive multiple of 16 (CFD_E_SHAPE otherwise); every length must be <= nframes (the caller checks max == nframes)
 *   lengths     dev int32 [bs]: frame f of chunk c of sequence b is a valid key iff 16 c + f < lengths[b]
 *   mu_logvar   dev float32 [2 (mu, logvar)][2 (body, hands)][bs * nframes / 16][128]: mu = mu_logvar[0], logvar = mu_logvar[1]
 *   feats_out   dev float32 [bs * nframes][189]: the root-subtracted features (the third return value), bit-identical to the reference
 *   seqs_per_group  0 = automatic; 1 - 3 forces that many 18-token sequences per workgroup (measurement only) */
int cfd_vae_encode(cfd_handle h, const float* wpack, int d_model, int num_heads, int ff_size, int num_layers, int latent_size,
                   const float* features, int bs, int nframes, long long row_stride, const int* lengths, float* mu_logvar,
                   float* feats_out, int seqs_per_group, void* stream);

/* Replaces the reference's T5TextEncoder behind its tokenizer (convofusion/models/architectures/t5.py:9-109): the T5 v1.0 encoder
 * (transformers T5EncoderModel, feed_forward_proj "relu": RMS norms without mean or bias, attention without the 1/sqrt(d_kv) scale and
 * with block 0's relative-position bias in every block, ReLU feed-forward) followed by `Linear(relu(last_hidden_state))` (t5.py:48-49,
 * 57), in 5 launches per block + 1 (csrc/t5_enc.hpp).  Exact float32 on the float32 matrix instruction: no operand has a range limit,
 * no atomics, and a sequence's result is the same bits whatever else is in the batch and whatever it is padded to.
 *   wpack       dev float32: embed [vocab][768] | per block g1, Wq|Wk|Wv, Wo, g2, Wi, Wo_ff | g_final (csrc/t5_enc.hpp; built by
 *               convofusion_amd/text.py)
 *   d_model, d_kv, num_heads, d_ff, num_layers: must be 768, 64, 12, 3072, 1 - 12; gated_act must be 0 (CFD_E_ARG otherwise)
 *   n_seq, T    n_seq >= 1 sequences padded to 1 <= T <= 256 tokens (CFD_E_SHAPE otherwise)
 *   ids         dev int32 [n_seq][T], each in [0, vocab) (the caller checks; the kernels clamp a stray id into the table)
 *   mask        dev uint8 [n_seq][T], 1 = token: only KEYS are masked (probability exactly 0); padded queries are computed like any
 *               other, as the reference does.  Every sequence needs at least one token (a sequence without keys gives NaN rows).
 *   rel_bias    dev float32 [12][2 T - 1]: block 0's relative_attention_bias by relative distance, entry [h][j - i + T - 1] (the bucket
 *               function stays on the host: convofusion_amd/text.py)
 *   proj_w, proj_b, proj_dim   dev float32 [proj_dim][768], [proj_dim], proj_dim a multiple of 64; or proj_w NULL
 *   out         dev float32 [n_seq][T][proj_dim], or [n_seq][T][768] (the last hidden state) when proj_w is NULL
 * Everything is refused before the first launch.  The workspace (33 792 bytes per token row) lives on the handle and only grows. */
typedef struct {
  const float* wpack;
  int vocab;
  int d_model, d_kv, num_heads, d_ff, num_layers;
  int gated_act;
  float eps;
  int n_seq, T;
  const int32_t* ids;
  const uint8_t* mask;
  const float* rel_bias;
  const float* proj_w;
  const float* proj_b;
  int proj_dim;
} cfd_t5_args;
int cfd_t5_encode(cfd_handle h, const cfd_t5_args* a, float* out, void* stream);

/* Replaces the reference's Mel front end, which its data loader runs on the CPU with librosa 0.10 (convofusion/data/beat_dnd/dataset.py:
 * get_melspecs :506-520, check_audio :477-492, beat_extract_audio :473; per-window slicing unbounded_synthesis.py:279-308): waveforms to
 * log-Mel frames, to the audio memories of AudioConvEncoder and to the activity bits, float32 throughout, in 4 launches + 3 for the MLP
 * (csrc/audio_fe.hpp).  Semantics: librosa.feature.melspectrogram(y, sr, n_fft, hop_length, n_mels) with its defaults (center=True,
 * pad_mode="constant", win_length = n_fft, periodic Hann, power 2, Slaney filterbank) followed by power_to_db(ref=np.max, amin, top_db):
 * T = 1 + n_samples / hop frames; dB = 10 log10(max(amin, S)) - 10 log10(max(amin, max S)), the max over the ONE waveform's whole
 * spectrogram, clipped below at -top_db.  No atomics; the same bits on every call; a waveform's bits do not depend on the batch; a
 * window's rows are the bits of the same frames of the whole spectrogram.
 *   wave        dev float32 [n_wave][n_samples]: mono, equal length, at the sample rate the filterbank was built for.  1 <= n_wave <= 65535,
 *               1 <= n_samples <= 2^26 (CFD_E_SHAPE otherwise)
 *   normalize   1: every waveform is divided by its own max|y| first (librosa.util.normalize); a peak below FLT_MIN leaves it unchanged
 *   n_fft       256, 512, 1024 or 2048; hop >= 1; 1 <= n_mels <= n_fft / 2 + 1 (CFD_E_ARG otherwise)
 *   twiddle     dev float32 [n_fft][2]: (cos, -sin)(2 pi k / n_fft), computed in float64 and rounded once
 *   window      dev float32 [n_fft]: the periodic Hann window, computed in float64
 *   melfb       dev float32 [n_mels][n_fft / 2 + 1], dense
 *   mel_range   dev int32 [n_mels][2] or NULL: first and one-past-last bin of every band's non-zero weights; a band is summed over that
 *               range only (the bins outside weigh 0, so the sum is the same).  NULL: every band over all bins.
 *   amin, top_db   > 0, >= 0 (the reference: 1e-10, 80)
 *   n_win, win_start, win_frames   0 <= n_win <= 64 frame ranges [win_start[w], win_start[w] + win_frames) taken from every waveform;
 *               win_start is HOST int32 [n_win].  n_win = 0: the whole spectrogram (frames = T).  A range outside [0, T]: CFD_E_SHAPE.
 *   w0 b0 w1 b1 w2 b2, hidden, latent   AudioConvEncoder's main.0 [hidden][n_mels], main.3 [latent][hidden], out_net [latent][latent]
 *               with their biases, dev float32; LeakyReLU(0.1) behind the first two.  All NULL: no encoder.
 *   act_chunk, act_amin_power, act_thresh_power   the activity bit of chunk j < n_samples / act_chunk (whole chunks only) is
 *               max(act_amin_power, max|y|^2) > act_thresh_power on the waveform after normalisation: amplitude_to_db(chunk, ref=1).max()
 *               > threshold restated in power (the reference: 10240 samples, 1e-10, 10^-4.5)
 * Outputs, each may be NULL: mel_db [n_wave * max(n_win, 1)][frames][n_mels], memory [same rows][frames][latent] (needs the weights:
 * CFD_E_ARG without), activity int32 [n_wave][n_samples / act_chunk] (needs act_chunk >= 1), peak [n_wave] (max|y| before
 * normalisation).  Row u * n_win + w is window w of waveform u.
 * Everything is refused before the first launch.  The workspace lives on the handle and only grows. */
typedef struct {
  const float* wave;
  int n_wave;
  long long n_samples;
  int normalize;
  int n_fft, hop, n_mels;
  const float* twiddle;
  const float* window;
  const float* melfb;
  const int32_t* mel_range;
  float amin, top_db;
  int n_win;
  const int32_t* win_start;
  int win_frames;
  const float *w0, *b0, *w1, *b1, *w2, *b2;
  int hidden, latent;
  int act_chunk;
  float act_amin_power, act_thresh_power;
} cfd_audio_args;
int cfd_audio_encode(cfd_handle h, const cfd_audio_args* a, float* mel_db, float* memory, int32_t* activity, float* peak, void* stream);

/* The backward pass of AudioConvEncoder (audioenc.py:9-34; the module the reference trains against its denoising loss,
 * convofusion.py:552-584, 785-813): from the gradient at its output -- d_mem["alsn"] of cfd_denoise_vjp_mem -- the gradients of its three
 * weights, three biases and, where asked, its Mel frames, float32 throughout (csrc/audio_enc_bwd.hpp).  Dropout is the identity.  Per row r:
 *   z1 = x W0^T + b0, h1 = leaky(z1), z2 = h1 W1^T + b1, h2 = leaky(z2), y = h2 W2^T + b2          (leaky: slope 0.1 below 0)
 *   dW2 = d_out^T h2, db2 = sum_r d_out;  dz2 = (d_out W2) * leaky'(z2), dW1 = dz2^T h1, db1 = sum_r dz2
 *   dz1 = (dz2 W1) * leaky'(z1), dW0 = dz1^T x, db0 = sum_r dz1;  d_x = dz1 W0
 * leaky'(z) is 1 for z > 0 and 0.1 otherwise (torch's convention at exactly 0).  The forward is recomputed inside the call with the
 * launches of cfd_linear_act, so `out` carries the bits of three cfd_linear_act calls.  Every sum is one FMA chain in ascending order;
 * a weight gradient's rows are summed in segments of max(512, n_rows / 16 rounded up to 32) rows and the segments in ascending order.
 * No atomics: two calls give the same bits, and a call that asks for less gives the bits of the call that asks for everything.
 *   x           dev float32 [n_rows][in_dim]: Mel frames in dB.  1 <= n_rows <= 65535 * 32 (CFD_E_SHAPE otherwise)
 *   in_dim, hidden, latent   each in 1 .. 1024 (CFD_E_SHAPE otherwise)
 *   w0 b0 w1 b1 w2 b2   as in cfd_audio_args: [hidden][in_dim], [latent][hidden], [latent][latent] and their biases; none may be NULL
 *   d_out       dev float32 [n_rows][latent], not NULL (CFD_E_ARG)
 * Outputs, each may be NULL but not all (CFD_E_ARG): out [n_rows][latent]; d_param[6] in the order w0 b0 w1 b1 w2 b2, each of its
 * parameter's shape (d_param itself may be NULL); d_x [n_rows][in_dim].
 * Launches: 2 (h1, h2) + 1 with out + 1 (dz2) where anything of layers 0 / 1 or d_x is wanted + 1 (dz1) where anything of layer 0 or
 * d_x is + 1 with d_x + 1 for all parameter gradients + 1 closing pass beyond 512 rows: 8 with everything wanted, 7 up to 512 rows.
 * Everything is refused before the first launch.  The workspace lives on the handle and only grows. */
typedef struct {
  const float* x;
  long long n_rows;
  int in_dim, hidden, latent;
  const float *w0, *b0, *w1, *b1, *w2, *b2;
} cfd_audio_enc_args;
int cfd_audio_encoder_vjp(cfd_handle h, const cfd_audio_enc_args* a, const float* d_out, float* out, float* const d_param[6], float* d_x,
                          void* stream);

/* The audio onsets of the beat alignment, on the device: what the reference's Alignment.load_audio (quant_eval/metric_eval.py:102-122,
 * dyadic_eval.py:96-114) gets from librosa 0.10 on the host, one clip at a time -- onset_strength(y, sr), onset_detect(onset_envelope,
 * backtrack=False), feature.rms(S=|stft(y)|), onset_backtrack, frames_to_time -- as the CSR pair cfd_motion_eval takes, in 3 launches
 * (+ 1 with normalize; csrc/onset_fe.hpp).  float32 spectra and envelope, int32 frames, float64 times.  With T = 1 + n_samples / hop:
 *   Mel power M[t][m] as cfd_audio_encode's; D = max(10 log10(max(amin, M)), 10 log10(max(amin, max M)) - top_db), the max over the clip
 *   envelope[j] = mean_m max(0, D[j - pad_frames + lag][m] - D[j - pad_frames][m]) for pad_frames <= j < T, else 0
 *               (librosa: lag = 1, pad_frames = lag + n_fft / (2 hop))
 *   x = (envelope - min) / (max(envelope - min) + FLT_MIN); an all-zero or non-finite envelope has no onsets
 *   frame n is a candidate iff x[n] == max x[n - pre_max, n + post_max), x[n] >= mean x[n - pre_avg, n + post_avg) + delta and x[n] != 0,
 *               both windows clipped to [0, T); candidates are accepted in order when n > last accepted + wait
 *   energy r[t] = sqrt(2 (sum_k P[t][k] - P[t][0] / 2 - P[t][n_fft / 2] / 2) / n_fft^2), P the power spectrum of the SAME transform
 *   an onset moves back to the largest i <= n that is an energy minimum: i = 0, or 1 <= i <= T - 2 with r[i] <= r[i - 1] and r[i] < r[i + 1]
 *   time = (frame * time_hop) / time_sr.  The reference passes no sr to onset_detect and frames_to_time, so librosa's default 22050 sets
 *               the five window integers AND the times (time_hop 512, time_sr 22050) although its audio is at 16 kHz; that is the
 *               reference's number.  The two travel as a pair because a product with one rounded scale is not that quotient.
 * No atomics; the same bits on every call; a waveform's results do not depend on the batch.  Equal-length clips only; resampling and file
 * decoding other than plain PCM stay with the caller.
 *   wave ... top_db   as in cfd_audio_args (the reference: n_fft 2048, hop 512, 128 bands, 1e-10, 80); normalize 1 is util.normalize
 *   pre_max, pre_avg, wait >= 0; post_max, post_avg >= 1; delta >= 0; lag >= 1; pad_frames >= lag (CFD_E_ARG otherwise)
 *   T <= 2048, what the detection workgroup's LDS plan holds (CFD_E_SHAPE otherwise)
 *   capacity    entries of onset_t (and frames_raw, frames).  Two accepted onsets are more than `wait` frames apart, so the total cannot
 *               exceed n_wave * ceil(T / (wait + 1)); a capacity below that bound is refused (CFD_E_SHAPE) -- by the bound, before the first
 *               launch, not by the data.  n_wave * T always suffices.
 *   envelope, rms   optional outputs dev float32 [n_wave][T] (the envelope before normalisation)
 *   frames_raw, frames   optional outputs dev int32 [capacity]: the accepted frames and the backtracked ones, segmented by onset_off
 * onset_off dev int32 [n_wave + 1], onset_t dev float64 [capacity], n_total dev int32 [1] or NULL (= onset_off[n_wave]): a device word, so
 * cfd_motion_eval can follow on the same stream with n_onsets = capacity.  A waveform without onsets has an empty segment. */
typedef struct {
  const float* wave;
  int n_wave;
  long long n_samples;
  int normalize;
  int n_fft, hop, n_mels;
  const float* twiddle;
  const float* window;
  const float* melfb;
  const int32_t* mel_range;
  float amin, top_db;
  int lag, pad_frames;
  int pre_max, post_max, pre_avg, post_avg, wait;
  float delta;
  int time_hop;
  double time_sr;
  int capacity;
  float* envelope;
  float* rms;
  int32_t* frames_raw;
  int32_t* frames;
} cfd_onset_args;
int cfd_audio_onsets(cfd_handle h, const cfd_onset_args* a, int32_t* onset_off, double* onset_t, int32_t* n_total, void* stream);

/* Motion evaluation: what the reference's quant_eval/ scripts compute on the host, one motion at a time, from decoded motions
 * [n_seq][n_frames][189] (63 joints x 3) on the device (csrc/metrics_eval.hpp).  1 launch for the per-sequence part; with the FGD embedding
 * 5 more per 128 sequences and 1 for the statistics.  No atomics; reductions in float64 in one fixed order; the same bits on every call; a
 * sequence's per-sequence outputs do not depend on what else is in the batch.
 *   pred        dev float32: n_seq x n_frames rows of `stride` floats, the first 189 used.  1 <= n_seq <= 65535, 24 <= n_frames <= 128,
 *               stride >= 189 (CFD_E_SHAPE otherwise)
 *   target, semantic   dev float32, target laid out as pred, semantic [n_seq][n_frames]; NULL: none
 *   fps, order, sigma, srgr_threshold   metric_eval.py:451-452 uses 25, 10, 0.3, 0.3; dyadic_eval.py:373 order 12, sigma 1.25
 *   onset_off, onset_t, n_onsets   the audio onsets in seconds as a CSR pair: dev int32 [n_seq + 1] and dev float64 [n_onsets]; sequence b
 *               owns onset_t[onset_off[b] .. onset_off[b + 1]) (offsets are clamped to [0, n_onsets]).  cfd_audio_onsets makes the pair from waveforms on the
 *               device (n_onsets = its capacity); resampling and decoding audio files stay with the caller.
 *   fgd_pack, feature_length   HalfEmbeddingNet's pose encoder (motion_autoencoder.py:39-78), folded: per convolution W [N][k C_in]
 *               (column kk C_in + c, the eval-mode BatchNorm folded in) and b [N] for net.0 .. net.3, then out_net and fc_mu as ONE affine
 *               map W [F][59 F] (column t F + c) and b [F] -- their LeakyReLU(True) has negative_slope 1.0 (motion_autoencoder.py:52,55,58).
 *               dev float32, me_pack_floats(F) floats.  Needs n_frames = 128 (CFD_E_SHAPE otherwise).
 *   embed_raw   0: the net takes the processed motion (what the reference's scripts feed it); 1: it takes pred as it is, which is
 *               HalfEmbeddingNet.forward on its own (needs stride = 189, CFD_E_SHAPE otherwise)
 * Outputs, each may be NULL:
 *   l1div       dev float64 [n_seq]: sum over frames and features of |x - the sequence's mean over frames| (metric_eval.py:342-356)
 *   srgr, srgr_count   dev float64 / int32 [n_seq]: sum over frames and joints of [sum_xyz |pred - target| < threshold] x semantic[frame] / 0.165,
 *               and the number of such (frame, joint) pairs (:317-339); need target and semantic (CFD_E_ARG without)
 *   jitter      dev float64 [n_seq]: sum over (n_frames - 1) x 189 of | |d pred| - |d target| | (jitter_metric.py); needs target
 *   beats       dev uint8 [n_seq][6][n_frames - 1]: frame i of track k (joints 5 6 7 9 10 11) is a beat iff its frame-to-frame speed is strictly
 *               below that of frames clip(i +- s) for s = 1 .. order (:124-165: scipy.signal.argrelextrema(np.less, order, mode="clip"))
 *   align       dev float64 [n_seq]: mean over the sequence's onsets of exp(-d^2 / 2 sigma^2), d = distance to the nearest beat of joint 11
 *               at time frame / fps (:262-293); no beat: 0 per onset; no onset: 0 (the caller leaves the sequence out and counts it)
 *   processed   dev float32 [n_seq][n_frames][189]: process_motion (:376-421) -- floor, XZ origin, facing from joints 18 13 9 5 of frame 0,
 *               root-relative joints, wrist-relative hands
 *   embedding   dev float32 [n_seq][feature_length]: the net's mu of the processed motion
 *   stats       dev float64 [1 + F + F F], read and written: n, sum e, sum e e^T of every embedding so far (the Frechet distance itself is the
 *               host's: np.cov with ddof = 1 and scipy.linalg.sqrtm, :21-90)
 * Everything is refused before the first launch.  The workspace lives on the handle and only grows. */
typedef struct {
  const float* pred;
  const float* target;
  const float* semantic;
  int n_seq, n_frames;
  long long stride;
  double fps;
  int order;
  double sigma, srgr_threshold;
  const int32_t* onset_off;
  const double* onset_t;
  int n_onsets;
  const float* fgd_pack;
  int feature_length;
  int embed_raw;
  double* l1div;
  double* srgr;
  int32_t* srgr_count;
  double* jitter;
  uint8_t* beats;
  double* align;
  float* processed;
  float* embedding;
  double* stats;
} cfd_motion_eval_args;
int cfd_motion_eval(cfd_handle h, const cfd_motion_eval_args* a, void* stream);
/* out[0] (dev float64) = the mean over all pairs i < j of the Euclidean distance between rows of x, dev float32 [n][d] (calculate_avg_distance,
 * metric_eval.py:303-314): from the differences, accumulated in float64.  2 <= n <= 8192 (CFD_E_SHAPE otherwise); 2 launches. */
int cfd_motion_diversity(cfd_handle h, const float* x, int n, long long d, double* out, void* stream);

/* float32 pieces of word-excitation guidance (WEG): the attend-and-excite objective on the listener-text attention
 * maps and d(loss)/d(latents) through the denoiser -- what the reference gets from torch autograd over
 * Denoiser.forward (convofusion/models/modeltype/convofusion.py:437-496, iterative_refinement_step :298-388;
 * convofusion/models/tools/word_excitation_guidance.py:11-81).  convofusion_amd/weg.py strings them into the
 * forward-with-saved-activations and the hand-written backward pass; every transpose there is a strided view.
 *   cfd_mat             element (z1, z2, r, c) = p[z1*b1 + z2*b2 + r*rs + c*cs]
 *   cfd_gemm_f32        C(z; m, n) = alpha * sum_k A(z; m, k) B(z; k, n) + bias[n] (+ C when accumulate); nb1 x nb2 batch
 *   cfd_softmax         in-place softmax over [rows][Lk]; key_padding_mask [batch][Lk], batch = row / rows_per_batch
 *   cfd_softmax_bwd     dp <- p * ((dp + extra) - sum_k (dp + extra) p); extra (may be NULL) = gradient arriving at p directly
 *   cfd_layer_norm_bwd  nn.LayerNorm backward with respect to the input; accumulate != 0: dx += result
 *   cfd_ew              element-wise: 0 SiLU, 1 GELU, 2 a*SiLU'(b), 3 a*GELU'(b), 4 a + alpha*b (weg.update_latent),
 *                       5 a + b[r0*s0 + r1*s1 + d] (broadcast add over a [R0][R1][D] tensor), 6 TimeBlock modulate
 *                       a*(1 + b[r1][d]) + b[r1][D + d] (cross_attention.py:433-436), 7 its backward a*(1 + b[r1][d])
 *   cfd_weg_focus       aggregate_attentions + get_max_attention_at_indices (softmax over text[1:last), 3x3 Gaussian sigma 0.5
 *                       on the reflect-padded map, max over frames) + compute_attention_focus_loss, and the gradient with
 *                       respect to att: att / d_att dev [B][NL][L][S], tok_off dev int32 [B+1], tok_idx dev int32 (text
 *                       positions), kernel3 HOST {corner, edge, centre} of the normalised 3x3 kernel, workspace dev
 *                       >= B*(3*L*(last-1) + 3*nt_max) floats, losses dev [B], max_att dev [tok_off[B]]
 *   cfd_sample_write    overwrite the current latents of the open sampling run (the WEG update between two iterations)
 *   cfd_sample_inpaint  do the next iteration's in-painting overwrite of the first preseq_len tokens now (the captured
 *                       iteration then skips it): in the rollout the WEG update lands between the overwrite and the
 *                       replication (unbounded_synthesis.py:70-143); no-op without preseq */
typedef struct {
  const float* p;
  long long rs, cs, b1, b2;
} cfd_mat;
int cfd_gemm_f32(cfd_handle h, int M, int N, int K, int nb1, int nb2, const cfd_mat* A, const cfd_mat* B, const cfd_mat* C, const float* bias,
                 float alpha, int accumulate, void* stream);
int cfd_softmax(cfd_handle h, float* scores, long long rows, int Lk, const uint8_t* key_padding_mask, long long rows_per_batch, void* stream);
int cfd_softmax_bwd(cfd_handle h, const float* p, float* dp, const float* extra, long long rows, int Lk, void* stream);
int cfd_layer_norm_bwd(cfd_handle h, const float* x, const float* gamma, const float* dy, float* dx, long long rows, int D, float eps,
                       int accumulate, void* stream);
int cfd_ew(cfd_handle h, int op, const float* a, const float* b, float* out, size_t numel, int D, int R1, long long s0, long long s1, float alpha,
           void* stream);
int cfd_weg_focus(cfd_handle h, const float* att, int B, int NL, int L, int S, const int32_t* tok_off, const int32_t* tok_idx, int last, int nt_max,
                  const float kernel3[3], float* workspace, float* losses, float* max_att, float* d_att, void* stream);
/* One evaluation of the WEG objective on the text-only guidance chunk and d(loss)/d(latents), all launches enqueued from
 * C++: replaces  latents.requires_grad_(True); _, att = denoiser(latents, t, text_only_states, ...);
 * loss = compute_attention_focus_loss(get_max_attention_at_indices(aggregate_attentions(att[2]), ...));
 * torch.autograd.grad(loss, latents)   (convofusion.py:447-471,490-495; iterative_refinement_step :322-346,372-386).
 *   losses dev [B], max_att dev [tok_off[B]] (>= 1 float), grad dev [B][L][128]; loss_host (may be NULL): mean of losses,
 *   copied back after a stream synchronise (the loop branches on it: `loss > 1 - threshold`, `loss != 0`). */
typedef struct {
  int B, L;                      /* rows of the text-only chunk (the reference requires B == 1 with normalize_eot) */
  int timestep;
  const float* latents;          /* dev [B][L][128] */
  cfd_memory mem[CFD_NUM_MEM];   /* chunk 1 of the guidance batch: U == B, row_map NULL, masks as in cfd_forward */
  const int32_t* tok_off;        /* HOST [B + 1] offsets into tok_idx */
  const int32_t* tok_idx;        /* HOST focus token positions (text positions, BOS = 0), each in [1, last) */
  int last;                      /* text slice [1, last): eot index (normalize_eot) or S_text - 1 */
  float kernel3[3];              /* {corner, edge, centre} of GaussianSmoothing(1, 3, 0.5, dim=2).weight */
  int reuse_memory_side;         /* != 0: the memory CONTENTS (and masks) are those of the previous call, so their LayerNorms and
                                    key / value projections are taken from it (ignored when shapes / pointers differ).
                                    1: the timestep is the previous call's too (the refinement loop at one timestep,
                                       convofusion.py:322-346): its time embedding is reused as well.
                                    2: the timestep may differ (the guided sampling loop evaluates the objective once per
                                       iteration with the same conditioning, convofusion.py:437-471): small problems keep
                                       per-timestep tables for every timestep, built at the first such call (a few ms), and an
                                       evaluation selects its row; larger problems treat a new timestep like 0. */
} cfd_weg_args;
int cfd_weg_eval(cfd_handle h, const cfd_weg_args* args, float* losses, float* max_att, float* grad, float* loss_host, void* stream);
/* One evaluation AND update of word-excitation guidance for B rows that are each their own utterance -- a batch, or the windows of a
 * tied long-form run -- as one device call: row b gets exactly what cfd_weg_eval + weg.update_latent give it alone with B = 1.
 *   text slice   row b uses [1, last_rows[b]) (its own EOT): softmax, the 3x3 reflect-padded smoothing, arg-max and hinge run on the
 *                row's own width; in the maps' gradient key 0 and the keys from last_rows[b] on receive exact zeros.
 *   objective    losses[b] as cfd_weg_eval forms it; the gradient is d losses[b] / d x[b] (upstream factor -1 / nt_b, no 1 / B).  A
 *                row without focus tokens has loss 0 and gradient 0.
 *   update       x_new[b] = x[b] - row_step[b] * g[b]: the host gates a row by giving it its step or 0 (weg.row_steps).
 *   tie          (cfd_guide_args' tie / tie_csr) the objective is evaluated at x~, x with every tied token replaced by its source; a
 *                tied token's gradient is folded onto its source, weighted by the step of the row the TIED token sits in (the row
 *                whose loss it serves); a tied token of x_new takes its source's new value bit for bit, so x_new satisfies the tie:
 *                  grad[s]  = g~[s] + sum_t g~[t]                                 over the tokens t tied to s, ascending (tie_csr)
 *                  x_new[s] = x~[s] - (row_step[r(s)] g~[s] + sum_t row_step[r(t)] g~[t])
 * Launches, eagerly on the handle's own stream behind `stream` (no captured graph): x~ (only with a tie), the time tables and memory
 * side (unless reused), cfd_weg_eval's forward with saved activations, the per-row objective, its reverse sweep, the gated update.
 * Float32 throughout, no atomics: two calls on the same inputs return the same bits.
 *   losses dev [B]; max_att dev [tok_off[B]] (>= 1 float); grad dev [B][L][128] or NULL: the folded, unstepped gradient, tied tokens 0;
 *   x_new dev [B][L][128] or NULL (may alias latents); losses_host HOST [B] or NULL: when given the call waits and fills it (the loop
 *   branches per row on it), otherwise `stream` continues behind the call and the census is read by the handle's next entry point.
 * reuse_memory_side: cfd_weg_args' meaning; cfd_weg_eval and this call reuse what either left.
 * Limits: the row-tile gradient engine only -- CFD_E_ARG names the limit exceeded (L <= 32, B * L <= 700 token rows
 * (CFD_ROWTILE_MAX_ROWS), padded keys <= 1024), before any launch; CFD_E_SHAPE for a row whose slice is shorter than 2; CFD_E_ARG for a
 * focus index outside its row's slice, naming the row; a tie only with its tie_csr. */
typedef struct {
  int B, L;
  int timestep;
  const float* latents;          /* dev [B][L][128] */
  cfd_memory mem[CFD_NUM_MEM];   /* as in cfd_weg_args: U == B, row_map NULL */
  const int32_t* tok_off;        /* HOST [B + 1] offsets into tok_idx */
  const int32_t* tok_idx;        /* HOST focus token positions of row b (text positions, BOS = 0), each in [1, last_rows[b]) */
  const int32_t* last_rows;      /* HOST [B]: row b's text slice is [1, last_rows[b]) */
  float kernel3[3];              /* as in cfd_weg_args */
  const float* row_step;         /* HOST [B] or NULL (every step 0: an evaluation; x_new is then x~) */
  const int32_t* tie;            /* dev [B][L] or NULL, as in cfd_guide_args */
  const int32_t* tie_csr;        /* dev [2 B L + 1] (cfd_guide_tie_csr); NULL without a tie */
  int reuse_memory_side;         /* 0 / 1 / 2, as in cfd_weg_args */
} cfd_weg_rows_args;
int cfd_weg_step(cfd_handle h, const cfd_weg_rows_args* args, float* losses, float* max_att, float* grad, float* x_new, float* losses_host,
                 void* stream);
/* The vector-Jacobian product of one denoiser forward with respect to its sample: replaces
 *   sample.requires_grad_(True); out, _ = denoiser(sample, t, encoder_hidden_states, ...); torch.autograd.grad(out, sample, d_out)
 * for any cotangent d_out at the output (cfd_weg_eval's gradient is hard-wired to the attention-focus objective of the text maps).
 * One call runs the forward with saved activations through the whole network and the reverse sweep of cfd_weg_eval's row-tile path
 * seeded at the output: d_out . latent_proj.weight, decoder.norm, then every layer from the top; no term from the attention maps, no
 * gradients to weights (the memories' gradients: cfd_denoise_vjp_mem, below).  It launches eagerly on the handle's own stream behind `stream` and returns with its results
 * complete.  It shares the row-tile arena and workspace with cfd_weg_eval: a cfd_weg_eval after it reuses nothing
 * (reuse_memory_side is then ignored once), and the bits of a sampling run that is open on the handle are unchanged.
 *   d_out dev [Be][L][128]   the cotangent at the forward's output
 *   out   dev [Be][L][128]   or NULL: the forward's output as this call computed it (cfd_forward's, bit for bit, on the same path)
 *   grad  dev [Be][L][128]   d_out^T . d(out)/d(sample)
 * Limits (those of the row-tile path; CFD_E_ARG names the one exceeded): L <= 32, Be * L <= 700 token rows (CFD_ROWTILE_MAX_ROWS), the
 * padded keys of the five memories together (each length rounded up to 32) <= 1024, one timestep for all rows. */
typedef struct {
  int Be, L;
  int timestep;
  const float* sample;           /* dev [Be][L][128] */
  cfd_memory mem[CFD_NUM_MEM];   /* as in cfd_forward: U distinct memories, an optional row_map [Be], key-padding masks */
} cfd_vjp_args;
int cfd_denoise_vjp(cfd_handle h, const cfd_vjp_args* args, const float* d_out, float* out, float* grad, void* stream);
/* The same call with the vector-Jacobian product with respect to the MEMORIES as well: replaces
 *   torch.autograd.grad(out, encoder_hidden_states, d_out)
 * through the reference module -- what fitting a conditioning tensor to data needs (a new listener identity, a fitted null
 * conditioning, gradient x input attribution).  No weight gradients, no gradients to masks or the timestep.
 *   d_mem[j] dev [U_j][S_j][512] or NULL (not wanted): d_out^T . d(out)/d(mem_j).  With a row_map, instance u receives the SUM over the
 *            batch rows b with row_map_j[b] == u (what autograd gives a tensor that several rows share); an instance no row maps to
 *            and every masked key receive exact zeros.
 *   out      as in cfd_denoise_vjp
 *   grad     as in cfd_denoise_vjp, or NULL: only the sweep's last product (the latent embedding's backward) is then skipped
 * At least one of grad and d_mem[*] must be non-NULL.  Limits, refusals (CFD_E_ARG names the limit), stream behaviour (returns with
 * its results complete), arena and workspace are cfd_denoise_vjp's; with every d_mem[j] NULL the launches are cfd_denoise_vjp's too.
 * Float32 throughout the backward, no atomics: two calls on the same inputs return the same bits.  The first call that asks for a
 * memory gradient builds float32 copies of the folded memory-side weights on the handle (94 MB at nine layers; freed with the
 * handle, rebuilt after cfd_finalize_weights); a handle that never asks pays nothing. */
int cfd_denoise_vjp_mem(cfd_handle h, const cfd_vjp_args* args, const float* d_out, float* out, float* grad, float* const d_mem[CFD_NUM_MEM],
                        void* stream);
/* One guided update of the sampling loop's latents by a key-pose loss of the predicted clean latents, as one device call: replaces
 *   x.requires_grad_(True); e = denoiser(x.repeat(n, 1, 1), t, ...).view(n, B, L, 128)
 *   eps = e[0] + sum_{k=1..n-1} w[:, k] (e[k] - e[0]); x0 = (x - sqrt_1m_acp eps) / sqrt_acp
 *   loss = inv_n sum (mask (x0 - target))^2; g = torch.autograd.grad(loss, x); x_new = x - step g
 * (sampler.sample_with_loss_guidance with edit.keyframe_loss) without autograd and without a host round trip between the stages.
 * B latent rows of L tokens under n evaluated guidance chunks: the forward has Be = n * B rows, chunk-major (row c * B + b is chunk c
 * of latent row b), against `mem` as in cfd_vjp_args (U distinct memories, row_map [Be], masks).  Stages, on the handle's own stream
 * behind `stream`; the call returns with its results complete, as cfd_denoise_vjp does:
 *   1. x~ = x with every tied token replaced by its source's value (tie == NULL: x bit for bit), replicated n times;
 *   2. cfd_denoise_vjp's forward with saved activations;  3. the combine, x0, the loss and the cotangent rows d_out;
 *   4. cfd_denoise_vjp's reverse sweep from d_out;  5. g~[b] = d loss / d x0 / sqrt_acp + the n chunks' rows in ascending order; the fold
 *   g[src] = g~[src] + sum of g~[t] over the tokens t tied to src, ascending (tie_csr); a tied token's own g is 0; x_new = x~ - step g on
 *   free tokens, and a tied token of x_new takes its source's new value bit for bit (the run's overwrite rule applied).
 * Float32 throughout, no atomics: two calls on the same inputs return the same bits.  No memory gradients.  The loss in pose space: cfd_denoise_guide_pose.
 *   loss  dev float, grad dev [B][L][128], x_new dev [B][L][128] (may alias x), d_out dev [Be][L][128] (the cotangent it seeded): each may
 *   be NULL, not all four.
 * reuse_memory_side: 0, or 2 with cfd_weg_args' meaning: the memory CONTENTS, masks and row maps are those of the previous
 * cfd_denoise_guide call on this handle, the timestep may differ.  The call then keeps per-timestep tables for every timestep (built by
 * the first such call) and skips the time-table and memory-side launches while shapes, pointers and instance counts match.  Nothing is
 * shared with the other callers of the row-tile arena: a cfd_weg_eval, cfd_denoise_vjp or cfd_denoise_vjp_mem between two guide calls
 * makes the next guide call run its memory side again, and neither of them reuses what a guide call left (cfd_denoise_guide_pose is a
 * guide call: the two share what they leave).
 * Limits (CFD_E_ARG names the one exceeded, before any launch): L <= 32; Be * L <= 4096 token rows (CFD_GUIDE_MAX_ROWS; this call's own
 * limit in place of CFD_ROWTILE_MAX_ROWS -- the arena of saved activations is ~0.19 MB per token row at nine layers, 0.8 GB at the limit, and an
 * allocation that fails returns CFD_E_HIP); the padded keys of the five memories together <= 1024; one timestep; n >= 1; target, mask and w non-NULL;
 * inv_n > 0; sqrt_acp > 0; a tie only with its tie_csr.  The launches run eagerly (no captured graph). */
typedef struct {
  int B, L, n;
  int timestep;
  float sqrt_acp, sqrt_1m_acp;   /* sqrt(alphas_cumprod[t]), sqrt(1 - alphas_cumprod[t]), rounded from the scheduler's float64 table */
  const float* x;                /* dev [B][L][128] */
  cfd_memory mem[CFD_NUM_MEM];   /* as in cfd_vjp_args, for Be = n * B rows */
  const float* w;                /* dev [B][n]: this iteration's chunk weights; chunk 0 is the base (w[b][0] is not read) */
  const float* target;           /* dev [B][L][128] */
  const float* mask;             /* dev [B][L], 0 or 1 */
  float inv_n;                   /* 1 / (kept tokens * 128) */
  float step;
  const int32_t* tie;            /* dev [B][L]: -1 or the flat index of the token's source (cfd_tie_args), or NULL */
  const int32_t* tie_csr;        /* dev [2 B L + 1]: the inverse table cfd_guide_tie_csr builds; NULL without a tie */
  int reuse_memory_side;         /* 0 or 2 */
} cfd_guide_args;
int cfd_denoise_guide(cfd_handle h, const cfd_guide_args* args, float* loss, float* grad, float* x_new, float* d_out, void* stream);
/* The inverse of a tie table for cfd_guide_args.tie_csr, on the host: tie HOST [n_tokens] -> csr HOST [2 n_tokens + 1] (offsets
 * [n_tokens + 1], then the tied tokens grouped by source, ascending within a source).  CFD_E_ARG for an entry outside [-1, n_tokens), a
 * token tied to itself or a source that is itself tied.  Needs no handle and no device. */
int cfd_guide_tie_csr(const int32_t* tie, long long n_tokens, int32_t* csr);
/* cfd_denoise_guide with the loss in POSE space: the guided update for frame-accurate key poses, replaces
 *   ... x0 as above; feats = vae.decode(loop_to_vae(x0), lengths)
 *   loss = inv_n sum (frame_mask[b][f] feature_mask[j] (feats - target))^2; g = torch.autograd.grad(loss, x); x_new = x - step g
 * (sampler.sample_with_loss_guidance with edit.pose_keyframe_loss) as one device call.  `args` keeps its cfd_denoise_guide meaning --
 * chunk-major forward rows, w, tie / tie_csr, step, reuse_memory_side -- except that args->target and args->mask must be NULL and
 * args->inv_n is not read: the loss is `pose`.  Stages, on the handle's own stream behind `stream`; the call returns complete:
 *   1. x~, replicated;  2. the forward with saved activations;  3. the combine and x0, written in the decoder's layout z[part][b][p][128]
 *   for token l = 2 p + part;  4. cfd_vae_decode_vjp's saving forward of bs = B sequences of L / 2 chunks on THIS handle's VAE workspace;
 *   5. the loss and its cotangent d_feats = 2 inv_n r (a selected frame at or beyond lengths[b] decodes to 0: it counts target^2 towards
 *   the loss and pulls nothing, the sweep does not read its cotangent);  6. cfd_vae_decode_vjp's sweep to d_z;  7. d_x0 read back through
 *   the layout map, d loss / d x0 / sqrt_acp and the cotangent rows d_out as cfd_denoise_guide forms them;  8. cfd_denoise_vjp's reverse
 *   sweep;  9. chunk sum, tie fold and update as in cfd_denoise_guide.
 * Float32 throughout, no atomics: two calls on the same inputs return the same bits.
 *   loss, grad, x_new, d_out as in cfd_denoise_guide; feats dev [B][nframes][189] the decode of the predicted clean latents as the call
 *   computed it.  Each may be NULL, not all five.
 * The call drops whatever forward the handle's cfd_vae_decode kept: a ticket taken on the same handle goes stale, and
 * cfd_vae_decode_sweep's CFD_E_STATE names this call.
 * reuse_memory_side: as in cfd_denoise_guide.  The denoiser's memory side does not depend on the loss, so the two calls share one
 * signature: a pose call with reuse_memory_side = 2 reuses what a cfd_denoise_guide call with the same shapes, pointers and instance
 * counts left, and the other way round; either way the results are a fresh call's bits.
 * Limits (CFD_E_ARG names the one exceeded, before any launch): cfd_denoise_guide's; cfd_vae_decode_vjp's with bs = B, n_chunks = L / 2
 * (so L <= 32 even, nframes <= 256, odd num_layers <= 9 ...); 1 <= nframes <= 16 * (L / 2); pose and every pointer in it non-NULL;
 * pose->inv_n > 0; args->target and args->mask NULL.  The VAE workspace is 27 KB per padded frame row (2 stacks * B * nframes rounded
 * up to 16; 6.9 MB per 128-frame sequence at 5 layers); one that cannot be allocated returns CFD_E_HIP, like the arena. */
typedef struct {
  const float* wpack;                 /* dev: packed decoder weights, as cfd_vae_decode_args */
  int d_model, num_heads, ff_size, num_layers;
  int nframes;                        /* 1 .. 256; n_chunks is args->L / 2 */
  const int32_t* lengths;             /* dev [B], each in [1, nframes] */
  const float* target;                /* dev [B][nframes][189], decode's own (root-subtracted) space */
  const float* frame_mask;            /* dev [B][nframes], 0 or 1 */
  const float* feature_mask;          /* dev [189], 0 or 1 */
  float inv_n;                        /* 1 / (selected frames * selected features) */
} cfd_guide_pose;
int cfd_denoise_guide_pose(cfd_handle h, const cfd_guide_args* args, const cfd_guide_pose* pose,
                           float* loss, float* grad, float* x_new, float* d_out, float* feats, void* stream);
/* ConvoFusionVae.decode together with its vector-Jacobian product with respect to the latents: replaces
 *   z.requires_grad_(True); feats = vae.decode(z, lengths); torch.autograd.grad(feats, z, d_feats)
 * i.e. autograd over convofusion/models/architectures/vae.py:268-372 (two SkipTransformerDecoders, cross_attention.py:66-125, of pre-norm
 * TransformerDecoderLayers :361-382).  One call recomputes the forward of both stacks with saved activations and runs the reverse sweep from
 * the cotangent at the 189 output features back to z (csrc/vae_dec.hpp): exact float32, no atomics -- two calls on the same inputs return
 * the same bits.  z enters only as the cross-attention memory z[s] + mem_pos_decoder.pe; the queries are query_pos_decoder.pe rows.  No
 * gradients to weights or lengths.  Every launch (a few dozen) is enqueued on `stream`; the call does not wait.  The workspace belongs to
 * the handle and to this call alone: a sampling run, a cfd_weg_eval or a cfd_denoise_vjp on the same handle share nothing with it.
 *   feats  dev [bs][nframes][189] or NULL: the forward as this call computed it, frames at or beyond lengths[b] exactly 0
 *   d_z    dev [2][bs][n_chunks][128]: d_feats^T . d(feats)/d(z); cotangent entries of frames at or beyond lengths[b] are not read
 * Limits (CFD_E_ARG names the one exceeded): d_model 128, 2 heads, ff 1024, odd num_layers <= 9; 1 <= nframes <= 256; 1 <= n_chunks <= 16;
 * 1 <= bs <= 65535. */
typedef struct {
  const float* wpack;        /* dev: packed decoder weights of both stacks and the two PE tables, layout in csrc/vae_dec.hpp */
  int d_model, num_heads, ff_size, num_layers;
  int bs, nframes, n_chunks;
  const float* z;            /* dev [2 (body, hands)][bs][n_chunks][128] */
  const int32_t* lengths;    /* dev [bs], each in [1, nframes]; the caller checks max == nframes */
  const float* d_feats;      /* dev [bs][nframes][189]: cotangent at decode's output */
} cfd_vae_decode_vjp_args;
int cfd_vae_decode_vjp(cfd_handle h, const cfd_vae_decode_vjp_args* a, float* feats, float* d_z, void* stream);
/* ConvoFusionVae.decode as a call of its own, on cfd_vae_decode_vjp's forward kernels (the same arithmetic in the same order: the same bits
 * as that call's feats), and the reverse sweep as a second call over a forward that was kept.  cfd_vae_decode_vjp is the two in a row.
 *   cfd_vae_decode, ticket == NULL   forward-only: 1 + (num_layers + 1) + num_layers launches (12 at 5 layers) that store only what a later
 *       forward launch reads.  The workspace holds (num_layers - 1) / 2 + 6 rows of 128 floats per token row (both stacks, frames padded
 *       to 16 per sequence: 2 * bs * fp rows; 4096 bytes each at 5 layers) plus num_layers * 16 KiB per (stack, sequence) for the memory's
 *       K | V -- against 27 KB per token row for the saving forward.  feats must not be NULL.
 *   cfd_vae_decode, ticket != NULL   the forward with saves, on cfd_vae_decode_vjp's workspace; one of its launches also copies the stacks'
 *       packed weights and the lengths into the workspace, so that the sweep reads nothing of the caller's but d_feats.  *ticket names
 *       this kept forward on this handle (never 0).  feats may be NULL.
 *   cfd_vae_decode_sweep   d_z = d_feats^T . d(feats)/d(z) over the kept forward `ticket` names, bit for bit what cfd_vae_decode_vjp
 *       returns for the same inputs; it may run more than once on a ticket.  CFD_E_STATE (the message names the reason) unless `ticket`
 *       is the handle's current kept forward: a ticket goes stale with any later cfd_vae_decode (either mode) or cfd_vae_decode_vjp on
 *       the handle, which includes every growth of the VAE workspace.
 *   cfd_vae_decode_ticket  the current kept forward's ticket, or 0: lets a caller decide before it launches anything.
 * All of them only enqueue on `stream` (a workspace that has to grow is reallocated first).  Arguments, limits and refusals are
 * cfd_vae_decode_vjp's (CFD_E_ARG names the limit exceeded). */
typedef struct {
  const float* wpack;        /* as cfd_vae_decode_vjp_args */
  int d_model, num_heads, ff_size, num_layers;
  int bs, nframes, n_chunks;
  const float* z;
  const int32_t* lengths;
} cfd_vae_decode_args;
int cfd_vae_decode(cfd_handle h, const cfd_vae_decode_args* a, float* feats, uint64_t* ticket, void* stream);
int cfd_vae_decode_sweep(cfd_handle h, uint64_t ticket, const float* d_feats, float* d_z, void* stream);
uint64_t cfd_vae_decode_ticket(cfd_handle h);
int cfd_sample_write(cfd_handle h, const float* latents);
int cfd_sample_inpaint(cfd_handle h);

/* Device N(0,1) draws of the product's counter-based stream (DESIGN.md "RNG"): out dev [B][per_utt]. */
int cfd_philox_normal(cfd_handle h, float* out, int B, int per_utt, uint64_t seed, uint32_t step,
                      uint32_t first_utterance, uint32_t stream_id, void* stream);

/* Measurement hook for bench.py: runs ONE denoiser forward of the currently configured problem eagerly
 * with every kernel class bracketed by HIP events on the launch stream; returns milliseconds per class
 * and the number of launches per class.  Classes: see CFD_PROF_* below. */
#define CFD_PROF_GEMM_TOKEN 0    /* token-side projections (QK, V^T, Wo, TimeBlocks, FFN, embed, proj) */
#define CFD_PROF_GEMM_MEM 1      /* memory-side K / V^T projections */
#define CFD_PROF_GEMM_ATTN 2     /* fused self-attention; score and P.V products of the three-launch cross-attention path */
#define CFD_PROF_ROWS 3          /* LayerNorm / AdaLN / softmax / memory prep */
#define CFD_PROF_OTHER 4
#define CFD_PROF_XATTN 5         /* fused cross-attention kernel (scores + softmax + P.V + residual of the five memories) */
#define CFD_PROF_NCLASS 6
int cfd_profile_forward(cfd_handle h, float ms[CFD_PROF_NCLASS], int launches[CFD_PROF_NCLASS]);

#ifdef __cplusplus
}
#endif
#endif
