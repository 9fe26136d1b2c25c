"""The fused sampling loop: drop-in for ``Convofusion._diffusion_reverse`` (reference
convofusion/models/modeltype/convofusion.py:391-549) and for ``diffusion_reverse_forecast``
(unbounded_synthesis.py:28-187).

The whole loop body -- replicate latents x7, denoiser forward, modality-guidance combine, scheduler
step (and the in-painting overwrite of the rollout) -- is one hipGraph captured by libcfdenoise and
replayed N times; nothing returns to the host between steps (the reference syncs ~3x per step:
``t.item()``, CPU-side scheduler tables, ``if t > 0``).
"""
import ctypes as C
import inspect
import warnings

import torch

from . import _lib
from .denoiser import Denoiser
# the pure half of opening a run: the argument checks of every kind and the kind of a run (importable from here as before)
from .run_kind import (_AUTO_RUN, RunKind, check_anchor, check_edit, check_inversion, check_keyframe_guidance, check_weg_rows,  # noqa: F401
                       check_loss_guidance, check_pose_keyframes, check_noise_space, check_operands, check_tie, edit_first_iteration, refuse_sample_prediction, resolve_run_kind,
                       sample_prediction)

# which guidance chunk carries which conditional memory (reference convofusion.py:909-929, 527-541)
CFG_CHUNKS = 7

# Operand policy of a run's fused cross-attention (cfd_sample_args.operand_policy; 0 = fp16 split pairs everywhere), per scheduler kind
# (scheduler.KIND: 0 DDPM, 1 DDIM, 2 DPM-Solver++).  Non-zero: the attention against the LONG memories (128 padded keys and more: the audio memory) runs on
# single-fp16 operands -- bits 0 / 1: their folded values / keys as single-fp16 tiles, bits 2 / 3: the probabilities / queries of those
# products as one fp16 as well (1 MFMA per product instead of 3); the shipped library implements the four bits together (15).  Measured on
# every DDPM golden (profiles/r06_xa_operands_*): the 1000-step DDPM run at the headline shape ends 2.3e-5 from the
# reference trajectory (pairs: 8e-6; budget 1e-3), its 5-step golden 6.1e-5, the product shape's 20-step golden 9.1e-5, for +12 % headline
# throughput; the DDPM loop re-injects noise every step and does not amplify the perturbation.  DDIM (eta = 0) does -- the 50-step golden goes
# from 1.4e-4 to 4.1e-4 -- and keeps pairs.  ``install(model, operands=0)`` /
# ``sample(..., operands=0)`` is the precision escape for a checkpoint whose attention turns out to be less forgiving than the seeded weights
# (the heavy-tailed stress weights: DESIGN.md section 2).  ``operands="auto"`` (opt-in) decides per run: the default policy with the
# attention-concentration census on, and a restart with pairs from iteration 0 when the census trips (see CENSUS_TAU).
# DPM-Solver++ (kind 2) is deterministic like DDIM -- no noise re-injected, its multistep history carries a perturbation forward -- and keeps
# pairs as well, and so does DDIM inversion (kind 3, DDIMInverseScheduler), for the same reason.  A run whose scheduler has
# prediction_type="sample" keeps pairs whatever its kind (``resolve_run_kind``): the policy's error enters an x0 step through other
# coefficients than an epsilon step, and nobody has measured that case; an explicit ``operands=`` still wins.
OPERAND_POLICY = {0: 15, 1: 0, 2: 0, 3: 0}

# Attention-concentration census (cfd_sample_args.census_tau, ``SamplingRun.census``): the fused cross-attention kernel reports, per layer, the
# largest probability of every query row against a long memory and how many rows exceed CENSUS_TAU.  The single-fp16 operands are safe where
# the attention against the 1500-key audio memory is spread out (the seeded goldens' peaks stay within a small factor of 1 / 1500), not where a
# row concentrates on few keys (the heavy-tailed stress weights); CENSUS_TAU separates the two -- calibration table: DESIGN.md section 2.
# ``operands="auto"`` reads the census every CENSUS_CHUNK iterations.
CENSUS_TAU = 0.05
CENSUS_CHUNK = 100

# Modality guidance weights w_c of the guidance chunks 1 - 6, by the reference's variable names (convofusion.py:527-541: "w_c for each
# modality is kept 1 as a standard"), and the reference's values.  Chunk 0 is the unconditional prediction.
MODALITY_NAMES = ("text", "audio", "spk", "apb", "lsnid", "all")
REFERENCE_MODALITY_WEIGHTS = dict(text=1.0, audio=1.0, spk=1.0, apb=1.0, lsnid=1.0, all=0.0)


def check_modality_weights(modality_weights):
    """The form of ``modality_weights`` without the run's sizes: None, a dict over MODALITY_NAMES (missing keys: the reference's values), or
    a tensor / array of shape [6], [B, 6] or [N, B, 6] (N = len(scheduler.timesteps); [N, 1, 6] broadcasts over utterances), all finite.
    Returns None, the completed dict, or a float64 numpy array.  Anything else raises ValueError."""
    import numpy as np
    if modality_weights is None:
        return None
    if isinstance(modality_weights, dict):
        unknown = set(modality_weights) - set(MODALITY_NAMES)
        if unknown:
            raise ValueError(f"modality_weights: unknown keys {sorted(map(str, unknown))} (known: {', '.join(MODALITY_NAMES)})")
        w = dict(REFERENCE_MODALITY_WEIGHTS)
        for k, v in modality_weights.items():
            try:
                w[k] = float(v)
            except (TypeError, ValueError):
                raise ValueError(f"modality_weights[{k!r}] = {v!r} is not a number") from None
        if not all(np.isfinite(v) for v in w.values()):
            raise ValueError(f"modality_weights: non-finite weight in {w}")
        return w
    if isinstance(modality_weights, torch.Tensor):
        arr = modality_weights.detach().to("cpu", torch.float64).numpy()
    elif isinstance(modality_weights, (str, bytes)):
        raise ValueError(f"modality_weights must be a dict or a tensor / array, not {modality_weights!r}")
    else:
        try:
            arr = np.asarray(modality_weights, dtype=np.float64)
        except (TypeError, ValueError):
            raise ValueError(f"modality_weights must be a dict or a tensor / array, not {type(modality_weights).__name__}") from None
    if arr.ndim not in (1, 2, 3) or arr.shape[-1] != len(MODALITY_NAMES):
        raise ValueError(f"modality_weights must have shape [6], [B, 6] or [N, B, 6], not {list(arr.shape)}")
    if not np.isfinite(arr).all():
        raise ValueError("modality_weights: non-finite weight")
    return arr


def modality_weight_table(modality_weights, guidance_scale, N, B, guidance_chunks=CFG_CHUNKS):
    """The weight table of cfd_sample_begin_weighted: float32 [N, B, 8], entry [i, b, c] = float32(guidance_scale * w_c) with the product
    taken in double -- what the reference computes with w_c edited (``self.guidance_scale * w_c * (e_c - e_0)``, convofusion.py:533-538)
    -- for the guidance chunks c = 1 - 6; column 0 is 0.  ``modality_weights``: see ``check_modality_weights``."""
    import numpy as np
    if int(guidance_chunks) != CFG_CHUNKS:
        raise ValueError(f"modality_weights need the {CFG_CHUNKS}-chunk guidance batch (guidance_chunks = {guidance_chunks})")
    w = check_modality_weights(modality_weights)
    if w is None:
        raise ValueError("modality_weights is None: the run takes the default path")
    if isinstance(w, dict):
        w = np.array([w[k] for k in MODALITY_NAMES], dtype=np.float64)
    if w.ndim == 2 and w.shape[0] != B:
        raise ValueError(f"modality_weights [B, 6] has {w.shape[0]} rows for B = {B} utterances")
    if w.ndim == 3 and (w.shape[0] != N or w.shape[1] not in (1, B)):
        raise ValueError(f"modality_weights [N, B, 6] has shape {list(w.shape)}; the run has N = {N} iterations (len(scheduler.timesteps)) "
                         f"and B = {B} utterances ([N, 1, 6] broadcasts over them)")
    full = np.broadcast_to(w, (N, B, len(MODALITY_NAMES)))
    table = np.zeros((N, B, 8), dtype=np.float32)
    with np.errstate(over="ignore"):
        table[:, :, 1:1 + len(MODALITY_NAMES)] = (float(guidance_scale) * full).astype(np.float32)
    if not np.isfinite(table).all():
        raise ValueError(f"modality_weights: guidance_scale * w overflows float32 (guidance_scale = {guidance_scale})")
    return table


class CensusTripped(Exception):
    """Raised inside an ``operands="auto"`` run when its census counts a row above the threshold (caught by the loop entry points)."""

    def __init__(self, census):
        super().__init__(census)
        self.census = census


def _with_auto_operands(fn, operands):
    """``fn(operands)`` -- for ``operands="auto"`` first with the default policy and the census on; if the census trips, a warning and the
    whole loop again from iteration 0 with ``operands=0`` (same seed, initial latents and step noise: the result is the policy-0 run's)."""
    operands = check_operands(operands)
    if operands != "auto":
        return fn(operands)
    try:
        return fn(_AUTO_RUN)
    except CensusTripped as e:
        c = e.census
        warnings.warn(f"operands='auto': the attention against a long memory concentrates (peak probability {c['peak_max']:.3g} in layer "
                      f"{c['worst_layer']}, {c['rows_over']} rows above {c['tau']:g} within {c['iterations']} iterations): the run is repeated "
                      "from iteration 0 with fp16 split-pair operands (operands=0)", UserWarning, stacklevel=3)
        return fn(0)


def _dedup_rows_exact(m, mk):
    """Row-by-row grouping with exact comparisons (the fallback when two different rows share a hash)."""
    Be = m.shape[0]
    reps, rmap = [], []
    for b in range(Be):
        found = -1
        for ui, rb in enumerate(reps):
            if (mk is None or bool((mk[b] == mk[rb]).all())) and torch.equal(m[b], m[rb]):
                found = ui
                break
        if found < 0:
            reps.append(b)
            found = len(reps) - 1
        rmap.append(found)
    return torch.tensor(reps, device=m.device), torch.tensor(rmap, dtype=torch.int32, device=m.device)


def dedup_memories(encoder_hidden_states, cond_masks=None):
    """Exact de-duplication of the replicated conditioning batch.

    The reference materialises every memory 7x per utterance (convofusion.py:909-929) although each
    takes only two values per utterance -- its own and one shared unconditional tensor.  Rows are grouped by a
    cheap hash on the device (identical rows reduce identically) and every row is then compared bit for bit, masks
    included, with its group's first row; a hash collision between different rows falls back to pairwise exact
    comparisons, so any input works (in the worst case nothing is shared).  Distinct rows keep the order of their first
    occurrence.  Returns (unique 5x[U_j,S_j,512], row_maps 5x int32[Be], unique masks dict)."""
    cond_masks = cond_masks or {}
    uniq, maps, umasks = [], [], {}
    for j, name in enumerate(_lib.MEM_NAMES):
        m = encoder_hidden_states[j].detach().to(torch.float32).contiguous()
        mask = cond_masks.get(name)
        Be = m.shape[0]
        flat = m.reshape(Be, -1)
        mk = mask.to(device=m.device, dtype=torch.uint8).reshape(Be, -1) if mask is not None else None
        cols = [flat.sum(1), (flat * flat).sum(1), flat[:, ::97].sum(1)]
        if mk is not None:
            w = torch.arange(1, mk.shape[1] + 1, device=m.device, dtype=torch.float32)
            cols += [mk.to(torch.float32).sum(1), (mk.to(torch.float32) * w).sum(1)]
        key = torch.stack(cols, dim=1)
        _, inv = torch.unique(key, dim=0, return_inverse=True)
        ar = torch.arange(Be, device=m.device)
        first = torch.full((int(inv.max()) + 1,), Be, device=m.device, dtype=torch.long).scatter_reduce_(0, inv, ar, reduce="amin")
        order = torch.argsort(first)                       # groups in the order of their first row
        rank = torch.empty_like(order)
        rank[order] = torch.arange(order.numel(), device=m.device)
        idx, rmap = first[order], rank[inv]
        rep_row = idx[rmap]                                # every row's group representative
        same = (flat == flat[rep_row]).all(dim=1)
        if mk is not None:
            same &= (mk == mk[rep_row]).all(dim=1)
        if not bool(same.all()):                           # two different rows with one hash: exact pairwise grouping
            idx, rmap = _dedup_rows_exact(m, mk)
        uniq.append(m.index_select(0, idx).contiguous())
        maps.append(rmap.to(torch.int32))
        umasks[name] = mask.index_select(0, idx.to(mask.device)).contiguous() if mask is not None else None
    return uniq, maps, umasks


def build_guidance_batch(cond, uncond, cond_masks=None, uncond_masks=None):
    """Structured alternative to materialising the 7x replicated conditioning batch and de-duplicating it again.

    ``cond``   : 5 tensors [B, S_j, 512]  -- each utterance's own (spk_emb, alsn, tlsn, apb, lsnemb)
    ``uncond`` : 5 tensors [1, S_j, 512]  -- the shared unconditional memories (dummy text, -90 dB Mel,
                 activity bit 2, listener id 0; reference convofusion.py:909-929)
    Returns (unique memories 5x[(B+1), S_j, 512], row_maps 5x int32[7B], unique masks dict) in the
    reference's chunk order [all_drop, text_only, audio_only, spk_only, apb_only, lsnid_only, full]
    (convofusion.py:527-541); pass them to ``SamplingRun(..., dedup=False, row_maps=...)``."""
    cond_chunks = {0: (3, 6), 1: (2, 6), 2: (1, 6), 3: (4, 6), 4: (5, 6)}   # memory j is conditional in these chunks
    B = cond[0].shape[0]
    uniq, maps, masks = [], [], {}
    for j, name in enumerate(_lib.MEM_NAMES):
        uniq.append(torch.cat([uncond[j].to(cond[j].dtype), cond[j]], dim=0).contiguous())
        rm = torch.zeros((CFG_CHUNKS, B), dtype=torch.int32)
        for c in cond_chunks[j]:
            rm[c] = 1 + torch.arange(B, dtype=torch.int32)
        maps.append(rm.reshape(-1).to(cond[j].device))
        cm = (cond_masks or {}).get(name)
        um = (uncond_masks or {}).get(name)
        if cm is None and um is None:
            masks[name] = None
        else:
            S = cond[j].shape[1]
            cm = cm if cm is not None else torch.zeros((B, S), dtype=torch.bool, device=cond[j].device)
            um = um if um is not None else torch.zeros((1, S), dtype=torch.bool, device=cond[j].device)
            masks[name] = torch.cat([um.to(torch.bool), cm.to(torch.bool)], dim=0).contiguous()
    return uniq, maps, masks


def select_memories(encoder_hidden_states, cond_masks, G, B, dedup=True, row_maps=None):
    """The guidance memories of a run or a level-batch call as (memories, row maps or None, masks): already-distinct memories with their
    ``row_maps`` (``build_guidance_batch``), else the G * B-row replicated batch de-duplicated (``dedup_memories``) or as it is."""
    if row_maps is not None:
        if any(int(m.numel()) != G * B for m in row_maps):
            raise ValueError(f"row_maps must have G*B = {G * B} entries")
        return list(encoder_hidden_states), list(row_maps), dict(cond_masks or {})
    if encoder_hidden_states[0].shape[0] != G * B:
        raise ValueError(f"conditioning batch is {encoder_hidden_states[0].shape[0]} rows, expected G*B = {G * B}")
    if dedup:
        return dedup_memories(encoder_hidden_states, cond_masks)
    return list(encoder_hidden_states), None, dict(cond_masks or {})


def fill_scheduler_args(a, scheduler, num_inference_steps, table, eta=0.0):
    """The scheduler part of cfd_sample_args ``a``: kind, counts, clip_sample, eta, set_alpha_to_one, steps_offset, prediction_type,
    alphas_cumprod and the timestep table.  Returns the two host buffers the library reads through ``a``: the caller keeps them alive as
    long as it does."""
    a.scheduler = scheduler.KIND
    a.num_train_timesteps = scheduler.config.num_train_timesteps
    a.num_inference_steps = num_inference_steps
    a.clip_sample = 1 if scheduler.config.get("clip_sample", False) else 0      # (DPM-Solver++ has none)
    a.eta = float(eta)
    a.set_alpha_to_one = 1 if scheduler.config.get("set_alpha_to_one", True) else 0
    a.steps_offset = int(scheduler.config.get("steps_offset", 0))
    a.prediction_type = _lib.PREDICTION_TYPES[scheduler.config.get("prediction_type", "epsilon")]
    acp = scheduler.alphas_cumprod.detach().to("cpu", torch.float32).contiguous()
    a.alphas_cumprod = acp.data_ptr()
    ts = (C.c_int32 * len(table))(*[int(t) for t in table])
    a.timesteps, a.num_timesteps = C.cast(ts, C.c_void_p), len(table)
    return acp, ts


def default_guidance_weights(G, guidance_scale):
    """cfd_sample_args.guidance_weight of the default combine e_0 + sum_k w_k (e_k - e_0) over G chunks: the reference's w_c = 1 for the
    chunks 1 - 5 and guidance_scale * 0 for the full-conditioning chunk 6 (convofusion.py:527-541); fewer chunks: guidance_scale each."""
    w = [0.0] * 8
    if G == CFG_CHUNKS:
        w[1:7] = [float(guidance_scale) * 1] * 5 + [float(guidance_scale) * 0]
    elif G > 1:
        w[1:G] = [float(guidance_scale)] * (G - 1)
    return w


def plain_chunks_evaluated(G, weights, skip_zero_weight_chunks):
    """Guidance chunks a run of the plain opener evaluates.  cfd_sample_begin takes no table and reports no count, so this restates the
    library's ``trim_zero_weight_chunks``: with skip_zero_weight_chunks the trailing chunks of weight 0 are not evaluated."""
    g = G
    while skip_zero_weight_chunks and g > 1 and weights[g - 1] == 0.0:
        g -= 1
    return g


def operand_policy_and_census(a, scheduler_kind, operands, census_tau):
    """cfd_sample_args.operand_policy and census_tau of a run.  Returns whether the run watches its census: "auto" where the kind's
    default policy is not pairs ("auto" with pairs as the default -- DDIM -- is exactly the default run: nothing to decide, no census)."""
    operands = check_operands(operands)
    default_policy = int(OPERAND_POLICY.get(scheduler_kind, 0))
    auto = operands is _AUTO_RUN or operands == "auto"
    guard = auto and default_policy != 0
    a.operand_policy = default_policy if (operands is None or auto) else operands
    if guard and census_tau is None:
        census_tau = CENSUS_TAU
    a.census_tau = float(census_tau or 0.0)
    return guard


def select_opener(lib, kind, B, L, n_full, trajectory=None, weighted=False):
    """The library call that opens a run of ``kind`` as (function, its arguments between cfd_sample_args and the weight table, what they
    keep alive): the argument struct of every piece the kind has, built once, and the one opener that takes them.  Precedence: a tie
    (with or without an edit), then the trajectory ring of an inversion, an anchor, a replay, an edit, else the weighted or plain opener.
    The rings of an anchor and a replay are read in place for the whole run."""
    def ptr(t):
        return t.data_ptr() if t is not None else None
    e = an = ta = rp = None
    if kind.replay is not None:
        rp = _lib.ReplayArgs()
        rp.trajectory, rp.noise, rp.steps, rp.B, rp.L = kind.replay[0].data_ptr(), kind.replay[1].data_ptr(), n_full, B, L
        rp.keep, rp.first_iteration = ptr(kind.replay[2]), kind.replay[3]
    if kind.edit is not None:
        e = _lib.EditArgs()
        e.source, e.keep, e.first_iteration = kind.edit[0].data_ptr(), ptr(kind.edit[1]), kind.edit[2]
    if kind.anchor is not None:
        an = _lib.AnchorArgs()
        an.trajectory, an.steps, an.B, an.L, an.keep = kind.anchor[0].data_ptr(), n_full, B, L, ptr(kind.anchor[1])
    if kind.tie is not None:
        ta = _lib.TieArgs()
        ta.tie = kind.tie.data_ptr()
    keep = [*(kind.replay or ())[:3], *(kind.edit or ())[:2], *(kind.anchor or ()), rp, e, an, ta]
    if ta is not None:
        return lib.cfd_sample_begin_tied, (C.byref(e) if e is not None else None, C.byref(ta)), keep
    if trajectory is not None:
        return lib.cfd_sample_begin_invert, (C.c_void_p(trajectory.data_ptr()),), keep
    if an is not None:
        return lib.cfd_sample_begin_anchored, (C.byref(an),), keep
    if rp is not None:
        return lib.cfd_sample_begin_replay, (C.byref(rp),), keep
    if e is not None:
        return lib.cfd_sample_begin_edit, (C.byref(e),), keep
    return (lib.cfd_sample_begin_weighted if weighted else lib.cfd_sample_begin), (), keep


class SamplingRun:
    """An open sampling run on the device (thin wrapper over cfd_sample_begin/steps/read).  The constructor's arguments, by what they
    select:

    Every run.
    attention_ring: keep the attention maps of the full-conditioning chunk of EVERY iteration (the reference's per-iteration dict,
    convofusion.py:517-523): the captured iteration stores them into ``self.att_ring`` -- five tensors [iterations, B, layers, L, S_j]
    -- with no extra forward and no host round trip (cfd_sample_args.att_ring: the row-tile kernels store them from their second
    cross-attention launch, the fused cross-attention kernel of the tile path from its softmax; a run that has neither -- dynamic
    memories -- gets CFD_E_SHAPE and ``sample`` then takes the maps with one forward per iteration).  The ring is
    iterations x B x layers x L x keys floats: ``sample`` / ``diffusion_reverse`` ask for it only up to ATT_RING_MAX_BYTES.
    ``attention_dict()`` turns the ring into the dict.
    operands: cfd_sample_args.operand_policy of this run (None: OPERAND_POLICY of the scheduler kind).  "auto": that default with the
    census on at CENSUS_TAU, and ``steps`` raises CensusTripped (checked every CENSUS_CHUNK iterations and at the last one) when it trips
    -- the loop entry points (``sample``, ``sample_with_weg``) then repeat the run with ``operands=0``.
    census_tau: cfd_sample_args.census_tau (None / 0: off unless operands="auto"); ``census()`` reads it.
    side_engine: open the run on the denoiser's second library handle (its own weights copy, workspace and stream), so that
    two runs on one module can be open at once (the attention forward of ``last_step_attention`` uses it for a plain forward).
    dynamic_memories: indices j of memories whose CONTENTS the caller rewrites between iterations (DyadicRun's partner
    projection).  All others are constants of the run, as in the reference loop, and the library computes the
    timestep-independent part of their projections once (cfd_sample_args.dynamic_memory_mask).

    A weighted run.
    modality_weights: per-modality guidance weights w_c (``check_modality_weights``: a dict over MODALITY_NAMES, or [6] / [B, 6] /
    [N, B, 6]); the combine is then e_0 + sum_c float32(guidance_scale * w_c) (e_c - e_0) with that table (cfd_sample_begin_weighted),
    and skip_zero_weight_chunks is ignored.  None: the default path (the reference's w_c).  prune_zero_weight_chunks (weighted runs): a
    chunk whose weight is 0 in every iteration for every utterance is not evaluated -- same latents, fewer denoiser rows.
    ``chunks_evaluated``: guidance chunks the run's denoiser evaluates per iteration.

    An edit run.
    source_latents / keep_mask / strength: an edit run (cfd_sample_begin_edit, ``check_edit``; ``convofusion_amd.edit``).  At the start
    of every iteration i the tokens with keep_mask = 1 are set to sa_i * source + sb_i * eps (eps = the run's initial draw), the rollout's
    in-painting with a token mask; strength < 1 starts at iteration k0 = N - min(int(N * strength), N) of the scheduler's table from
    sa_k0 * source + sb_k0 * eps.  ``timesteps`` / ``N`` are then the executed iterations, ``first_iteration`` is k0; step_noise and
    modality_weights [N, ...] still cover the full table (iteration i keeps its full-table index).

    A DDIM inversion.
    trajectory (DDIMInverseScheduler only): record the inversion's trajectory (cfd_sample_begin_invert) into ``self.trajectory``
    [N + 1, B, L, 128]: slot 0 the initial latents (the source), slot j the latents after j iterations, stored by the captured
    iteration's scheduler step.  A DDIM inversion run (scheduler kind 3, ``check_inversion``) refuses preseq, an edit, dynamic memories
    and WEG.

    An anchored run.
    anchor_trajectory / keep_mask (DDIMScheduler, eta 0, no clipping): a re-conditioning run over a recorded inversion trajectory
    (cfd_sample_begin_anchored, ``check_anchor``): at the start of iteration i the tokens with keep_mask = 1 are set to
    anchor_trajectory[N - i], the inverted latents at the level the iteration starts from.  The trajectory is read in place: the run
    keeps a reference to it.

    A tied run.
    tie: a tied run (cfd_sample_begin_tied, ``check_tie``; ``convofusion_amd.longform``): int tensor [B, L], -1 or the flat index
    b' * L + l' of the token that token (b, l) copies at the start of every iteration (the source as the previous iteration left it)
    and once more after the last one: ``read()`` of the finished run has every tied token bit-identical to its source, ``read()``
    before that the latents as the scheduler left them.  Goes with source_latents / keep_mask at strength 1, modality_weights, the
    attention ring and every scheduler but the inverse one; ``write`` (WEG) is refused.  None: the run's usual entry point.

    A replay.
    noise_space / keep_mask / strength (DDPMScheduler): the replay of an edit-friendly DDPM noise space (``invert_ddpm``,
    cfd_sample_begin_replay, ``check_noise_space``): the pair (trajectory [N + 1, B, L, 128], noise [N, B, L, 128]).  The run starts
    from trajectory[N - k0] (k0 from ``strength`` as for an edit: the paper's T_skip), iteration i takes noise[i] as its step noise, and
    the tokens with keep_mask = 1 are set to trajectory[N - i] at the start of iteration i.  init_latents / step_noise are not taken.
    ``operands`` None or "auto" means 0 here whatever OPERAND_POLICY says: the inversion ran on split pairs, and a replay on single-fp16
    audio tiles would not close.  Both rings are read in place: the run keeps references.  ``write`` (WEG) is refused."""

    def __init__(self, denoiser, scheduler, encoder_hidden_states, cond_masks, B, L, num_inference_steps,
                 guidance_scale=7.5, guidance_chunks=CFG_CHUNKS, eta=0.0, init_latents=None, step_noise=None,
                 seed=0, first_utterance=0, preseq=None, dedup=True, skip_zero_weight_chunks=False, row_maps=None,
                 dynamic_memories=(), side_engine=False, attention_ring=False, operands=None, census_tau=None, modality_weights=None,
                 prune_zero_weight_chunks=True, source_latents=None, keep_mask=None, strength=1.0, trajectory=False,
                 anchor_trajectory=None, tie=None, noise_space=None):
        """The stages of opening a run, in order (the arguments: the class docstring); ``sample_begin`` is the library's half."""
        # 1. denoiser, device, scheduler: leaves self.lib / device / _denoiser
        if not isinstance(denoiser, Denoiser):
            raise TypeError("denoiser must be a convofusion_amd.denoiser.Denoiser")
        dev = encoder_hidden_states[0].device
        if dev.type != "cuda":
            raise RuntimeError("the fused sampler runs on an MI355X only (no CPU fallback)")
        self.lib, self.device, self._denoiser = _lib.load(), dev, denoiser
        if getattr(scheduler, "KIND", None) is None:
            raise TypeError("scheduler must be a convofusion_amd.scheduler DDPMScheduler / DDIMScheduler / DPMSolverMultistepScheduler / "
                            "DDIMInverseScheduler")
        # 2. the table: the loop runs over scheduler.timesteps -- DDPM clamps the count to the training schedule, and for a count that does
        # not divide it the (opt-in, unpinned) 0.14.0 table has more entries than the count (scheduler.timestep_table)
        num_inference_steps, table = scheduler.timestep_table(num_inference_steps)
        n_full, G = len(table), guidance_chunks
        # 3. the kind: leaves tie / replay / first_iteration and the executed part of the table (N = loop iterations executed)
        kind = resolve_run_kind(scheduler, table, eta, B=B, L=L, preseq=preseq, source_latents=source_latents, keep_mask=keep_mask,
                                strength=strength, trajectory=trajectory, anchor_trajectory=anchor_trajectory, tie=tie,
                                noise_space=noise_space, init_latents=init_latents, step_noise=step_noise,
                                dynamic_memories=dynamic_memories, operands=operands, device=dev)
        self.tie, self.replay, self.first_iteration = kind.tie, kind.replay is not None, kind.first_iteration
        self.timesteps = [int(t) for t in table][self.first_iteration:]
        self.B, self.L, self.N = B, L, len(self.timesteps)
        # 4. the weighted run's table [N, B, 8] (cfd_sample_begin_weighted), or None: the default path
        self.modality_weights = None if modality_weights is None else modality_weight_table(modality_weights, guidance_scale, n_full, B, G)
        # 5. the memories, distinct rows and their maps
        mems, maps, masks = select_memories(encoder_hidden_states, cond_masks, G, B, dedup, row_maps)
        # 6. the engine handle and the packed memories; _keep: everything the library reads after the opener returns
        self.handle = denoiser.engine(dev, mem_len=max(int(m.shape[1]) for m in mems), side=bool(side_engine))
        marr, keep = Denoiser.pack_memories(mems, masks, maps)
        self._keep = [keep]
        # 7. cfd_sample_args: the scheduler part, the default combine's weights, the rest
        a = _lib.SampleArgs()
        self._keep += fill_scheduler_args(a, scheduler, num_inference_steps, table, eta)
        w = default_guidance_weights(G, guidance_scale)
        self._fill_args(a, G, w, marr, dict(init_latents=init_latents, step_noise=step_noise, preseq=preseq), n_full, seed, first_utterance,
                        skip_zero_weight_chunks, dynamic_memories)
        # 8. operand policy and census: leaves _guard (an "auto" run that watches its census)
        self._guard = operand_policy_and_census(a, scheduler.KIND, kind.operands, census_tau)
        self._checked = self._done = 0
        # 9. the rings: leaves trajectory / att_ring (None where the run has none)
        self._alloc_rings(a, kind.trajectory, attention_ring, skip_zero_weight_chunks, n_full, mems)
        self._args = a
        # 10. the kind's argument structs and the opener that takes them
        opener, extra, keep = select_opener(self.lib, kind, B, L, n_full, self.trajectory, self.modality_weights is not None)
        self._keep += keep
        # 11. the call: leaves chunks_evaluated and the run open
        self._begin(opener, extra, w, skip_zero_weight_chunks, prune_zero_weight_chunks)

    def _fill_args(self, a, G, weights, marr, tensors, n_full, seed, first_utterance, skip_zero_weight_chunks, dynamic_memories):
        """Everything of cfd_sample_args but the scheduler part, the operand policy and the attention ring; the caller's tensors
        (init_latents, step_noise, preseq) as float32 on the device, kept alive by the run."""
        B, L = self.B, self.L
        a.B, a.L, a.G = B, L, G
        a.guidance_weight = (C.c_float * 8)(*weights)
        for name, shape, text in (("init_latents", (B, L, 128), "[B, L, 128]"),
                                  ("step_noise", (n_full, B, L, 128), "[len(scheduler.timesteps), B, L, 128]")):
            if tensors[name] is not None and tuple(tensors[name].shape) != shape:
                raise ValueError(f"{name} must be {text}")
        for name, t in tensors.items():
            if t is not None:
                t = t.detach().to(device=self.device, dtype=torch.float32).contiguous()
                self._keep.append(t)
                setattr(a, name, t.data_ptr())
        a.preseq_len = int(tensors["preseq"].shape[1]) if tensors["preseq"] is not None else 0
        a.seed = int(seed) & 0xFFFFFFFFFFFFFFFF
        a.first_utterance = int(first_utterance)
        a.mem = marr
        # the full-conditioning chunk enters the combine with weight guidance_scale * 0 (convofusion.py:538):
        # optionally do not evaluate it (identical latents, 1/7 less work; the reference needs it only for
        # the per-step attention maps it logs)
        a.skip_zero_weight_chunks = 1 if skip_zero_weight_chunks else 0
        a.dynamic_memory_mask = sum(1 << int(j) for j in set(dynamic_memories))

    def _alloc_rings(self, a, record_trajectory, attention_ring, skip_zero_weight_chunks, n_full, mems):
        """self.trajectory (an inversion that records it) and self.att_ring with cfd_sample_args.att_ring, or None."""
        B, L, dev = self.B, self.L, self.device
        self.att_ring = None
        self.trajectory = None
        if record_trajectory:     # torch.empty: slot 0 is written at begin, slot j by iteration j - 1
            self.trajectory = torch.empty((n_full + 1, B, L, 128), dtype=torch.float32, device=dev)
        if attention_ring:
            if skip_zero_weight_chunks:
                raise ValueError("attention_ring keeps the last guidance chunk's maps: that chunk must be evaluated (skip_zero_weight_chunks=False)")
            nl = int(self._denoiser.num_layers)
            # memory lengths as the CALLER sees them (the maps' key axis); torch.empty: every element is written by the iteration that owns the slot
            self.att_ring = [torch.empty((self.N, B, nl, L, int(m.shape[1])), dtype=torch.float32, device=dev) for m in mems]
            a.att_ring = (C.c_void_p * _lib.NUM_MEM)(*[t.data_ptr() for t in self.att_ring])

    def _begin(self, opener, extra, weights, skip_zero_weight_chunks, prune_zero_weight_chunks):
        """Calls the opener on torch's current stream; every opener but the plain one takes the weight table (or NULL) and the pruning
        switch and reports the chunks it evaluates."""
        a, dev = self._args, self.device
        plain = opener is self.lib.cfd_sample_begin
        g_eval = C.c_int(plain_chunks_evaluated(a.G, weights, skip_zero_weight_chunks) if plain else a.G)
        w_ptr = self.modality_weights.ctypes.data_as(C.c_void_p) if self.modality_weights is not None else None
        table_args = () if plain else (w_ptr, 1 if prune_zero_weight_chunks else 0, C.byref(g_eval))
        with torch.cuda.device(dev):
            torch.cuda.current_stream(dev).synchronize()
            _lib.check(opener(self.handle, C.byref(a), *extra, *table_args, C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)))
        self.chunks_evaluated = int(g_eval.value)
        self.open = True

    def steps(self, n):
        n = int(n)
        if n <= 0:   # (the library checks the run and the count)
            with torch.cuda.device(self.device):
                _lib.check(self.lib.cfd_sample_steps(self.handle, n))
        while n > 0:
            k = n
            if self._guard:   # up to the next census check
                k = min(n, self._checked + CENSUS_CHUNK - self._done)
            with torch.cuda.device(self.device):
                _lib.check(self.lib.cfd_sample_steps(self.handle, k))
            self._done += k
            n -= k
            if self._guard and (self._done - self._checked >= CENSUS_CHUNK or self._done == self.N):
                self._checked = self._done
                c = self.census()
                if c["measured"] and c["rows_over"] > 0:
                    raise CensusTripped(c)

    def census(self):
        """The run's attention-concentration census so far (cfd_sample_census; waits for the run's stream): dict with tau, measured,
        iterations, worst_layer, peak_max, rows_over, rows_seen and the per-layer lists layer_peak / layer_over.  measured = False: nothing of
        the run could count (census off, or a run without the fused cross-attention kernel: the row-tile path, att_ring, dynamic memories)."""
        c = _lib.Census()
        with torch.cuda.device(self.device):
            _lib.check(self.lib.cfd_sample_census(self.handle, C.byref(c)))
        nl = min(_lib.CENSUS_MAX_LAYERS, int(self._denoiser.num_layers))
        return dict(tau=float(c.tau), measured=bool(c.measured), iterations=int(c.iterations), worst_layer=int(c.worst_layer),
                    peak_max=float(c.peak_max), rows_over=int(c.rows_over), rows_seen=int(c.rows_seen),
                    layer_peak=[float(c.layer_peak[i]) for i in range(nl)], layer_over=[int(c.layer_over[i]) for i in range(nl)])

    def attention_dict(self, upto=None):
        """{timestep: [5 tensors [B, layers, L, S_j]]} of the iterations executed so far (views into the ring; read the latents first --
        ``read`` waits for the run's stream)."""
        if self.att_ring is None:
            raise RuntimeError("the run was opened without attention_ring=True")
        n = self._done if upto is None else int(upto)     # (also valid after the run has been closed)
        return {int(t): [r[i] for r in self.att_ring] for i, t in enumerate(self.timesteps[:n])}

    @property
    def position(self):
        return self.lib.cfd_sample_position(self.handle)

    def read(self, close=False):
        out = torch.empty((self.B, self.L, 128), dtype=torch.float32, device=self.device)
        with torch.cuda.device(self.device):
            _lib.check(self.lib.cfd_sample_read(self.handle, C.c_void_p(out.data_ptr()), 1 if close else 0))
        if close:
            self.open = False
        return out

    def write(self, latents, satisfies_tie=False):
        """Overwrite the current latents of the open run (the WEG update between two iterations).  satisfies_tie: the caller states
        that every tied token of ``latents`` already holds its source's value (``Denoiser.guide``'s x_new does), which is the only
        way a tied run takes an update: the run's own overwrite then changes nothing."""
        if self.tie is not None and not satisfies_tie:
            raise ValueError("a tied run takes no WEG update (write): its tied tokens are overwritten from their sources every iteration")
        if self.replay:
            raise ValueError("a replay of a noise space takes no WEG update (write): its noise was solved for the recorded levels")
        if tuple(latents.shape) != (self.B, self.L, 128):
            raise ValueError(f"latents must be [{self.B}, {self.L}, 128]")
        lat = latents.detach().to(device=self.device, dtype=torch.float32).contiguous()
        with torch.cuda.device(self.device):
            torch.cuda.current_stream(self.device).synchronize()
            _lib.check(self.lib.cfd_sample_write(self.handle, C.c_void_p(lat.data_ptr())))

    def inpaint(self):
        """Do the next iteration's in-painting overwrite now (the captured iteration then skips it)."""
        with torch.cuda.device(self.device):
            _lib.check(self.lib.cfd_sample_inpaint(self.handle))

    def profile(self):
        ms = (C.c_float * len(_lib.PROF_CLASSES))()
        n = (C.c_int * len(_lib.PROF_CLASSES))()
        with torch.cuda.device(self.device):
            _lib.check(self.lib.cfd_profile_forward(self.handle, ms, n))
        return {k: (float(ms[i]), int(n[i])) for i, k in enumerate(_lib.PROF_CLASSES)}

    def close(self):
        if self.open:
            try:
                self.read(close=True)
            finally:
                self.open = False

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def guidance_chunk_rows(encoder_hidden_states, cond_masks, chunks, G, B, row_maps=None):
    """(memories, masks) of the guidance chunks ``chunks`` of a chunk-major guidance batch of G chunks x B utterances, in list order:
    slices of the replicated batch, or -- with ``row_maps`` (``build_guidance_batch``) -- the distinct memories gathered through the
    maps' rows c * B .. (c + 1) * B of every listed chunk.  A mask goes by its memory's index in ``_lib.MEM_NAMES``; None stays None."""
    def rows(x, j):
        if row_maps is not None:
            return x.index_select(0, torch.cat([row_maps[j][c * B:(c + 1) * B] for c in chunks]).long().to(x.device))
        parts = [x.chunk(G)[c] for c in chunks]
        return parts[0] if len(parts) == 1 else torch.cat(parts)
    return ([rows(e, j) for j, e in enumerate(encoder_hidden_states)],
            {k: (rows(v, _lib.MEM_NAMES.index(k)) if v is not None else None) for k, v in (cond_masks or {}).items()})


def last_step_attention(run, denoiser, timestep, encoder_hidden_states, cond_masks, guidance_chunks=CFG_CHUNKS, row_maps=None):
    """The attention maps the reference keeps from an iteration: ``att_mats`` of the LAST guidance chunk (full
    conditioning) of the denoiser call (convofusion.py:517-523, unbounded_synthesis.py:159-161) -- 5 tensors
    [B, layers, L, S_j].  Call it right before ``run.steps(1)`` of that iteration: the in-painting overwrite of the rollout
    is pulled in front (``run.inpaint``), the maps come from one extra forward of the B full-conditioning rows on the
    denoiser's second engine (the run owns the first), so a loop that skips the zero-weight chunk still returns them."""
    run.inpaint()
    lat = run.read()
    enc, masks = guidance_chunk_rows(encoder_hidden_states, cond_masks, [guidance_chunks - 1], guidance_chunks, run.B, row_maps)
    keep = denoiser.return_attention
    denoiser.return_attention = True
    try:
        with torch.no_grad():
            _, att = denoiser(sample=lat, timestep=int(timestep), encoder_hidden_states=enc, mem_mask_dict=masks, side_engine=True)
        # the side engine's forward runs on torch's current stream, the captured iteration replays on the run's own stream: wait
        # here, so that the two never execute side by side (two queues at once are not reliable on this stack)
        torch.cuda.current_stream(lat.device).synchronize()
    finally:
        denoiser.return_attention = keep
    return att


# Largest attention ring the loop drop-ins allocate by themselves (bytes): the product shape with 32 utterances and 1000 iterations is
# 4.0 GB (test.py's batch: it must fit); the headline shape (196 tokens, 1500 audio keys) would be 356 MB PER ITERATION.  Beyond it -- or
# beyond half of the memory that is free on the device right now -- "auto" keeps the last entry.  What the ring costs where it is kept:
# the zero-weight full-conditioning chunk is evaluated (it is what the maps come from; "last" skips it: 1/7 of the rows) plus 2 - 5 % for
# the stores, i.e. ~ +20 % run time against attention_steps="last" (DESIGN.md section 11.4); the ring stays alive as long as the
# returned dict's views do.
ATT_RING_MAX_BYTES = 6 << 30


def _open_run(denoiser, scheduler, encoder_hidden_states, cond_masks, B, L, num_inference_steps, want_ring, **kw):
    """SamplingRun with the attention ring when every iteration's maps are wanted, the ring fits ATT_RING_MAX_BYTES and the run is one
    the library keeps them for (every run but those with dynamic memories or with the fused cross-attention switched off); otherwise --
    CFD_E_SHAPE from cfd_sample_begin -- a plain run, and the caller takes the maps with one forward per iteration (``last_step_attention``)."""
    if want_ring:
        n_it = len(scheduler.timestep_table(num_inference_steps)[1])
        if kw.get("source_latents") is not None or kw.get("noise_space") is not None:      # an edit run / a replay executes the iterations from k0 on (its ring has that many slots)
            n_it -= edit_first_iteration(kw.get("strength", 1.0), n_it)
        keys = sum(int(m.shape[1]) for m in encoder_hidden_states)
        budget = ATT_RING_MAX_BYTES
        dev = encoder_hidden_states[0].device
        if dev.type == "cuda":
            budget = min(budget, torch.cuda.mem_get_info(dev)[0] // 2)
        want_ring = 4 * n_it * B * int(denoiser.num_layers) * L * keys <= budget
    if want_ring:
        try:
            return SamplingRun(denoiser, scheduler, encoder_hidden_states, cond_masks, B, L, num_inference_steps,
                               **dict(kw, attention_ring=True, skip_zero_weight_chunks=False))
        except _lib.CfdError as e:
            # CFD_E_SHAPE: a run whose maps the captured iteration cannot keep; CFD_E_HIP: the library's own buffers for the maps did not
            # fit (hipMalloc failed) -- either way the maps are taken the other way; anything else is the caller's error
            if e.code not in (-2, -4):
                raise
        except torch.cuda.OutOfMemoryError:
            pass                  # the ring did not fit beside what the caller holds: the maps are taken the other way
    return SamplingRun(denoiser, scheduler, encoder_hidden_states, cond_masks, B, L, num_inference_steps, **kw)


DONE = object()     # an ``update``'s answer (``_drive``): not this iteration and none after it


def _drive(run, denoiser, encoder_hidden_states, cond_masks, G, row_maps, return_attention, update=None, write=None):
    """Every iteration of the open ``run``, the final read and the close (also on an exception): what ``sample`` and the guided loops
    share.  Returns the latents, with ``return_attention`` (latents, maps) as ``sample`` describes them.
    ``update(i, t, latents) -> new latents | None | DONE`` is what a guided loop does before iteration i of the scheduler's full table
    (timestep t): ``latents()`` pulls the iteration's in-painting overwrite in front (``run.inpaint``; rollout / edit: the re-noised
    tokens go in before the update, unbounded_synthesis.py:70-76) and reads the current latents, and what ``update`` returns is written
    back; None leaves the iteration as it is (nothing read), DONE this one and every later one.  An iteration that is changed, or whose
    maps are taken, is replayed at once; the un-changed ones before it go out as one ``steps`` call.  ``write``: what writes an update
    back (default ``run.write``)."""
    write = run.write if write is None else write
    try:
        ring = run.att_ring is not None and return_attention in ("all", "auto")   # the captured iteration keeps every iteration's maps
        every = return_attention == "all" and not ring     # the reference's dict (convofusion.py:517-523): one extra forward + sync per step
        last = run.first_iteration + run.N - 1
        atts, idle = {}, 0         # idle: un-changed iterations not replayed yet (they go out as one ``steps(idle)``)

        def replay(n):
            if n:
                run.steps(n)
            return 0

        def latents():
            nonlocal idle
            idle = replay(idle)
            run.inpaint()
            return run.read()

        for i, t in enumerate(run.timesteps, start=run.first_iteration):
            new = update(i, t, latents) if update is not None else None
            if new is DONE:
                update = new = None
            maps = every or (return_attention and not ring and i == last)
            if new is None and not maps:
                idle += 1
                continue
            idle = replay(idle)
            if new is not None:
                write(new)
            if maps:
                atts[int(t)] = last_step_attention(run, denoiser, t, encoder_hidden_states, cond_masks, G, row_maps)
            run.steps(1)
        replay(idle)
        lat = run.read(close=not ring)
        if ring:
            atts = run.attention_dict()
        if not return_attention:
            return lat
        return (lat, atts) if return_attention in ("all", "auto") else (lat, atts[int(run.timesteps[-1])])
    finally:
        run.close()     # an exception (bad focus index, CfdError ...) must not leave the run open on the denoiser's handle


def sample(denoiser, scheduler, encoder_hidden_states, cond_masks=None, *, B, L=16, num_inference_steps=1000,
           guidance_scale=7.5, guidance_chunks=CFG_CHUNKS, eta=0.0, init_latents=None, step_noise=None, seed=0,
           first_utterance=0, preseq=None, dedup=True, skip_zero_weight_chunks=False, row_maps=None, return_attention=False, operands=None,
           modality_weights=None, prune_zero_weight_chunks=True, source_latents=None, keep_mask=None, strength=1.0, anchor_trajectory=None,
           tie=None, noise_space=None):
    """Run the whole loop; returns latents [B, L, 128] (batch-first); with ``return_attention=True`` also the last
    iteration's attention maps (``last_step_attention``), with ``return_attention="all"`` a dict {timestep: maps} over every
    iteration like the reference's: kept by the captured iteration itself (``SamplingRun(attention_ring=True)``) while the ring fits
    ATT_RING_MAX_BYTES, otherwise taken with one extra forward and one host round trip per step; ``return_attention="auto"`` always
    returns a dict: every iteration's entries where the captured iteration keeps them itself, the last iteration's entry otherwise.
    ``operands``: None (OPERAND_POLICY of the scheduler kind), an operand policy, or "auto": the default policy while the census
    (CENSUS_TAU) finds no concentrated attention against a long memory; when it trips -- read every CENSUS_CHUNK iterations -- a
    UserWarning, and the loop runs again from iteration 0 with ``operands=0``.  The result is then bit for bit the policy-0 run's (same
    seed, initial latents and step noise), otherwise the default policy's; the worst case costs up to one extra partial run.
    ``modality_weights`` / ``prune_zero_weight_chunks``: per-modality guidance weights, as in ``SamplingRun``.
    ``source_latents`` / ``keep_mask`` / ``strength``: an edit run (token-masked in-painting, img2img strength), as in ``SamplingRun``; the
    attention dict then holds the executed iterations.  ``anchor_trajectory`` / ``keep_mask``: a re-conditioning run over a recorded DDIM
    inversion (``invert``), as in ``SamplingRun``.  With a ``DDIMInverseScheduler`` and ``init_latents`` = the source the loop is a DDIM
    inversion: the same latents as ``invert`` with the same guidance.  ``tie``: tied tokens (int [B, L], ``check_tie``), as in ``SamplingRun``;
    None changes nothing.  ``noise_space`` = (trajectory, noise) of ``invert_ddpm`` with ``keep_mask`` / ``strength``: the replay of an
    edit-friendly DDPM noise space, as in ``SamplingRun``; ``operands`` None or "auto" is then 0.  It goes with ``modality_weights`` and
    pruning and ``return_attention``; tie, preseq, anchor_trajectory, source_latents, init_latents and step_noise are refused."""
    if (noise_space is not None or sample_prediction(scheduler)) and (operands is None or check_operands(operands) == "auto"):
        operands = 0
    if check_operands(operands) == "auto":
        args = dict(locals())
        return _with_auto_operands(lambda ops: sample(**dict(args, operands=ops)), "auto")
    run = _open_run(denoiser, scheduler, encoder_hidden_states, cond_masks, B, L, num_inference_steps, return_attention in ("all", "auto"),
                    guidance_scale=guidance_scale, guidance_chunks=guidance_chunks, eta=eta, init_latents=init_latents, step_noise=step_noise,
                    seed=seed, first_utterance=first_utterance, preseq=preseq, dedup=dedup, skip_zero_weight_chunks=skip_zero_weight_chunks,
                    row_maps=row_maps, operands=operands, modality_weights=modality_weights, prune_zero_weight_chunks=prune_zero_weight_chunks,
                    source_latents=source_latents, keep_mask=keep_mask, strength=strength, anchor_trajectory=anchor_trajectory,
                    **({} if tie is None else dict(tie=tie)), **({} if noise_space is None else dict(noise_space=noise_space)))
    if return_attention:
        scheduler.set_timesteps(num_inference_steps)
    return _drive(run, denoiser, encoder_hidden_states, cond_masks, guidance_chunks, row_maps, return_attention)


# Guidance of an inversion by default: the conditional prediction alone, eps = e_0 + 1 * (e_full - e_0) at guidance_scale 1 (the
# full-conditioning chunk is the last one); a pruned run evaluates 2 of the 7 chunks.
INVERSION_WEIGHTS = dict(text=0.0, audio=0.0, spk=0.0, apb=0.0, lsnid=0.0, all=1.0)


def invert(denoiser, scheduler, encoder_hidden_states, cond_masks=None, *, source_latents, num_inference_steps=50, guidance_scale=1.0,
           modality_weights=None, return_trajectory=False, operands=None):
    """Deterministic DDIM inversion of ``source_latents`` [B, L, 128] on the fused loop (scheduler kind 3): the noise that the DDIM loop
    with the same table and guidance maps back onto the source.  ``scheduler``: a ``DDIMInverseScheduler``; encoder_hidden_states /
    cond_masks: the 7-chunk guidance batch, as for ``sample``.  The guidance is the weighted combine with ``modality_weights`` at
    ``guidance_scale`` (any table ``modality_weight_table`` accepts); None: INVERSION_WEIGHTS at guidance_scale 1, the conditional prediction
    alone.  Returns the inverted latents [B, L, 128], and with ``return_trajectory=True`` also the trajectory [N + 1, B, L, 128] (slot 0 the
    source, slot j the latents after j iterations), recorded by the captured iteration itself -- the ``anchor_trajectory`` of a
    re-conditioning run (``sample(..., anchor_trajectory=, keep_mask=)``)."""
    if getattr(scheduler, "KIND", None) != 3:
        raise TypeError("invert needs a convofusion_amd.scheduler.DDIMInverseScheduler")
    if not isinstance(source_latents, torch.Tensor) or source_latents.dim() != 3 or int(source_latents.shape[2]) != 128:
        raise ValueError("source_latents must be a tensor [B, L, 128]")
    B, L = int(source_latents.shape[0]), int(source_latents.shape[1])
    weights = INVERSION_WEIGHTS if modality_weights is None else modality_weights
    with SamplingRun(denoiser, scheduler, encoder_hidden_states, cond_masks, B, L, num_inference_steps, guidance_scale=guidance_scale,
                     guidance_chunks=CFG_CHUNKS, init_latents=source_latents, modality_weights=weights, operands=check_operands(operands),
                     trajectory=bool(return_trajectory)) as run:
        run.steps(run.N)
        lat = run.read(close=True)
        return (lat, run.trajectory) if return_trajectory else lat


# Philox stream of the level draws of ``invert_ddpm`` (0: step noise, 1: initial latents)
LEVEL_NOISE_STREAM = 2


def _positive_int(name, v, none_ok=False):
    if not (none_ok and v is None) and (isinstance(v, bool) or int(v) != v or int(v) < 1):
        raise ValueError(f"{name} must be a positive integer{' or None' if none_ok else ''}, not {v!r}")


def _float_tensor_or_none(name, t, shape, shape_text):
    if t is not None and (not isinstance(t, torch.Tensor) or not t.is_floating_point() or tuple(t.shape) != shape):
        raise ValueError(f"{name} must be a floating-point tensor {shape_text}")


def _level_batch_args(denoiser, scheduler, enc, masks, B, L, num_inference_steps, table, seed, first_utterance, dedup, row_maps):
    """What the level-batched DDPM calls (``invert_ddpm``, ``sample_parallel``) share: the de-duplicated memories of the 7-chunk guidance
    batch on the denoiser's engine and the DDPM run's cfd_sample_args over ``table``.  Returns (lib, handle, device, args, keep-alive)."""
    dev = enc[0].device
    if dev.type != "cuda":
        raise RuntimeError("the fused sampler runs on an MI355X only (no CPU fallback)")
    G = CFG_CHUNKS
    mems, maps, mks = select_memories(enc, masks, G, B, dedup, row_maps)
    lib = _lib.load()
    handle = denoiser.engine(dev, mem_len=max(int(m.shape[1]) for m in mems))
    marr, keep = Denoiser.pack_memories(mems, mks, maps)
    a = _lib.SampleArgs()
    a.B, a.L, a.G = B, L, G
    alive = fill_scheduler_args(a, scheduler, num_inference_steps, table)     # (a DDPMScheduler: the callers' check)
    a.seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    a.first_utterance = int(first_utterance)
    a.mem = marr
    return lib, handle, dev, a, (keep, *alive)


def invert_ddpm(denoiser, scheduler, enc, masks=None, *, source_latents, num_inference_steps=1000, guidance_scale=1.0, modality_weights=None,
                seed=0, level_noise=None, levels_per_batch=None, first_utterance=0, dedup=True, row_maps=None, workspace_bytes=None):
    """Edit-friendly DDPM inversion (Huberman-Spiegelglas et al., CVPR 2024) of ``source_latents`` [B, L, 128] (cfd_ddpm_invert): for every
    iteration i of the DDPM table an independent level x_i = sqrt(abar_i) source + sqrt(1 - abar_i) eps_i, the guided prediction at every
    level under the conditioning ``enc`` / ``masks`` (the 7-chunk guidance batch, as for ``sample``), and the step noise
    z_i = (x_{i+1} - mu_i(x_i)) / sigma_i that makes the DDPM loop walk these levels.  The N evaluations are independent and run as a few
    large forwards of ``levels_per_batch`` levels each (None: chosen from a workspace budget, ``workspace_bytes``, 4 GiB by default), on
    split-pair operands.  ``scheduler``: a ``DDPMScheduler`` (clip_sample honoured).  The guidance is the weighted combine with
    ``modality_weights`` at ``guidance_scale``; None: INVERSION_WEIGHTS at guidance_scale 1, as for ``invert``.  ``level_noise``
    [N, B, L, 128]: the eps_i; None: Philox stream LEVEL_NOISE_STREAM keyed by ``seed``, step index i, utterance first_utterance + b.
    Returns (trajectory [N + 1, B, L, 128], noise [N, B, L, 128]): slot 0 of the trajectory is the source, slot N - i the level entering
    iteration i; noise[i] is iteration i's step noise, exactly 0 for the last iteration (t = 0 adds none).  Pass the pair to
    ``sample(..., noise_space=, keep_mask=, strength=)``.  ``invert_ddpm.last`` holds dict(chunks_evaluated, levels_per_batch) of the
    last call."""
    if not isinstance(denoiser, Denoiser):
        raise TypeError("denoiser must be a convofusion_amd.denoiser.Denoiser")
    if getattr(scheduler, "KIND", None) != 0:
        raise TypeError("invert_ddpm needs a convofusion_amd.scheduler.DDPMScheduler")
    refuse_sample_prediction(scheduler, "invert_ddpm (the edit-friendly DDPM noise space) runs")
    if not isinstance(source_latents, torch.Tensor) or not source_latents.is_floating_point() or source_latents.dim() != 3 \
            or int(source_latents.shape[2]) != 128:
        raise ValueError("source_latents must be a floating-point tensor [B, L, 128]")
    B, L = int(source_latents.shape[0]), int(source_latents.shape[1])
    num_inference_steps, table = scheduler.timestep_table(num_inference_steps)
    N = len(table)
    _positive_int("levels_per_batch", levels_per_batch, none_ok=True)
    _float_tensor_or_none("level_noise", level_noise, (N, B, L, 128), f"[N, B, L, 128] = [{N}, {B}, {L}, 128]")
    weights = modality_weight_table(INVERSION_WEIGHTS if modality_weights is None else modality_weights, guidance_scale, N, B, CFG_CHUNKS)
    lib, handle, dev, a, keep = _level_batch_args(denoiser, scheduler, enc, masks, B, L, num_inference_steps, table, seed, first_utterance,
                                                  dedup, row_maps)
    src = source_latents.detach().to(device=dev, dtype=torch.float32).contiguous()
    eps = level_noise.detach().to(device=dev, dtype=torch.float32).contiguous() if level_noise is not None else None
    trajectory = torch.empty((N + 1, B, L, 128), dtype=torch.float32, device=dev)
    noise = torch.empty((N, B, L, 128), dtype=torch.float32, device=dev)
    iv = _lib.DdpmInvertArgs()
    iv.source, iv.weights, iv.prune = src.data_ptr(), weights.ctypes.data_as(C.c_void_p), 1
    iv.level_noise = eps.data_ptr() if eps is not None else None
    iv.trajectory, iv.noise = trajectory.data_ptr(), noise.data_ptr()
    iv.levels_per_batch = int(levels_per_batch or 0)
    iv.workspace_bytes = int(workspace_bytes or 0)
    g_eval, j_used = C.c_int(0), C.c_int(0)
    with torch.cuda.device(dev):
        torch.cuda.current_stream(dev).synchronize()
        _lib.check(lib.cfd_ddpm_invert(handle, C.byref(a), C.byref(iv), C.byref(g_eval), C.byref(j_used),
                                       C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)))
    del keep
    _lib.wrote(trajectory, noise)
    invert_ddpm.last = dict(chunks_evaluated=int(g_eval.value), levels_per_batch=int(j_used.value))
    return trajectory, noise


class ParallelStats:
    """What a ``sample_parallel`` call did: ``sweeps`` level-batched forwards, the window's advance after each (``strides``, summing to the
    iterations of the table), the levels per batch J (``levels_per_batch``) and the guidance chunks evaluated (``chunks_evaluated``)."""

    def __init__(self, sweeps, strides, levels_per_batch, chunks_evaluated):
        self.sweeps, self.strides = int(sweeps), [int(v) for v in strides]
        self.levels_per_batch, self.chunks_evaluated = int(levels_per_batch), int(chunks_evaluated)

    def __repr__(self):
        mean = sum(self.strides) / max(len(self.strides), 1)
        return (f"ParallelStats(sweeps={self.sweeps}, mean stride={mean:.2f}, levels_per_batch={self.levels_per_batch}, "
                f"chunks_evaluated={self.chunks_evaluated})")


def sample_parallel(denoiser, scheduler, enc, masks=None, *, B, L=16, num_inference_steps=1000, tolerance=0.1, levels_per_batch=None,
                    workspace_bytes=None, guidance_scale=7.5, modality_weights=None, init_latents=None, step_noise=None, seed=0,
                    trajectory=False, max_sweeps=None, first_utterance=0, dedup=True, row_maps=None):
    """Parallel-in-time DDPM sampling (ParaDiGMS, Shih et al., NeurIPS 2023; cfd_sample_parallel): Picard sweeps over a sliding window of
    ``levels_per_batch`` consecutive latents of the DDPM chain, each sweep one level-batched forward on split-pair operands (the batch of
    ``invert_ddpm``; None: chosen from ``workspace_bytes``, 4 GiB by default).  ``tolerance`` 0 computes the sequential chain (in at most N
    sweeps); a larger one lets the window slide past levels whose change in a sweep is within tolerance^2 of the step's noise variance per
    element.  ``scheduler``: a ``DDPMScheduler`` (clip_sample honoured); ``enc`` / ``masks``: the 7-chunk guidance batch, as for ``sample``.
    ``modality_weights`` None: the reference's guidance at ``guidance_scale`` (the zero-weight full-conditioning chunk is not evaluated);
    else the weighted combine, as for ``sample``.  ``init_latents`` [B, L, 128] / ``step_noise`` [N, B, L, 128]: as for ``sample``; None: the
    Philox draws ``sample`` makes with the same ``seed``.  Returns (latents [B, L, 128], ParallelStats), and with ``trajectory=True``
    (latents, trajectory [N + 1, B, L, 128], ParallelStats): slot N - i of the trajectory is the latent entering iteration i, slot 0 the
    result.  ``max_sweeps``: None (N, always enough) or a cap; a run that needs more raises ``_lib.CfdError``."""
    if not isinstance(denoiser, Denoiser):
        raise TypeError("denoiser must be a convofusion_amd.denoiser.Denoiser")
    if getattr(scheduler, "KIND", None) != 0:
        raise TypeError("sample_parallel needs a convofusion_amd.scheduler.DDPMScheduler")
    refuse_sample_prediction(scheduler, "sample_parallel (Picard sweeps over level batches) runs")
    _positive_int("B", B)
    _positive_int("L", L)
    B, L = int(B), int(L)
    try:
        tol = float(tolerance)
    except (TypeError, ValueError):
        raise ValueError(f"tolerance must be a finite number >= 0, not {tolerance!r}") from None
    if not (tol >= 0.0) or tol == float("inf"):
        raise ValueError(f"tolerance must be a finite number >= 0, not {tolerance!r}")
    num_inference_steps, table = scheduler.timestep_table(num_inference_steps)
    N = len(table)
    _positive_int("levels_per_batch", levels_per_batch, none_ok=True)
    _positive_int("max_sweeps", max_sweeps, none_ok=True)
    _float_tensor_or_none("init_latents", init_latents, (B, L, 128), [B, L, 128])
    _float_tensor_or_none("step_noise", step_noise, (N, B, L, 128), [N, B, L, 128])
    weights = None if modality_weights is None else modality_weight_table(modality_weights, guidance_scale, N, B, CFG_CHUNKS)
    lib, handle, dev, a, keep = _level_batch_args(denoiser, scheduler, enc, masks, B, L, num_inference_steps, table, seed, first_utterance,
                                                  dedup, row_maps)
    # the default combine, its zero-weight full-conditioning chunk skipped
    a.guidance_weight = (C.c_float * 8)(*default_guidance_weights(CFG_CHUNKS, guidance_scale))
    a.skip_zero_weight_chunks = 1
    init = init_latents.detach().to(device=dev, dtype=torch.float32).contiguous() if init_latents is not None else None
    noise = step_noise.detach().to(device=dev, dtype=torch.float32).contiguous() if step_noise is not None else None
    a.init_latents = init.data_ptr() if init is not None else None
    a.step_noise = noise.data_ptr() if noise is not None else None
    latents = torch.empty((B, L, 128), dtype=torch.float32, device=dev)
    traj = torch.empty((N + 1, B, L, 128), dtype=torch.float32, device=dev) if trajectory else None
    pa = _lib.ParallelArgs()
    pa.weights, pa.prune = (weights.ctypes.data_as(C.c_void_p) if weights is not None else None), 1
    pa.tolerance = tol
    pa.levels_per_batch, pa.workspace_bytes, pa.max_sweeps = int(levels_per_batch or 0), int(workspace_bytes or 0), int(max_sweeps or 0)
    pa.latents, pa.trajectory = latents.data_ptr(), (traj.data_ptr() if traj is not None else None)
    strides = (C.c_int32 * N)()
    ps = _lib.ParallelStats()
    ps.strides, ps.strides_capacity = C.cast(strides, C.c_void_p), N
    with torch.cuda.device(dev):
        torch.cuda.current_stream(dev).synchronize()
        _lib.check(lib.cfd_sample_parallel(handle, C.byref(a), C.byref(pa), C.byref(ps),
                                           C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)))
    del keep
    _lib.wrote(latents, traj)
    stats = ParallelStats(ps.sweeps, strides[:ps.sweeps], ps.levels_per_batch, ps.chunks_evaluated)
    return (latents, traj, stats) if trajectory else (latents, stats)


# the WEG constants diffusion_reverse_forecast hard-codes instead of reading cfg.model.weg_parameters (unbounded_synthesis.py:80-84)
FORECAST_WEG_PARAMETERS = dict(scale_factor=100, scale_range=(1.0, 0.5), max_iter_to_alter=800,
                               thresholds={0: 0.05, 200: 0.4, 400: 0.6, 600: 0.8}, max_refinement_steps=300)


def _loop_from_model(model, encoder_hidden_states, cond_masks, preseq, focus_indices, init_latents, seed, weg_parameters=None,
                     attention=True, operands=None):
    if not model.do_classifier_free_guidance:
        # the reference itself raises NameError here (guidance_bs_mulitplier undefined, convofusion.py:517)
        raise NameError("guidance_bs_mulitplier: the reference loop requires classifier-free guidance")
    G = model.clf_guidance_drops + 1
    bsz = encoder_hidden_states[0].shape[0] // G
    L = 16  # 8 chunks x {body, hands}, convofusion.py:412-416
    dev = encoder_hidden_states[0].device
    if init_latents is None:
        init_latents = torch.randn((bsz, L, model.latent_dim[-1]), device=dev, dtype=torch.float)  # :412-416
    init_latents = init_latents * model.scheduler.init_noise_sigma                                  # :419
    n_steps = model.cfg.model.scheduler.num_inference_timesteps
    model.scheduler.set_timesteps(n_steps)                                                          # :421-422
    eta = 0.0
    if "eta" in set(inspect.signature(model.scheduler.step).parameters.keys()):                    # :427-429
        eta = model.cfg.model.scheduler.eta
    if seed is None:
        seed = int(torch.randint(0, 2 ** 62, (1,)).item())   # per-step noise stream keyed off torch's global generator
    kw = dict(B=bsz, L=L, num_inference_steps=n_steps, guidance_scale=model.guidance_scale, guidance_chunks=G, eta=eta,
              init_latents=init_latents, seed=seed, preseq=preseq,
              # the full-conditioning chunk has guidance weight 0 (convofusion.py:538) and the fused loop keeps no
              # attention maps, so its forward is dead work: identical latents without it
              skip_zero_weight_chunks=True)
    kw["return_attention"] = attention
    kw["operands"] = check_operands(getattr(model, "_cfd_operands", None) if operands is None else operands)
    mw = getattr(model, "_cfd_modality_weights", None)
    if mw is not None:     # install(model, modality_weights=...)
        kw["modality_weights"] = mw
    if len(focus_indices) == 0:
        return sample(model.denoiser, model.scheduler, encoder_hidden_states, cond_masks, **kw)
    # ``weg_parameters`` given = the rollout (its constants are hard-coded and its scale table is fresh every iteration);
    # otherwise ``_diffusion_reverse``, which reads model.weg_parameters and carries the table (convofusion.py:395,442-444)
    return sample_with_weg(model.denoiser, model.scheduler, encoder_hidden_states, cond_masks, focus_indices,
                           weg_parameters if weg_parameters is not None else model.weg_parameters,
                           carry_scale_range=weg_parameters is None, **kw)


def sample_with_weg(denoiser, scheduler, encoder_hidden_states, cond_masks, focus_indices, weg_parameters, *, B, L=16,
                    num_inference_steps=1000, guidance_chunks=CFG_CHUNKS, return_attention=False, carry_scale_range=True, per_row=False,
                    tie=None, weg_stats=None, **kw):
    """The loop with its word-excitation-guidance branch (convofusion.py:437-496): before iteration i the latents are
    moved down the gradient of the attention-focus objective of the text-only chunk (``convofusion_amd.weg``), then the
    captured guided step runs as usual.  ``weg_parameters``: scale_factor, scale_range, max_iter_to_alter, thresholds,
    max_refinement_steps (configs/assets.yaml:18-23).  ``carry_scale_range``: True reproduces ``_diffusion_reverse``, which
    re-assigns its ``scale_range`` table from the previous iteration's first two entries (convofusion.py:442-444: the step
    size stays ~scale_factor after iteration 0); False is the rollout, which takes a fresh 1.0 -> 0.5 table every
    iteration (unbounded_synthesis.py:82-89).  See ``weg.scale_range_schedule``.  ``operands="auto"``, ``modality_weights`` and the edit
    arguments ``source_latents`` / ``keep_mask`` / ``strength`` (in ``kw``): as in ``sample``; an edit's masked overwrite goes in before the
    WEG update (``run.inpaint``), and the WEG schedule is indexed by the full table's iteration.
    ``per_row=True``: every row is its own utterance (``weg.weg_update_rows``, cfd_weg_step) -- its own text slice up to its own EOT,
    its own loss, thresholds test, refinement rounds and closing update, exactly what the row gets alone with B = 1; B >= 1, and the
    run may be tied (``tie``, ``longform``): the objective is evaluated with tied tokens replaced by their sources, their gradients
    are folded onto the sources, and the written latents satisfy the tie.  The rows must fit the row-tile gradient engine
    (``weg.step_refusal``).  ``per_row=False`` is the reference's loop: one loss for the batch, B = 1 (its EOT normalisation asserts
    it); it takes no ``tie``.  ``carry_scale_range`` is one table for the run either way.  ``weg_stats`` (per_row): a list that
    receives, per guided iteration, dict(i, losses, rounds, calls) -- the rows' final losses, their refinement rounds and the
    cfd_weg_step calls of the iteration."""
    if check_operands(kw.get("operands")) == "auto":
        args = dict(locals())
        rest = args.pop("kw")
        return _with_auto_operands(lambda ops: sample_with_weg(**args, **dict(rest, operands=ops)), "auto")
    if kw.get("noise_space") is not None:
        raise NotImplementedError("sample_with_weg: the replay of a noise space (noise_space) takes no word-excitation guidance")
    if getattr(scheduler, "KIND", None) == 3:
        raise NotImplementedError("sample_with_weg: a DDIM inversion (DDIMInverseScheduler) takes no word-excitation guidance -- its latents "
                                  "are its own; use invert() or sample() without focus_indices")
    if getattr(scheduler, "KIND", None) == 2:
        raise NotImplementedError("sample_with_weg: the word-excitation-guidance loop (focus_indices) runs with DDPMScheduler / DDIMScheduler; "
                                  "with DPMSolverMultistepScheduler it has no reference trajectory to be checked against -- use sample() "
                                  "without focus_indices")
    refuse_sample_prediction(scheduler, "sample_with_weg: the word-excitation-guidance loop (focus_indices) runs")
    check_weg_rows(per_row, tie, B, L, [int(m.shape[1]) for m in encoder_hidden_states] if per_row else None)
    from . import weg
    G = guidance_chunks
    scheduler.set_timesteps(num_inference_steps)
    text_states, text_masks = guidance_chunk_rows(encoder_hidden_states, cond_masks, [1], G, B, kw.get("row_maps"))     # :447-448
    text_masks = {k: (v.to(torch.uint8).contiguous() if v is not None else v) for k, v in text_masks.items()}
    thresholds = dict(weg_parameters["thresholds"])
    n_full = len(scheduler.timestep_table(num_inference_steps)[1])      # (an edit run starts at iteration k0 of the table: i counts from there)
    carry = [weg_parameters["scale_range"][0], weg_parameters["scale_range"][1]] if carry_scale_range else None   # :395
    guided = 0                            # evaluations of the objective so far (their conditioning never changes inside the loop)
    if per_row:
        from .denoiser import tie_csr
        dev = encoder_hidden_states[0].device
        tie_dev = None if tie is None else tie.detach().to(device=dev, dtype=torch.int32).contiguous()
        csr = None if tie_dev is None else tie_csr(tie_dev)
        text_states = [m.detach().contiguous() for m in text_states]

    def update(i, t, latents):
        nonlocal guided
        # past max_iter_to_alter the reference still evaluates the objective but only acts on it at a threshold step
        if i >= weg_parameters["max_iter_to_alter"] and i not in thresholds:
            if not any(k > i for k in thresholds):
                return DONE
            if carry is not None:   # the skipped iteration still re-assigns the table (convofusion.py:442-444)
                weg.scale_range_schedule(weg_parameters, n_full, i, carry)
            return None
        if per_row:
            st = {}
            lat, losses = weg.weg_update_rows(denoiser, latents(), i, t, text_states, text_masks, focus_indices, weg_parameters, n_full,
                                              scale_carry=carry, same_memories=guided > 0, tie=tie_dev, csr=csr, stats=st)
            if weg_stats is not None:
                weg_stats.append(dict(i=i, losses=[float(v) for v in losses], **st))
        else:
            lat, _ = weg.weg_update(denoiser, latents(), i, t, text_states, text_masks, focus_indices, weg_parameters, n_full,
                                    scale_carry=carry, same_memories=guided > 0)
        guided += 1
        return lat

    run = _open_run(denoiser, scheduler, encoder_hidden_states, cond_masks, B, L, num_inference_steps, return_attention in ("all", "auto"),
                    guidance_chunks=G, **({} if tie is None else dict(tie=tie)), **kw)
    write = (lambda new: run.write(new, satisfies_tie=True)) if per_row and tie is not None else None
    return _drive(run, denoiser, encoder_hidden_states, cond_masks, G, kw.get("row_maps"), return_attention, update, write)


def guided_chunks(weights):
    """The guidance chunks a combine e_0 + sum_k w_k (e_k - e_0) needs: chunk 0 and every k whose weight is not 0 somewhere in
    ``weights`` [..., 8] (a run's default weights or its table)."""
    import numpy as np
    w = np.asarray(weights, dtype=np.float64).reshape(-1, 8)
    return [0] + [k for k in range(1, 8) if bool((w[:, k] != 0).any())]


def _loss_guidance_step_size(step_size, i, t):
    if callable(step_size):
        return float(step_size(i, t))
    try:
        return float(step_size[i])
    except TypeError:
        return float(step_size)


def _guided_loop_plan(caller, refusal, limit_text, scheduler, encoder_hidden_states, cond_masks, B, L, num_inference_steps, guidance_scale,
                      G, guided_iterations, kw, chunk_columns):
    """What ``caller`` (``sample_with_loss_guidance`` / ``sample_with_keyframes``) sets up before it opens its run: refuses
    ``operands="auto"`` and shapes beyond the call's limit (``refusal``: ``vjp_refusal`` / ``guide_refusal``; ``limit_text``: the
    message, with {n} and {why}), sets the scheduler's timesteps and returns ``chunks``, the evaluated guidance chunks; ``states`` /
    ``masks``, their rows of the memories; ``acp``, the float64 alphas_cumprod on the host; ``guides(i)``, whether iteration i is
    guided; ``weights(i)``, its float32 weight row on the device, [B, 8] or with ``chunk_columns`` the chunks' columns alone [B, n]."""
    from types import SimpleNamespace
    if check_operands(kw.get("operands")) == "auto":
        raise NotImplementedError(f"{caller}: operands='auto' restarts a run whose census trips; give an operand policy")
    n_full = len(scheduler.timestep_table(num_inference_steps)[1])
    mw = kw.get("modality_weights")
    wtab = modality_weight_table(mw, guidance_scale, n_full, B, G) if mw is not None else None      # [n_full, B, 8]
    chunks = guided_chunks(wtab if wtab is not None else default_guidance_weights(G, guidance_scale))
    why = refusal(len(chunks) * B, L, [int(m.shape[1]) for m in encoder_hidden_states])
    if why is not None:
        raise NotImplementedError(f"{caller}: " + limit_text.format(n=len(chunks), why=why))
    guided = None if guided_iterations is None else {int(i) for i in guided_iterations}
    scheduler.set_timesteps(num_inference_steps)
    dev = encoder_hidden_states[0].device
    states, masks = guidance_chunk_rows(encoder_hidden_states, cond_masks, chunks, G, B, kw.get("row_maps"))
    cols = chunks if chunk_columns else list(range(8))
    w_default = torch.tensor(default_guidance_weights(G, guidance_scale), dtype=torch.float32, device=dev)[cols].expand(B, len(cols)).contiguous()
    return SimpleNamespace(
        chunks=chunks, dev=dev, states=[s.detach().contiguous() for s in states], masks=masks,
        acp=scheduler.alphas_cumprod.detach().to("cpu", torch.float64), guides=lambda i: guided is None or i in guided,
        weights=lambda i: torch.from_numpy(wtab[i][:, cols]).to(dev).contiguous() if wtab is not None else w_default)


def _drive_quietly(run, denoiser, encoder_hidden_states, cond_masks, G, row_maps, update, write=None):
    """``_drive`` without attention maps, whatever ``denoiser.return_attention`` says (restored afterwards)."""
    keep_att = denoiser.return_attention
    denoiser.return_attention = False
    try:
        return _drive(run, denoiser, encoder_hidden_states, cond_masks, G, row_maps, False, update, write)
    finally:
        denoiser.return_attention = keep_att


def sample_with_loss_guidance(denoiser, scheduler, encoder_hidden_states, cond_masks, loss_fn, step_size, *, B, L=16,
                              num_inference_steps=1000, guidance_scale=7.5, guidance_chunks=CFG_CHUNKS, guided_iterations=None, **kw):
    """The loop with guidance by any differentiable loss of the predicted clean latents: before iteration i of ``guided_iterations``
    (an iterable of indices into the scheduler's full table; None: every iteration) the latents move by
    -step_size_i * d loss / d latents, then the captured guided step runs as usual (the shape of ``sample_with_weg``).
    loss = loss_fn(x0_hat) with x0_hat = (x - sqrt(1 - acp_t) eps_guided(x)) / sqrt(acp_t); eps_guided is the run's own guidance
    combine e_0 + sum_k w_k (e_k - e_0) (``default_guidance_weights`` or the ``modality_weights`` table) of the chunks whose weight is
    not 0, evaluated through the differentiable ``Denoiser.forward`` on the denoiser's second engine (the run owns the first).
    ``loss_fn``: any torch function [B, L, 128] -> scalar (``edit.keyframe_loss``: soft key-pose constraints).  ``step_size``: a
    number, a sequence indexed by iteration, or a callable (i, t).  With step_size 0 the result is ``sample``'s, bit for bit.
    DDPMScheduler and DDIMScheduler with epsilon prediction; every refusal: ``check_loss_guidance``.  The evaluated chunks times B
    rows must fit the differentiable forward (``denoiser.vjp_refusal``).  Other keywords: as in ``sample`` (no ``operands="auto"``)."""
    from .denoiser import vjp_refusal
    check_loss_guidance(scheduler, noise_space=kw.get("noise_space"), anchor_trajectory=kw.get("anchor_trajectory"), tie=kw.get("tie"))
    if not callable(loss_fn):
        raise TypeError("loss_fn must be a callable [B, L, 128] -> scalar")
    G = guidance_chunks
    p = _guided_loop_plan("sample_with_loss_guidance", vjp_refusal,
                          "the gradient of the {n} evaluated guidance chunks runs on the row-tile path only: {why}", scheduler,
                          encoder_hidden_states, cond_masks, B, L, num_inference_steps, guidance_scale, G, guided_iterations, kw, False)
    chunks = p.chunks

    def update(i, t, latents):
        if not p.guides(i):
            return None
        x = latents().requires_grad_(True)
        w = p.weights(i)      # [B, 8]
        with torch.enable_grad():
            out, _ = denoiser(sample=x.repeat(len(chunks), 1, 1), timestep=int(t), encoder_hidden_states=p.states, mem_mask_dict=p.masks,
                              side_engine=True)
            e = out.view(len(chunks), B, L, out.shape[-1])
            eps = e[0]
            for n, c in enumerate(chunks[1:], start=1):
                eps = eps + w[:, c].view(B, 1, 1) * (e[n] - e[0])
            a_t = float(p.acp[int(t)])
            x0 = (x - (1.0 - a_t) ** 0.5 * eps) / a_t ** 0.5
            loss = loss_fn(x0)
            (g,) = torch.autograd.grad(loss, x)
        # (the side engine ran on torch's current stream, the captured iteration replays on the run's own: ``write`` waits for
        #  the former, so the two never execute side by side)
        return x.detach() - _loss_guidance_step_size(step_size, i, int(t)) * g

    run = _open_run(denoiser, scheduler, encoder_hidden_states, cond_masks, B, L, num_inference_steps, False,
                    guidance_scale=guidance_scale, guidance_chunks=G, **kw)
    return _drive_quietly(run, denoiser, encoder_hidden_states, cond_masks, G, kw.get("row_maps"), update)


def sample_with_keyframes(denoiser, scheduler, encoder_hidden_states, cond_masks, target, mask, step_size, *, B, L=16,
                          num_inference_steps=1000, guidance_scale=7.5, guidance_chunks=CFG_CHUNKS, guided_iterations=None, tie=None, **kw):
    """The loop with key-pose guidance on the device: ``sample_with_loss_guidance`` with ``edit.keyframe_loss(target, mask)`` -- before
    iteration i of ``guided_iterations`` the latents move by -step_size_i * d loss / d latents, loss = the mean-square error of the
    predicted clean latents against ``target`` [B, L, 128] over the tokens of ``mask`` [B, L] -- with the update as ONE
    ``Denoiser.guide`` call (cfd_denoise_guide) per guided iteration on the denoiser's second engine: the run's own guidance combine,
    the loss, the reverse sweep, the sum over the evaluated chunks and the update, with no torch autograd (the loop runs under
    ``torch.inference_mode()``) and with the memory side kept from one guided iteration to the next.  Unlike the torch loop it takes
    a tied run (``tie``, ``longform``): a key token on a tied token pulls its source, and the written latents satisfy the tie.  The
    evaluated chunks times B rows must fit the guide call (``denoiser.guide_refusal``: 4096 token rows, not the differentiable
    forward's 700).  With step_size 0 the result is ``sample``'s, bit for bit.  Every refusal: ``check_keyframe_guidance``.  Other
    keywords: as in ``sample`` (no ``operands="auto"``)."""
    from .denoiser import guide_refusal
    check_keyframe_guidance(scheduler, noise_space=kw.get("noise_space"), anchor_trajectory=kw.get("anchor_trajectory"), tie=tie)
    if not isinstance(target, torch.Tensor) or tuple(target.shape) != (B, L, 128):
        raise ValueError(f"target must be a tensor [B, L, 128] = [{B}, {L}, 128]")
    if not isinstance(mask, torch.Tensor) or tuple(mask.shape) != (B, L):
        raise ValueError(f"mask must be a tensor [B, L] = [{B}, {L}]")
    kept = int((mask != 0).sum().item())
    if kept == 0:
        raise ValueError("sample_with_keyframes: mask keeps no token")

    def guide_call(p):
        tgt = target.detach().to(device=p.dev, dtype=torch.float32).contiguous()
        msk = (mask != 0).to(device=p.dev, dtype=torch.float32).contiguous()
        return lambda x, t, w, **kw_call: denoiser.guide(x, t, p.states, p.masks, w, tgt, msk, inv_n=1.0 / (kept * 128), **kw_call)[2]
    return _device_guided_loop("sample_with_keyframes", guide_refusal, guide_call, denoiser, scheduler, encoder_hidden_states, cond_masks, step_size,
                               B, L, num_inference_steps, guidance_scale, guidance_chunks, guided_iterations, tie, kw)


def _device_guided_loop(caller, refusal, guide_call, denoiser, scheduler, encoder_hidden_states, cond_masks, step_size, B, L, num_inference_steps,
                        guidance_scale, G, guided_iterations, tie, kw):
    """The loop of ``sample_with_keyframes`` and ``sample_with_pose_keyframes`` behind their argument checks: the plan, the tie and its
    inverse table once, one guide call per guided iteration on the denoiser's second engine under ``torch.inference_mode()`` --
    ``guide_call(plan)`` returns the function (x, t, w, **keywords of Denoiser.guide) -> x_new -- with the memory side kept from one
    guided iteration to the next, and the write that states that the latents satisfy the tie."""
    from .denoiser import tie_csr
    with torch.inference_mode():
        p = _guided_loop_plan(caller, refusal, "the guided update of the {n} evaluated guidance chunks: {why}",
                              scheduler, encoder_hidden_states, cond_masks, B, L, num_inference_steps, guidance_scale, G,
                              guided_iterations, kw, True)
        call = guide_call(p)
        tie_dev = None if tie is None else tie.detach().to(device=p.dev, dtype=torch.int32).contiguous()
        csr = None if tie_dev is None else tie_csr(tie_dev)
        calls = 0

        def update(i, t, latents):
            nonlocal calls
            if not p.guides(i):
                return None
            x = latents()
            a_t = float(p.acp[int(t)])
            # (the side engine runs on its own stream behind torch's current one and returns complete; ``write`` then waits for
            #  the current stream, so the update and the captured iteration never execute side by side)
            x_new = call(x, int(t), p.weights(i), sqrt_acp=a_t ** 0.5, sqrt_1m_acp=(1.0 - a_t) ** 0.5,
                         step=_loss_guidance_step_size(step_size, i, int(t)), tie=tie_dev, csr=csr, side_engine=True,
                         reuse_memory_side=2 if calls else 0, want=("x_new",), x_new=x)
            calls += 1
            return x_new

        run = _open_run(denoiser, scheduler, encoder_hidden_states, cond_masks, B, L, num_inference_steps, False,
                        guidance_scale=guidance_scale, guidance_chunks=G, tie=tie, **kw)
        lat = _drive_quietly(run, denoiser, encoder_hidden_states, cond_masks, G, kw.get("row_maps"), update,
                             write=lambda new: run.write(new, satisfies_tie=True))
    return lat.clone()      # (outside inference mode: an ordinary tensor, like ``sample``'s)


def sample_with_pose_keyframes(denoiser, scheduler, encoder_hidden_states, cond_masks, vae, target, frame_mask, step_size, *,
                               feature_mask=None, lengths=None, B, L=16, num_inference_steps=1000, guidance_scale=7.5,
                               guidance_chunks=CFG_CHUNKS, guided_iterations=None, tie=None, **kw):
    """The loop with frame-accurate key poses on the device: ``sample_with_loss_guidance`` with
    ``edit.pose_keyframe_loss(vae, target, frame_mask, feature_mask, lengths)`` -- loss = the mean-square error of the DECODED predicted
    clean latents against ``target`` [B, F, 189] (decode's own, root-subtracted space) over the frames of ``frame_mask`` [B, F] and the
    features of ``feature_mask`` [189] (None: all) -- with the update as ONE ``Denoiser.guide_pose`` call (cfd_denoise_guide_pose) per
    guided iteration: the denoiser's saved forward, x0 in the decoder's layout, the saving decode, the loss, the decoder's sweep, the
    denoiser's sweep and the update on one stream, with no torch autograd and no host round trip.  ``vae``: the
    ``convofusion_amd.vae.ConvoFusionVae`` whose decoder it is.  ``lengths``: frames per row (None: F each; the largest must be F);
    F <= 8 L.  Like ``sample_with_keyframes`` and unlike the torch loop it takes a tied run (``tie``, ``longform``) and
    ``denoiser.guide_refusal``'s 4096 token rows; every other keyword, the refusals (``check_keyframe_guidance``,
    ``denoiser.guide_pose_refusal``) and the bit-for-bit ``sample`` at step_size 0 are that loop's."""
    from .denoiser import guide_pose_refusal
    check_keyframe_guidance(scheduler, noise_space=kw.get("noise_space"), anchor_trajectory=kw.get("anchor_trajectory"), tie=tie)
    Bt, F, _, fm, cm, lens, n_sel = check_pose_keyframes("sample_with_pose_keyframes", target, frame_mask, feature_mask, lengths)
    if Bt != B:
        raise ValueError(f"sample_with_pose_keyframes: target must be [B, F, nfeats] with B = {B}, got {tuple(target.shape)}")
    decoder = dict(latent_dim=vae.latent_dim, num_heads=vae.num_heads, ff_size=vae.ff_size, num_layers=vae.num_layers, latent_size=vae.latent_size)

    def guide_call(p):
        tgt = target.detach().to(device=p.dev, dtype=torch.float32).contiguous()
        fmask, cmask = fm.to(device=p.dev, dtype=torch.float32).contiguous(), cm.to(device=p.dev, dtype=torch.float32).contiguous()
        lens_t = torch.tensor(lens, dtype=torch.int32)
        return lambda x, t, w, **kw_call: denoiser.guide_pose(x, t, p.states, p.masks, w, vae, tgt, fmask, feature_mask=cmask, lengths=lens_t,
                                                              inv_n=1.0 / n_sel, **kw_call)[2]
    return _device_guided_loop("sample_with_pose_keyframes", lambda Be, L_, S: guide_pose_refusal(Be, L_, S, B, F, **decoder), guide_call, denoiser,
                               scheduler, encoder_hidden_states, cond_masks, step_size, B, L, num_inference_steps, guidance_scale,
                               guidance_chunks, guided_iterations, tie, kw)


def diffusion_reverse(model, encoder_hidden_states, lengths=None, cond_masks=dict(), focus_indices=[], *,
                      init_latents=None, seed=None, attention_steps="last"):
    """``Convofusion._diffusion_reverse(self, encoder_hidden_states, lengths, cond_masks, focus_indices)``
    with ``self`` passed as ``model`` (reads model.denoiser / scheduler / cfg / guidance_scale /
    clf_guidance_drops / latent_dim / do_classifier_free_guidance exactly like the reference).
    Returns (latents [L, B, 128], attention_matrices dict).  The reference fills the dict with the full-conditioning
    chunk's ``att_mats`` of EVERY iteration (1000 x 5 tensors kept alive, written out as att_<t>.npy by base.py:252-259);
    ``attention_steps="last"`` keeps the last iteration's entry only: {t_last: att_mats} (``last_step_attention``);
    ``"all"`` fills the whole dict like the reference -- the captured iteration stores the maps itself (cfd_sample_args.att_ring: +2 - 5 %
    run time) while the ring fits ATT_RING_MAX_BYTES, otherwise at the price of one extra forward of the B full-conditioning rows and
    one host round trip per iteration; ``"auto"`` (what ``convofusion_amd.install`` binds by default) is "all" where the captured
    iteration keeps the maps and "last" elsewhere."""
    if attention_steps not in ("last", "all", "auto"):
        raise ValueError("attention_steps must be 'auto', 'last' or 'all'")
    last = attention_steps == "last"
    lat, atts = _loop_from_model(model, encoder_hidden_states, cond_masks, None, focus_indices, init_latents, seed, attention=last or attention_steps)
    return lat.permute(1, 0, 2), ({int(model.scheduler.timesteps[-1]): atts} if last else atts)   # :523,548-549


def diffusion_reverse_forecast(model, encoder_hidden_states, lengths=None, preseq=None, cond_masks=dict(),
                               focus_indices=[], *, init_latents=None, seed=None):
    """``unbounded_synthesis.diffusion_reverse_forecast`` (reference unbounded_synthesis.py:28-187): the same
    loop with the first ``preseq.shape[1]`` tokens re-noised from the previous window every step (:70-76).
    Returns (latents [L, B, 128], att_mats of the last iteration's full-conditioning chunk) like the reference (:159,187)."""
    lat, att = _loop_from_model(model, encoder_hidden_states, cond_masks, preseq, focus_indices, init_latents, seed,
                                weg_parameters=FORECAST_WEG_PARAMETERS)
    return lat.permute(1, 0, 2), att
