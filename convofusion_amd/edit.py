"""Motion editing with the fused loop: token-masked in-painting and img2img strength (``SamplingRun(source_latents=, keep_mask=,
strength=)``, cfd_sample_begin_edit).

The loop's 16 latent tokens are 8 time chunks x {body, hands}: token 2c + p is 16-frame chunk c, part p (the reference's reshape of the
loop's latents into the VAE's [2, B, T, 128], convofusion.py:1028-1030), and frame f of a 128-frame window lies in chunk f // 16.  One
[B, L] keep mask therefore selects time spans, body parts or both:

    keep the body, regenerate the hands   token_mask(B, keep_parts=("body",))
    in-betweening                         token_mask(B, keep_frames=[(0, 32), (96, 128)])
    variation of the whole gesture        no mask, strength 0.5

``keyframe_loss`` (latent tokens) and ``pose_keyframe_loss`` (motion features of single frames, through the differentiable VAE decode) are
the soft constraints of ``sampler.sample_with_loss_guidance``.

``edit_motion`` runs the whole edit: HIP ``encode`` of the source motion, the fused edit loop, HIP ``decode``.

``reperform_motion`` re-conditions a recorded motion ("the same gesture, re-performed to new speech"): deterministic DDIM inversion of its
latents under the source conditioning (``sampler.invert``), then a DDIM regeneration from the inverted noise under the target
conditioning, with the kept tokens anchored to the inversion's trajectory.  Whether re-performed motions look right under a trained
checkpoint is not measured here: the weights of the tests are seeded.
"""
import inspect

import torch

from .run_kind import check_pose_keyframes
from .sampler import check_operands, invert, refuse_sample_prediction, sample
from .vae import LATENT_PARTS

FRAMES_PER_CHUNK = 16   # vae.py:178


def part_index(part):
    """Index p of a body part on the VAE latent's first axis, which is also its place in a token pair (token 2c + p)."""
    if part not in LATENT_PARTS:
        raise ValueError(f"unknown body part {part!r} (known: {', '.join(LATENT_PARTS)})")
    return LATENT_PARTS.index(part)


def token_mask(B, keep_frames=None, keep_parts=("body", "hands"), L=16):
    """bool [B, L] keep mask of the loop's tokens (the same for every utterance; stack or index rows for per-utterance masks).
    keep_frames: None (every frame) or half-open frame spans [(start, stop), ...] within the L / 2 * 16 frames of the window; a chunk is
    kept when a span covers any of its frames (masks are not finer than a 16-frame chunk).  keep_parts: the parts kept in those chunks."""
    if L < 2 or L % 2:
        raise ValueError(f"L = {L}: the loop's tokens come in (body, hands) pairs")
    T = L // 2
    parts = [keep_parts] if isinstance(keep_parts, str) else list(keep_parts)
    chunks = torch.zeros(T, dtype=torch.bool)
    if keep_frames is None:
        chunks[:] = True
    else:
        for span in keep_frames:
            try:
                start, stop = (int(v) for v in span)
            except (TypeError, ValueError):
                raise ValueError(f"keep_frames: {span!r} is not a (start, stop) frame span") from None
            if not 0 <= start < stop <= T * FRAMES_PER_CHUNK:
                raise ValueError(f"keep_frames: span ({start}, {stop}) is not inside the window's {T * FRAMES_PER_CHUNK} frames")
            chunks[start // FRAMES_PER_CHUNK:(stop - 1) // FRAMES_PER_CHUNK + 1] = True
    mask = torch.zeros(T, 2, dtype=torch.bool)
    for part in parts:
        mask[:, part_index(part)] = chunks
    return mask.reshape(1, L).expand(int(B), L).clone()


def keyframe_loss(target, mask):
    """The loss of soft key-pose constraints for ``sampler.sample_with_loss_guidance``: a function x0 [B, L, 128] -> the mean-square
    error against ``target`` [B, L, 128] over the tokens of ``mask`` (bool / 0-1 [B, L], e.g. ``token_mask``).  Where ``edit_motion``
    REPLACES the kept tokens every iteration, the guided loop pulls the predicted clean latents towards them and leaves the denoiser
    free to reconcile the rest."""
    m = (mask != 0)
    n = int(m.sum().item()) * int(target.shape[-1])
    if tuple(m.shape) != tuple(target.shape[:2]) or n == 0:
        raise ValueError("keyframe_loss: mask must be [B, L] like target [B, L, 128] and keep at least one token")

    def loss(x0):
        w = m.to(device=x0.device, dtype=x0.dtype).unsqueeze(-1)
        d = (x0 - target.to(device=x0.device, dtype=x0.dtype)) * w
        return (d * d).sum() / n
    return loss


def pose_keyframe_loss(vae, target, frame_mask, feature_mask=None, lengths=None, fused=False):
    """The loss of frame-accurate key poses for ``sampler.sample_with_loss_guidance``: a function x0 [B, L, 128] -> the mean-square error
    of ``vae.decode(loop_to_vae(x0), lengths)`` against ``target`` [B, F, 189] over the frames of ``frame_mask`` (bool / 0-1 [B, F]) and
    the features of ``feature_mask`` (bool / 0-1 [189]; None = all).  Where ``keyframe_loss`` compares latent tokens (16-frame chunks of
    body or hands), this one constrains motion space: this wrist, these fingers, at frame 73.  ``target`` lives in decode's own feature
    space: the root-subtracted features ``vae.encode`` returns as its third value, not the raw input features.  ``lengths``: frames per
    sequence (default F for every sequence; max(lengths) must be F).  ``vae``: a ``convofusion_amd.vae.ConvoFusionVae`` (its ``decode``
    is differentiable with respect to the latents, backward ``decode_vjp``); decode runs on the stand-alone engine handle, not on the
    denoiser's, so an open sampling run is untouched.  Frames at or beyond a sequence's length decode to 0 and pull nothing.  Whether
    guided motions look right under a trained checkpoint is not measured here: the weights of the tests are seeded.  fused=True:
    ``vae.decode(..., fused=True)`` -- the forward is kept and the backward is the sweep alone, at the fused forward's bits."""
    B, F, nf, fm, cm, lens, n = check_pose_keyframes("pose_keyframe_loss", target, frame_mask, feature_mask, lengths)

    def loss(x0):
        if x0.dim() != 3 or x0.shape[0] != B:
            raise ValueError(f"pose_keyframe_loss: x0 must be [{B}, L, 128], got {tuple(x0.shape)}")
        feats = _decode(vae, loop_to_vae(x0), lens, fused)
        w = (fm.to(x0.device).unsqueeze(-1) & cm.to(x0.device)).to(feats.dtype)
        d = (feats - target.to(device=x0.device, dtype=feats.dtype)) * w
        return (d * d).sum() / n
    return loss


def _decode(vae, z, lengths, fused):
    """``vae.decode(z, lengths)``, with ``fused=True`` handed on only where it is asked for (the default call is the one it always was)."""
    return vae.decode(z, lengths, fused=True) if fused else vae.decode(z, lengths)


def vae_to_loop(z):
    """VAE latent [2, B, T, D] (body | hands) -> loop latents [B, 2T, D]: the reference's permute(1, 2, 0, 3) (convofusion.py:725) and
    reshape(bs, t * bh, dim) (:558)."""
    two, B, T, D = z.shape
    return z.permute(1, 2, 0, 3).reshape(B, T * two, D)


def loop_to_vae(z):
    """Loop latents [B, L, D] -> VAE latent [2, B, L / 2, D]: the reference's permute(1, 0, 2) (convofusion.py:548), then
    reshape(ntokens // 2, 2, bs, dim) and permute(1, 2, 0, 3) (:1027-1030)."""
    z = z.permute(1, 0, 2)
    ntokens, bs, dim = z.shape
    return z.reshape(ntokens // 2, 2, bs, dim).permute(1, 2, 0, 3)


def edit_motion(model, feats, lengths, encoder_hidden_states, cond_masks=None, *, keep_mask=None, strength=1.0, seed=0,
                sample_posterior=False, modality_weights=None, operands=None, fused_decode=False):
    """Edit motions with the fused loop.  ``model``: a Convofusion-like object (reads vae / denoiser / scheduler / cfg / guidance_scale /
    clf_guidance_drops / do_classifier_free_guidance as ``sampler.diffusion_reverse`` does); ``model.vae`` encodes and decodes on the HIP
    path (``convofusion_amd.vae.ConvoFusionVae``, or a reference module after ``attach_hip_encode`` / ``attach_hip_decode``).
    feats [B, nframes, 189], lengths: the source motions; encoder_hidden_states / cond_masks: the guidance batch as for the loop.
    The source latents are the posterior mean (``sample_posterior=True``: encode's draw from the default generator), the loop's initial
    noise and step noise come from Philox with ``seed``; keep_mask [B, nframes / 8] (``token_mask``), strength, modality_weights, operands:
    as in ``sampler.sample``; fused_decode: the final decode as ``decode(..., fused=True)``.
    Returns (features [B, nframes, 189], loop latents [B, nframes / 8, 128])."""
    if not model.do_classifier_free_guidance:
        raise NameError("guidance_bs_mulitplier: the reference loop requires classifier-free guidance")
    latent, dist, _ = model.vae.encode(feats, lengths)
    z = latent if sample_posterior else dist.mean.reshape(latent.shape)
    source = vae_to_loop(z)
    B, L = int(source.shape[0]), int(source.shape[1])
    G = model.clf_guidance_drops + 1
    if encoder_hidden_states[0].shape[0] != G * B:
        raise ValueError(f"the guidance batch has {encoder_hidden_states[0].shape[0]} rows for {B} motions and {G} chunks")
    sch = model.scheduler
    eta = 0.0
    if "eta" in set(inspect.signature(sch.step).parameters.keys()):          # convofusion.py:427-429
        eta = model.cfg.model.scheduler.eta
    if modality_weights is None:
        modality_weights = getattr(model, "_cfd_modality_weights", None)
    lat = sample(model.denoiser, sch, encoder_hidden_states, cond_masks, B=B, L=L,
                 num_inference_steps=model.cfg.model.scheduler.num_inference_timesteps, guidance_scale=model.guidance_scale,
                 guidance_chunks=G, eta=eta, seed=seed, skip_zero_weight_chunks=True,
                 operands=check_operands(getattr(model, "_cfd_operands", None) if operands is None else operands),
                 modality_weights=modality_weights, source_latents=source, keep_mask=keep_mask, strength=strength)
    out = _decode(model.vae, loop_to_vae(lat), lengths, fused_decode)
    return out, lat


def reperform_motion(model, feats, lengths, source_conditioning, target_conditioning, *, source_masks=None, target_masks=None,
                     num_inference_steps=50, keep_mask=None, inversion_weights=None, modality_weights=None, operands=None,
                     method="ddim", strength=1.0, seed=0, levels_per_batch=None, fused_decode=False):
    """Re-perform motions under new conditioning.  ``model`` / ``feats`` / ``lengths``: as in ``edit_motion``; source_conditioning /
    target_conditioning (+ their masks): the 7-chunk guidance batches of the recorded motion's conditioning and of the new one.
      1. HIP encode of the source to its posterior mean (loop layout);
      2. DDIM inversion under the source conditioning (``sampler.invert``, N = num_inference_steps): ``inversion_weights`` None inverts with
         the conditional prediction alone (guidance_scale 1), otherwise with those weights at model.guidance_scale;
      3. DDIM regeneration (a DDIMScheduler with the model scheduler's betas, set_alpha_to_one and steps_offset; eta 0, no clipping) from
         the inverted latents under the target conditioning at model.guidance_scale with ``modality_weights`` (None: the model's installed
         weights, else the reference's); the tokens of ``keep_mask`` [B, L] are anchored to the inversion's trajectory;
      4. HIP decode (fused_decode=True: ``decode(..., fused=True)``).
    Returns (features [B, nframes, 189], loop latents [B, L, 128], inverted latents [B, L, 128]).
    ``method="ddpm"``: the edit-friendly DDPM noise space instead, with the model's OWN scheduler (DDPM, clip_sample as configured) and
    its own step count (cfg.model.scheduler.num_inference_timesteps; num_inference_steps is not used): ``sampler.invert_ddpm`` under the
    source conditioning (``seed`` keys the level draws, ``levels_per_batch`` as there), then the replay under the target conditioning with
    ``keep_mask`` / ``strength`` (``sample(..., noise_space=)``, split-pair operands).  The third return value is then the noisiest level,
    trajectory[N].  Under the source conditioning the replay reproduces the source up to the last step, which adds no noise and returns
    the model's own x0 estimate.  ``method="ddim"`` (the default) is unchanged."""
    from .scheduler import DDIMInverseScheduler, DDIMScheduler
    if method not in ("ddim", "ddpm"):
        raise ValueError(f"method must be 'ddim' or 'ddpm', not {method!r}")
    refuse_sample_prediction(model.scheduler, "reperform_motion (inversion and regeneration) runs")
    if not model.do_classifier_free_guidance:
        raise NameError("guidance_bs_mulitplier: the reference loop requires classifier-free guidance")
    latent, dist, _ = model.vae.encode(feats, lengths)
    source = vae_to_loop(dist.mean.reshape(latent.shape))
    B, L = int(source.shape[0]), int(source.shape[1])
    G = model.clf_guidance_drops + 1
    for name, cond in (("source_conditioning", source_conditioning), ("target_conditioning", target_conditioning)):
        if cond[0].shape[0] != G * B:
            raise ValueError(f"{name} has {cond[0].shape[0]} rows for {B} motions and {G} chunks")
    sch = model.scheduler
    if method == "ddpm":
        from .sampler import invert_ddpm
        if getattr(sch, "KIND", None) != 0:
            raise TypeError("reperform_motion(method='ddpm') needs the model's scheduler to be a convofusion_amd.scheduler.DDPMScheduler")
        n = model.cfg.model.scheduler.num_inference_timesteps
        space = invert_ddpm(model.denoiser, sch, source_conditioning, source_masks, source_latents=source, num_inference_steps=n,
                            guidance_scale=1.0 if inversion_weights is None else model.guidance_scale, modality_weights=inversion_weights,
                            seed=seed, levels_per_batch=levels_per_batch)
        if modality_weights is None:
            modality_weights = getattr(model, "_cfd_modality_weights", None)
        lat = sample(model.denoiser, sch, target_conditioning, target_masks, B=B, L=L, num_inference_steps=n,
                     guidance_scale=model.guidance_scale, guidance_chunks=G, skip_zero_weight_chunks=True, operands=operands,
                     modality_weights=modality_weights, noise_space=space, keep_mask=keep_mask, strength=strength)
        return _decode(model.vae, loop_to_vae(lat), lengths, fused_decode), lat, space[0][-1]
    if float(strength) != 1.0:
        raise ValueError("strength belongs to method='ddpm' (the DDIM path regenerates from the fully inverted latents)")
    kw = dict(num_train_timesteps=sch.config.num_train_timesteps, trained_betas=sch.betas.tolist(), clip_sample=False,
              set_alpha_to_one=sch.config.get("set_alpha_to_one", True), steps_offset=sch.config.get("steps_offset", 0))
    ops = check_operands(getattr(model, "_cfd_operands", None) if operands is None else operands)
    anchored = keep_mask is not None
    inv = invert(model.denoiser, DDIMInverseScheduler(**kw), source_conditioning, source_masks, source_latents=source,
                 num_inference_steps=num_inference_steps, guidance_scale=1.0 if inversion_weights is None else model.guidance_scale,
                 modality_weights=inversion_weights, return_trajectory=anchored, operands=ops)
    inverted, traj = inv if anchored else (inv, None)
    if modality_weights is None:
        modality_weights = getattr(model, "_cfd_modality_weights", None)
    lat = sample(model.denoiser, DDIMScheduler(**kw), target_conditioning, target_masks, B=B, L=L, num_inference_steps=num_inference_steps,
                 guidance_scale=model.guidance_scale, guidance_chunks=G, eta=0.0, init_latents=inverted, skip_zero_weight_chunks=True,
                 operands=ops, modality_weights=modality_weights, anchor_trajectory=traj, keep_mask=keep_mask)
    out = _decode(model.vae, loop_to_vae(lat), lengths, fused_decode)
    return out, lat, inverted
