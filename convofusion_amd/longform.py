"""Long-form synthesis with the fused loop: the half-overlapping 128-frame windows of an utterance as rows of ONE tied run
(``SamplingRun(tie=)``, cfd_sample_begin_tied).

The reference makes a motion longer than one window with its rollout (unbounded_synthesis.py:244-512): 2 * parts - 1 half-overlapping
windows, one full sampling run after another, each in-painting its first 8 tokens (``preseq``) from the finished last 8 of the window
before.  Here all windows of an utterance are rows of one batch at the same noise level, and the first half of window w is *tied* to the
second half of window w - 1: at the start of every iteration (and once more after the last) those tokens take the value the previous
window's tokens have at that moment.  The tie is causal -- window w - 1 never reads window w -- and replaces the tokens rather than
averaging them: the synchronous form of the rollout's ``preseq`` in-painting (batched long-form schemes of this kind: PriorMDM's
DoubleTake for motion, Gen-L-Video for video).  It is NOT a reference feature, and whether tied windows look right under a trained
checkpoint is not measured here: the weights of the tests are seeded.

Rows are ordered utterance-major: row u * W + w is window w of utterance u, and that global index is also the row's Philox stream, so a
window draws the same noise whichever run it lands in.  The loop's 16 tokens are 8 time chunks x {body, hands} (token 2c + p,
``convofusion_amd.edit``): the first L / 2 tokens of a window are its first 4 chunks (64 frames), body and hands.

Grouping (``max_rows``) is part of the call's meaning, not a tuning knob.  Windows that share a run are tied (both still noisy, denoised
together); the first window of a later run *keeps* its first half from the finished second half of the window before it, re-noised every
iteration through the edit instance's ``keep`` / ``source`` -- the reference's ``preseq`` in-painting per row, without the rollout's
noise-aliasing quirk.  One run of all windows is the tied scheme, runs of one window are a rollout in the reference's manner, anything
between mixes the two, and the three give different motions.
"""
import inspect

import torch

from .distributed import shard_cfg_batch, shard_modality_weights
from .edit import _decode, loop_to_vae
from .sampler import CFG_CHUNKS, check_operands, sample, sample_with_keyframes, sample_with_pose_keyframes, sample_with_weg

WINDOW_FRAMES = 128     # unbounded_synthesis.py:272 (motion_len)


def window_ties(n_utterances, n_windows, L=16):
    """The tie table [U * W, L] (int32) of U utterances x W half-overlapping windows: token l < L / 2 of row u * W + w, w > 0, is tied to
    token l + L / 2 of row u * W + w - 1; every other entry is -1 (W = 1: all of them)."""
    U, W, L = int(n_utterances), int(n_windows), int(L)
    if U < 1 or W < 1 or L < 2 or L % 2:
        raise ValueError(f"window_ties: need n_utterances >= 1, n_windows >= 1 and an even L >= 2 (got {U}, {W}, {L})")
    tie = torch.full((U, W, L), -1, dtype=torch.int32)
    rows = torch.arange(U * W, dtype=torch.int32).reshape(U, W)
    half = torch.arange(L // 2, dtype=torch.int32)
    tie[:, 1:, :L // 2] = (rows[:, :-1, None] * L + half + L // 2)
    return tie.reshape(U * W, L)


def window_groups(n_utterances, n_windows, max_rows=None):
    """The runs of a long-form synthesis as half-open ranges [start, stop) of global rows (row u * W + w), each contiguous so that the run's
    ``first_utterance`` = start gives every row its global Philox stream.  max_rows None or >= U * W: one run.  max_rows >= W: whole
    utterances, max_rows // W of them per run (utterances are independent: nothing is carried).  max_rows < W: every utterance on its own,
    in groups of max_rows consecutive windows (the first window of a later group keeps its first half from the group before)."""
    U, W = int(n_utterances), int(n_windows)
    if max_rows is None or int(max_rows) >= U * W:
        return [(0, U * W)]
    m = int(max_rows)
    if m < 1:
        raise ValueError(f"max_rows = {max_rows!r} must be at least 1")
    if m >= W:
        k = m // W
        return [(u * W, min(u + k, U) * W) for u in range(0, U, k)]
    return [(u * W + w, u * W + min(w + m, W)) for u in range(U) for w in range(0, W, m)]


def group_ties(start, stop, n_windows, L=16):
    """The tie table [stop - start, L] of the run over global rows [start, stop), numbered inside the run, and the bool [stop - start, L]
    mask of the tokens whose source window lies before the run: those are kept from the finished window instead (``synthesize_latents``)."""
    rows = torch.arange(start, stop)
    tie = torch.full((stop - start, L), -1, dtype=torch.int32)
    carried = torch.zeros((stop - start, L), dtype=torch.bool)
    later = rows % n_windows > 0
    inside = later & (rows - 1 >= start)
    half = torch.arange(L // 2)
    tie[inside, :L // 2] = ((rows[inside] - 1 - start)[:, None] * L + half + L // 2).to(torch.int32)
    carried[later & ~inside, :L // 2] = True
    return tie, carried


def stitch_tokens(windows):
    """[U, W, L, 128] windows -> the token sequence [U, (W + 1) * L / 2, 128]: window 0 whole, then every later window's second half
    (token t of the sequence is token t of window 0 for t < L, else token L / 2 + (t - L) % (L / 2) of window 1 + (t - L) // (L / 2))."""
    U, W, L, D = windows.shape
    return torch.cat([windows[:, 0], windows[:, 1:, L // 2:].reshape(U, (W - 1) * (L // 2), D)], dim=1)


def synthesize_latents(model_or_denoiser, scheduler, encoder_hidden_states, cond_masks=None, *, n_utterances, n_windows, L=16,
                       num_inference_steps=1000, guidance_scale=7.5, guidance_chunks=CFG_CHUNKS, eta=0.0, seed=0, max_rows=None,
                       carry=None, skip_zero_weight_chunks=True, operands=None, modality_weights=None, keyframes=None,
                       pose_keyframes=None, vae=None, focus_indices=None, weg_parameters=None, carry_scale_range=False):
    """The latents of U = n_utterances motions of W = n_windows half-overlapping windows each.  ``model_or_denoiser``: the HIP ``Denoiser``
    or an object with a ``.denoiser``.  encoder_hidden_states / cond_masks: the guidance batch of ``sample`` for B = U * W rows in the
    order u * W + w (chunk-major, G * B rows per memory), every row conditioned on its own window of the audio and text as the caller
    sliced them (the reference's per-window data work, unbounded_synthesis.py:290-330; ``audio_windows`` does the audio side of it from the
    waveform).  modality_weights: as in ``sample`` over those rows.
    Noise: Philox with ``seed``, row u * W + w on stream u * W + w.
    max_rows: the most rows one run may have (``window_groups``); windows of one run are tied, a later run's first window keeps its first
    half from the finished window before it -- the grouping changes the result.  carry [U, L / 2, 128] (optional): the finished second half
    of the window before window 0 of every utterance (streaming: the previous call's ``windows[:, -1, L // 2:]``); window 0 then keeps
    its first half from it in the same way.
    keyframes (optional): (target [U * W, L, 128], mask [U * W, L], step_size, guided_iterations) in window rows -- soft key poses
    (``sampler.sample_with_keyframes``): every run whose rows hold a key token goes through the key-pose guided loop with the run's tie
    and kept tokens; a key token may fall on a tied token and then pulls its source.  step_size / guided_iterations as in that loop
    (a per-iteration step size or a callable serves every run alike).  None: exactly today's calls.
    pose_keyframes (optional, with ``vae``, the ``ConvoFusionVae`` that decodes): (target [U * W, 8 L, 189], frame_mask [U * W, 8 L],
    feature_mask [189] or None, step_size, guided_iterations) in window rows (``pose_keyframes_for_windows``) -- frame-accurate key poses
    (``sampler.sample_with_pose_keyframes``): every run whose rows hold a selected frame goes through that loop with the run's tie and kept
    tokens.  Not together with ``keyframes``.  None: exactly today's calls.
    focus_indices (optional, with ``weg_parameters``): U * W lists of text positions in window rows, each in its own window's text --
    word-excitation guidance per window (``sampler.sample_with_weg(per_row=True)``): every run whose rows hold a focus token goes
    through that loop with the run's tie and kept tokens, every window its own utterance (its own text slice, loss, refinement rounds);
    a focus word's gradient at a tied token pulls its source.  ``carry_scale_range`` as in that loop (one table per run).  Not together
    with ``keyframes`` or ``pose_keyframes``; a run beyond the row-tile gradient engine's rows raises NotImplementedError: pass
    ``max_rows``.  None, or all lists empty: exactly today's calls.
    Returns (windows [U, W, L, 128], sequence [U, (W + 1) * L / 2, 128] = ``stitch_tokens(windows)``)."""
    denoiser = getattr(model_or_denoiser, "denoiser", model_or_denoiser)
    U, W, L = int(n_utterances), int(n_windows), int(L)
    B, G = U * W, int(guidance_chunks)
    window_ties(U, W, L)      # (checks U, W, L)
    if encoder_hidden_states[0].shape[0] != G * B:
        raise ValueError(f"the guidance batch has {encoder_hidden_states[0].shape[0]} rows for {U} utterances x {W} windows and {G} chunks")
    if carry is not None and tuple(carry.shape) != (U, L // 2, 128):
        raise ValueError(f"carry must be [U, L / 2, 128] = [{U}, {L // 2}, 128], not {list(carry.shape)}")
    operands = check_operands(operands)
    dev = encoder_hidden_states[0].device
    if keyframes is not None:
        try:
            kf_target, kf_mask, kf_step, kf_iterations = keyframes
        except (TypeError, ValueError):
            raise ValueError("keyframes must be (target [U * W, L, 128], mask [U * W, L], step_size, guided_iterations)") from None
        if not isinstance(kf_target, torch.Tensor) or tuple(kf_target.shape) != (B, L, 128):
            raise ValueError(f"keyframes: target must be [U * W, L, 128] = [{B}, {L}, 128]")
        if not isinstance(kf_mask, torch.Tensor) or tuple(kf_mask.shape) != (B, L):
            raise ValueError(f"keyframes: mask must be [U * W, L] = [{B}, {L}]")
    if pose_keyframes is not None:
        if keyframes is not None:
            raise ValueError("keyframes and pose_keyframes cannot be combined: one guided update serves one loss")
        if vae is None:
            raise ValueError("pose_keyframes needs vae=, the ConvoFusionVae whose decoder the loss runs through")
        try:
            pk_target, pk_frames, pk_features, pk_step, pk_iterations = pose_keyframes
        except (TypeError, ValueError):
            raise ValueError("pose_keyframes must be (target [U * W, 8 L, 189], frame_mask [U * W, 8 L], feature_mask or None, step_size, "
                             "guided_iterations)") from None
        if not isinstance(pk_target, torch.Tensor) or pk_target.dim() != 3 or tuple(pk_target.shape[:2]) != (B, 8 * L):
            raise ValueError(f"pose_keyframes: target must be [U * W, 8 L, nfeats] = [{B}, {8 * L}, nfeats]")
        if not isinstance(pk_frames, torch.Tensor) or tuple(pk_frames.shape) != (B, 8 * L):
            raise ValueError(f"pose_keyframes: frame_mask must be [U * W, 8 L] = [{B}, {8 * L}]")
    if focus_indices is not None:
        if keyframes is not None or pose_keyframes is not None:
            raise ValueError("focus_indices and keyframes / pose_keyframes cannot be combined: one guided update serves one loss")
        if len(focus_indices) != B:
            raise ValueError(f"focus_indices must be U * W = {B} lists of text positions in window rows, not {len(focus_indices)}")
        focus_indices = [[int(i) for i in row] for row in focus_indices]
        if not any(focus_indices):
            focus_indices = None
        elif weg_parameters is None:
            raise ValueError("focus_indices needs weg_parameters= (scale_factor, scale_range, max_iter_to_alter, thresholds, "
                             "max_refinement_steps)")
    groups = window_groups(U, W, max_rows)
    if focus_indices is not None:
        from .weg import step_refusal
        for start, stop in groups:
            why = step_refusal(stop - start, L, [int(m.shape[1]) for m in encoder_hidden_states]) if any(focus_indices[start:stop]) else None
            if why is not None:
                raise NotImplementedError(f"synthesize_latents: the run of window rows {start} .. {stop - 1} holds focus words, and per-row "
                                          f"word-excitation guidance runs on the row-tile gradient engine only: {why}; pass max_rows= to "
                                          "split the windows into smaller runs")
    out = torch.empty((B, L, 128), dtype=torch.float32, device=dev)
    for start, stop in groups:
        n = stop - start
        tie, carried = group_ties(start, stop, W, L)
        src = keep = None
        for b in range(n):
            u, w = divmod(start + b, W)
            prev = out[start + b - 1, L // 2:] if carried[b].any() else (carry[u] if carry is not None and w == 0 else None)
            if prev is None:
                continue
            if src is None:
                src = torch.zeros((n, L, 128), dtype=torch.float32, device=dev)
                keep = torch.zeros((n, L), dtype=torch.bool, device=dev)
            src[b, :L // 2] = prev.to(device=dev, dtype=torch.float32)
            keep[b, :L // 2] = True
        enc = [shard_cfg_batch(m, start, stop, B, G) for m in encoder_hidden_states]
        masks = {k: shard_cfg_batch(v, start, stop, B, G) for k, v in (cond_masks or {}).items()}
        run_kw = dict(B=n, L=L, num_inference_steps=num_inference_steps, guidance_scale=guidance_scale, guidance_chunks=G, eta=eta, seed=seed,
                      first_utterance=start, skip_zero_weight_chunks=skip_zero_weight_chunks, operands=operands,
                      modality_weights=shard_modality_weights(modality_weights, start, stop, B), source_latents=src, keep_mask=keep,
                      tie=tie.to(dev) if bool((tie >= 0).any()) else None)
        if keyframes is not None and bool((kf_mask[start:stop] != 0).any()):
            out[start:stop] = sample_with_keyframes(denoiser, scheduler, enc, masks, kf_target[start:stop], kf_mask[start:stop], kf_step,
                                                    guided_iterations=kf_iterations, **run_kw)
        elif pose_keyframes is not None and bool((pk_frames[start:stop] != 0).any()):
            out[start:stop] = sample_with_pose_keyframes(denoiser, scheduler, enc, masks, vae, pk_target[start:stop], pk_frames[start:stop],
                                                         pk_step, feature_mask=pk_features, guided_iterations=pk_iterations, **run_kw)
        elif focus_indices is not None and any(focus_indices[start:stop]):
            out[start:stop] = sample_with_weg(denoiser, scheduler, enc, masks, focus_indices[start:stop], weg_parameters, per_row=True,
                                              carry_scale_range=carry_scale_range, **run_kw)
        else:
            out[start:stop] = sample(denoiser, scheduler, enc, masks, **run_kw)
    windows = out.reshape(U, W, L, 128)
    return windows, stitch_tokens(windows)


def audio_windows(front_end, wave, n_windows, normalize=False):
    """The listener-audio side of the per-window data work (unbounded_synthesis.py:279-308) from the waveform, on the device:
    ``front_end`` (``audio.AudioFrontEnd`` with an encoder) makes ONE spectrogram per utterance and the library slices it.
    wave [U, n_parts * window_samples] float32 on the device, n_windows = 2 n_parts - 1; anything else raises ValueError, and so does a
    length whose windows (``audio.window_slices`` / ``audio.activity_slices``) do not all have the same number of frames or bits.
    Returns (audio memory [U * W, frames, latent], activity bits int32 [U * W, bits per window], Mel windows [U * W, frames, n_mels] in dB,
    unconditional audio memory [1, frames, latent] = ``audio.uncond_mel`` through the same encoder), rows in the order u * W + w that
    ``build_guidance_batch`` and ``synthesize_latents`` take.  The text side of that work stays the caller's."""
    from .audio import AudioFrontEnd, activity_slices, frame_count, uncond_mel, window_slices
    if not isinstance(front_end, AudioFrontEnd) or front_end.audio_encoder is None:
        raise ValueError("audio_windows: front_end must be an AudioFrontEnd with an audio_encoder")
    W = int(n_windows)
    if W < 1 or W % 2 == 0:
        raise ValueError(f"audio_windows: n_windows = 2 n_parts - 1 is odd and positive (got {n_windows})")
    n_parts = (W + 1) // 2
    if not isinstance(wave, torch.Tensor) or wave.dim() != 2 or wave.shape[0] < 1 or wave.shape[1] < n_parts or wave.shape[1] % n_parts:
        raise ValueError(f"audio_windows: wave must be [U, n_parts * window_samples] with n_parts = {n_parts}")
    U, n = (int(v) for v in wave.shape)
    mel_sl = window_slices(frame_count(n, front_end.hop_length), n_parts)
    n_bits = n // front_end.act_chunk
    if n_bits < n_parts:
        raise ValueError(f"audio_windows: {n} samples hold {n_bits} activity chunks of {front_end.act_chunk} samples, fewer than {n_parts} parts")
    bit_sl = activity_slices(n_bits, n_parts)
    frames, bits = mel_sl[0][1] - mel_sl[0][0], bit_sl[0][1] - bit_sl[0][0]
    if any(b - a != frames for a, b in mel_sl) or any(b - a != bits for a, b in bit_sl):
        raise ValueError(f"audio_windows: the {W} windows of {n} samples do not all have {frames} Mel frames and {bits} activity bits "
                         f"(frames {mel_sl}, bits {bit_sl})")
    r = front_end.forward(wave, normalize=normalize, windows=([a for a, _ in mel_sl], frames))
    activity = torch.stack([r.activity[:, a:b] for a, b in bit_sl], dim=1).reshape(U * W, bits)
    uncond = front_end.encode_mel(uncond_mel(frames, front_end.n_mels).to(wave.device)[None])
    return r.memory, activity, r.mel, uncond


def pose_keyframes_for_windows(target, frame_mask, n_windows, feature_mask=None):
    """Key poses given on the stitched motion, as window rows for ``pose_keyframes=``: target [U, (W + 1) * 64, nfeats] and frame_mask
    [U, (W + 1) * 64] -> (target [U * W, 128, nfeats], frame_mask [U * W, 128]).  Frame f of the stitched motion goes to the window
    ``stitch_frames`` takes it from: window 0 for f < 128, otherwise window 1 + (f - 128) // 64 at frame 64 + (f - 128) % 64.
    ``stitch_frames`` moves the root x / z translation (features 0 and 2) of every later window by an offset that depends on the result,
    so with W > 1 a ``feature_mask`` (the one the loss will use; None: all features) that selects column 0 or 2 is refused: such targets
    have to be given in the window's own space, as window rows."""
    W, F, H = int(n_windows), WINDOW_FRAMES, WINDOW_FRAMES // 2
    if not isinstance(target, torch.Tensor) or target.dim() != 3 or W < 1 or target.shape[1] != (W + 1) * H:
        raise ValueError(f"pose_keyframes_for_windows: target must be [U, (W + 1) * {H}, nfeats] = [U, {(W + 1) * H}, nfeats]")
    U, _, nf = (int(v) for v in target.shape)
    if not isinstance(frame_mask, torch.Tensor) or tuple(frame_mask.shape) != (U, (W + 1) * H):
        raise ValueError(f"pose_keyframes_for_windows: frame_mask must be [U, (W + 1) * {H}] = [{U}, {(W + 1) * H}]")
    if W > 1:
        cols = torch.ones(nf, dtype=torch.bool) if feature_mask is None else (feature_mask != 0).reshape(-1).cpu()
        if cols.numel() != nf:
            raise ValueError(f"pose_keyframes_for_windows: feature_mask must be [{nf}]")
        if bool(cols[0]) or bool(cols[2]):
            raise ValueError("pose_keyframes_for_windows: the feature mask selects column 0 or 2, the root x / z translation that stitch_frames "
                             "moves in every later window by an offset that depends on the result; give such targets in the window's own "
                             "space (window rows) or leave the two columns out")
    t_rows = torch.zeros((U, W, F, nf), dtype=target.dtype, device=target.device)
    m_rows = torch.zeros((U, W, F), dtype=frame_mask.dtype, device=frame_mask.device)
    t_rows[:, 0], m_rows[:, 0] = target[:, :F], frame_mask[:, :F]
    if W > 1:
        t_rows[:, 1:, H:] = target[:, F:].reshape(U, W - 1, H, nf)
        m_rows[:, 1:, H:] = frame_mask[:, F:].reshape(U, W - 1, H)
    return t_rows.reshape(U * W, F, nf), m_rows.reshape(U * W, F)


def stitch_frames(feats):
    """[U, W, F, nfeats] decoded windows -> [U, (W + 1) * F / 2, nfeats], the reference's frame stitching (unbounded_synthesis.py:460-468):
    window 0 whole; every later window has its root x / z translation (features 0 and 2) moved so that its first frame sits where the
    first frame of the previous (already moved) window's second half does, and contributes its second half."""
    U, W, F, _ = feats.shape
    xz = torch.tensor([1.0, 0.0, 1.0], dtype=feats.dtype, device=feats.device)
    pieces = [feats[:, 0]]
    prev = feats[:, 0, F // 2:]
    for w in range(1, W):
        f = feats[:, w].clone()
        f[:, :, :3] = f[:, :, :3] - f[:, :1, :3] * xz
        f[:, :, :3] = f[:, :, :3] + prev[:, :1, :3] * xz
        prev = f[:, F // 2:]
        pieces.append(prev)
    return torch.cat(pieces, dim=1)


def synthesize_motion(model, encoder_hidden_states, cond_masks=None, *, n_utterances, n_windows, seed=0, max_rows=None, carry=None,
                      modality_weights=None, operands=None, fused_decode=False, keyframes=None, pose_keyframes=None, focus_indices=None,
                      weg_parameters=None, carry_scale_range=False):
    """Long-form motions from a Convofusion-like ``model`` (reads vae / denoiser / scheduler / cfg / guidance_scale / clf_guidance_drops /
    do_classifier_free_guidance as ``edit.edit_motion`` does; ``model.vae`` decodes on the HIP path): ``synthesize_latents``, one HIP
    ``decode`` of all U * W windows (fused_decode=True: ``decode(..., fused=True)``, one forward-only cfd_vae_decode on a workspace of 1.2 MB
    per window), the reference's frame stitching (``stitch_frames``) in torch on the device.  keyframes: soft key poses in latent
    tokens, as in ``synthesize_latents``; pose_keyframes: frame-accurate key poses in window rows (``pose_keyframes_for_windows``), decoded
    through ``model.vae``.  focus_indices / weg_parameters / carry_scale_range: word-excitation guidance per window, as in
    ``synthesize_latents`` (weg_parameters None: ``model.weg_parameters``).
    Returns (features [U, (W + 1) * 64, nfeats], windows [U, W, L, 128], token sequence [U, (W + 1) * L / 2, 128])."""
    if not model.do_classifier_free_guidance:
        raise NameError("guidance_bs_mulitplier: the reference loop requires classifier-free guidance")
    U, W = int(n_utterances), int(n_windows)
    sch = model.scheduler
    eta = 0.0
    if "eta" in set(inspect.signature(sch.step).parameters.keys()):          # convofusion.py:427-429
        eta = model.cfg.model.scheduler.eta
    if modality_weights is None:
        modality_weights = getattr(model, "_cfd_modality_weights", None)
    L = WINDOW_FRAMES // 8
    windows, tokens = synthesize_latents(
        model.denoiser, sch, encoder_hidden_states, cond_masks, n_utterances=U, n_windows=W, L=L,
        num_inference_steps=model.cfg.model.scheduler.num_inference_timesteps, guidance_scale=model.guidance_scale,
        guidance_chunks=model.clf_guidance_drops + 1, eta=eta, seed=seed, max_rows=max_rows, carry=carry,
        operands=getattr(model, "_cfd_operands", None) if operands is None else operands, modality_weights=modality_weights,
        **({} if keyframes is None else dict(keyframes=keyframes)),
        **({} if pose_keyframes is None else dict(pose_keyframes=pose_keyframes, vae=model.vae)),
        **({} if focus_indices is None else dict(focus_indices=focus_indices, carry_scale_range=carry_scale_range,
                                                 weg_parameters=model.weg_parameters if weg_parameters is None else weg_parameters)))
    feats = _decode(model.vae, loop_to_vae(windows.reshape(U * W, L, 128)), [WINDOW_FRAMES] * (U * W), fused_decode)
    return stitch_frames(feats.reshape(U, W, WINDOW_FRAMES, feats.shape[-1])), windows, tokens
