"""Restated loop with tied tokens -- TEST INFRASTRUCTURE (numpy, float32 like the reference).

``tests/edit_ref.edit_reverse`` (token-masked in-painting; its conventions: the scheduler's full table, step noise by full-table iteration
index, the kept tokens re-noised from the run's initial draw at the start of every iteration) with a tie table next to the keep mask: at the
top of every iteration token (b, l) with tie[b, l] = s >= 0 takes the current value of token s = b' * L + l' (what the previous iteration's
scheduler step left there; at iteration 0 its initial noise), before the replication into the guidance batch, and once more after the last
iteration.  Snapshots are the latents as the scheduler step left them (no copy applied), the returned latents have the final copy.  A tied
run starts at iteration 0 (no strength).  With a table of -1 throughout the loop is ``edit_reverse`` with k0 = 0, operation for operation.
"""
import numpy as np

from oracle.sampler_ref import CFG_CHUNKS, cfg_combine
from tests.edit_ref import F32, DpmState, add_noise, dpmpp_step


def check_ties(tie, keep):
    """The table's contract: range, no self-tie, a source is free (not tied, not kept), no token both kept and tied."""
    B, L = tie.shape
    flat, kflat = tie.reshape(-1), keep.reshape(-1)
    for e in np.nonzero(flat != -1)[0]:
        v = int(flat[e])
        assert 0 <= v < B * L and v != e, (e, v)
        assert flat[v] == -1 and not kflat[v] and not kflat[e], (e, v)


def tie_copy(latents, tie):
    """latents with every tied token replaced by its source's value in `latents` (all sources are read before anything is written)."""
    B, L, D = latents.shape
    flat = np.asarray(tie).reshape(-1)
    tied = np.nonzero(flat >= 0)[0]
    out = latents.reshape(B * L, D).copy()
    out[tied] = latents.reshape(B * L, D)[flat[tied]]
    return out.reshape(B, L, D)


def tied_reverse(denoise_fn, scheduler, encoder_hidden_states, cond_masks, init_noise, step_noise, tie, source=None, keep=None,
                 guidance_scale=7.5, num_inference_steps=20, eta=0.0, keep_steps=()):
    """denoise_fn(sample[7B, L, 128], t, enc, masks) -> (eps[7B, L, 128], att).  init_noise: the run's N(0,1) draw [B, L, 128];
    step_noise(i, t): the [B, L, 128] draw of iteration i; tie int [B, L]; source [B, L, 128] / keep bool [B, L]: the kept tokens, or None.
    Returns (latents [B, L, 128] after the final copy, {iterations: latents as stepped} for the counts in keep_steps)."""
    eps0 = (np.asarray(init_noise, dtype=F32) * F32(scheduler.init_noise_sigma)).astype(F32)
    tie = np.asarray(tie, dtype=np.int64)
    keep = np.zeros(tie.shape, dtype=bool) if keep is None else np.asarray(keep, dtype=bool)
    src = np.zeros_like(eps0) if source is None else np.asarray(source, dtype=F32)
    check_ties(tie, keep)
    scheduler.set_timesteps(num_inference_steps)
    ts = scheduler.timesteps
    is_ddim = hasattr(scheduler, "final_alpha_cumprod")
    is_dpm = hasattr(scheduler, "lambda_t")
    state = DpmState()
    latents = eps0.copy()
    snaps = {}
    for i in range(len(ts)):
        t = int(ts[i])
        latents = tie_copy(latents, tie)
        latents[keep] = add_noise(scheduler, src, eps0, t)[keep]
        model_in = np.concatenate([latents] * CFG_CHUNKS, axis=0)
        noise_pred, _ = denoise_fn(model_in, t, encoder_hidden_states, cond_masks)
        e = cfg_combine(noise_pred, guidance_scale)
        if is_dpm:
            latents = dpmpp_step(scheduler, state, e, i, latents)
        elif is_ddim:
            latents = scheduler.step(e, t, latents, eta=eta, noise=step_noise(i, t) if eta > 0 else None)
        else:
            latents = scheduler.step(e, t, latents, noise=step_noise(i, t) if t > 0 else None)
        if (i + 1) in keep_steps:
            snaps[i + 1] = latents.copy()
    return tie_copy(latents, tie), snaps
