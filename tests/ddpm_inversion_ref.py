"""Restated edit-friendly DDPM inversion and its replay -- TEST INFRASTRUCTURE (numpy, float32 like the reference).

The reference has no inversion.  Restated here is the "edit-friendly DDPM noise space" of Huberman-Spiegelglas et al. (CVPR 2024) on
oracle.scheduler_ref.DDPMSchedulerRef's float32 tables, for the table t_0 > t_1 > ... > t_{N-1} of a DDPM run:

    x_i   = fl(fl(sqrt(abar_i) * source) + fl(sqrt(1 - abar_i) * eps_i))        an independent draw eps_i per level
    mu_i  = c0 * clip((x_i - sb * eps_hat_i) / sa) + cx * x_i                    DDPMSchedulerRef.step without its noise term
    z_i   = (x_{i+1} - mu_i) / sigma_i   (x_N = source),   z_i = 0 where t_i = 0 (the step adds no noise)

``invert`` returns the trajectory [N + 1][B][L][128] in the DDIM inversion ring's convention (slot 0 the source, slot N - i the level
ENTERING iteration i) and the noise [N][B][L][128].  ``replay`` is the DDPM loop from trajectory[N - k0] with noise[i] as the step noise
of iteration i and the tokens of keep [B, L] set to trajectory[N - i] at the start of iteration i.  The guidance combine is
tests/modality_ref.cfg_combine_weighted with a per-iteration factor table, or the reference's combine (oracle.sampler_ref.cfg_combine).
"""
import numpy as np

from oracle.sampler_ref import CFG_CHUNKS, cfg_combine
from oracle.scheduler_ref import DDPMSchedulerRef  # noqa: F401  (the scheduler the functions below take)
from tests.inversion_ref import COND_ONLY, factor_table  # noqa: F401
from tests.modality_ref import cfg_combine_weighted

F32 = np.float32


def _combine(noise_pred, factors, i, guidance_scale):
    return cfg_combine_weighted(noise_pred, factors[i]) if factors is not None else cfg_combine(noise_pred, guidance_scale)


def level(scheduler, t, source, eps):
    """fl(fl(sa * source) + fl(sb * eps)) at timestep t (the edit run's re-noising arithmetic)."""
    sb, sa = scheduler.coefficients(t)[:2]
    return ((sa * np.asarray(source, F32)).astype(F32) + (sb * np.asarray(eps, F32)).astype(F32)).astype(F32)


def mean(scheduler, t, sample, model_output):
    """The DDPM step's posterior mean (DDPMSchedulerRef.step without the noise term) and sigma."""
    sb, sa, c0, cx, sigma = scheduler.coefficients(t)
    x0 = ((sample - sb * model_output) / sa).astype(F32)
    if scheduler.clip_sample:
        x0 = np.clip(x0, F32(-1.0), F32(1.0))
    return (c0 * x0 + cx * sample).astype(F32), sigma


def invert(denoise_fn, scheduler, encoder_hidden_states, cond_masks, source, level_noise, num_inference_steps, factors=None,
           guidance_scale=1.0):
    """denoise_fn(sample[7B, L, 128], t, enc, masks) -> (eps[7B, L, 128], att).  scheduler: DDPMSchedulerRef; source [B, L, 128];
    level_noise [N, B, L, 128]; factors: float32 [N, B, 8] or None.  Returns (trajectory [N + 1, B, L, 128], noise [N, B, L, 128])."""
    scheduler.set_timesteps(num_inference_steps)
    ts = [int(t) for t in scheduler.timesteps]
    N = len(ts)
    source = np.asarray(source, F32)
    level_noise = np.asarray(level_noise, F32)
    if level_noise.shape != (N,) + source.shape:
        raise ValueError(f"level_noise is {level_noise.shape} for {N} levels of {source.shape}")
    traj = np.empty((N + 1,) + source.shape, F32)
    traj[0] = source
    for i, t in enumerate(ts):
        traj[N - i] = level(scheduler, t, source, level_noise[i])
    noise = np.zeros((N,) + source.shape, F32)
    for i, t in enumerate(ts):
        x = traj[N - i]
        noise_pred, _ = denoise_fn(np.concatenate([x] * CFG_CHUNKS, axis=0), t, encoder_hidden_states, cond_masks)
        mu, sigma = mean(scheduler, t, x, _combine(noise_pred, factors, i, guidance_scale))
        if t > 0:
            noise[i] = ((traj[N - i - 1] - mu) / sigma).astype(F32)
    return traj, noise


def replay(denoise_fn, scheduler, encoder_hidden_states, cond_masks, trajectory, noise, num_inference_steps, keep=None, first_iteration=0,
           factors=None, guidance_scale=7.5, keep_steps=(), step_noise=None):
    """The DDPM loop from trajectory[N - k0] over iterations k0 .. N - 1 with noise[i] as iteration i's step noise (``step_noise``
    [N, B, L, 128]: another noise in its place -- the contrast of the closure test) and the tokens of keep [B, L] set to
    trajectory[N - i] at the start of iteration i.  Returns (latents, {iterations done, counted from 0 in the full table: latents})."""
    scheduler.set_timesteps(num_inference_steps)
    ts = [int(t) for t in scheduler.timesteps]
    N = len(ts)
    trajectory = np.asarray(trajectory, F32)
    z = np.asarray(noise if step_noise is None else step_noise, F32)
    if trajectory.shape[0] != N + 1 or z.shape[0] != N:
        raise ValueError(f"the noise space has {trajectory.shape[0]} / {z.shape[0]} slots for {N} iterations")
    keep = np.zeros(trajectory.shape[1:3], bool) if keep is None else np.asarray(keep, bool)
    k0 = int(first_iteration)
    x = trajectory[N - k0].copy()
    snaps = {}
    for i in range(k0, N):
        x = x.copy()
        x[keep] = trajectory[N - i][keep]
        noise_pred, _ = denoise_fn(np.concatenate([x] * CFG_CHUNKS, axis=0), ts[i], encoder_hidden_states, cond_masks)
        x = scheduler.step(_combine(noise_pred, factors, i, guidance_scale), ts[i], x, noise=z[i])
        if i + 1 in keep_steps:
            snaps[i + 1] = x.copy()
    return x, snaps


def rel_l2(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30))
