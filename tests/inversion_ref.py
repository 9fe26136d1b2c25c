"""Restated DDIM inversion and anchored DDIM loop -- TEST INFRASTRUCTURE (numpy, float32 like the reference).

The reference has no inversion.  The step restated here is prompt-to-prompt's deterministic ``next_step``: for N steps the table is the
DDIM table reversed (ascending, ``0, T // N, ..., T - T // N`` + steps_offset), and iteration i at timestep t evaluates the guided
prediction at t -- the level the step moves TO -- and moves from t_cur = t - T // N:

    a_cur = abar[t_cur] if t_cur >= 0 else final_alpha      (final_alpha = 1 with set_alpha_to_one, else abar[0])
    x0    = (x - sqrt(1 - a_cur) * eps) / sqrt(a_cur)
    x     = sqrt(abar[t]) * x0 + sqrt(1 - abar[t]) * eps

every product, sum and quotient rounded to float32 on its own.  ``invert`` records the trajectory [N + 1][B][L][128] (slot 0 the
source, slot j the latents after j iterations).  ``anchored_reverse`` is the DDIM loop (eta 0, no clipping) from the inverted latents in
which, at the start of iteration i, the tokens with keep = 1 are set to ring[N - i] -- the inverted latents at the level iteration i starts
from.  The guidance combine is tests/modality_ref.cfg_combine_weighted with a per-iteration factor table, or the reference's combine
(oracle.sampler_ref.cfg_combine) when no table is given.
"""
import numpy as np

from oracle.sampler_ref import CFG_CHUNKS, cfg_combine
from oracle.scheduler_ref import DDIMSchedulerRef
from tests.modality_ref import cfg_combine_weighted

F32 = np.float32
# the default guidance of an inversion: the conditional prediction alone (w_all = 1 at guidance_scale 1, every other chunk 0)
COND_ONLY = (0.0, 0.0, 0.0, 0.0, 0.0, 1.0)


class DDIMInverseRef:
    """The inversion's tables and step on DDIMSchedulerRef's float32 tables (clip_sample off)."""

    def __init__(self, set_alpha_to_one=True, steps_offset=0, **kw):
        self.ddim = DDIMSchedulerRef(clip_sample=False, set_alpha_to_one=set_alpha_to_one, steps_offset=steps_offset, **kw)
        self.alphas_cumprod = self.ddim.alphas_cumprod
        self.final_alpha_cumprod = self.ddim.final_alpha_cumprod
        self.num_train_timesteps = self.ddim.num_train_timesteps

    def set_timesteps(self, num_inference_steps):
        self.ddim.set_timesteps(num_inference_steps)
        self.num_inference_steps = num_inference_steps
        self.timesteps = self.ddim.timesteps[::-1].copy()

    def coefficients(self, t):
        """float32 (sb, sa, c0, cx): x0 = (x - sb eps) / sa, x = c0 x0 + cx eps (the library's StepCoef row of kind 3)."""
        t_cur = int(t) - self.num_train_timesteps // self.num_inference_steps
        a_cur = self.alphas_cumprod[t_cur] if t_cur >= 0 else F32(self.final_alpha_cumprod)
        a_nxt = self.alphas_cumprod[int(t)]
        return (F32(np.sqrt(F32(F32(1.0) - a_cur))), F32(np.sqrt(F32(a_cur))), F32(np.sqrt(a_nxt)), F32(np.sqrt(F32(F32(1.0) - a_nxt))))

    def step(self, model_output, t, sample):
        sb, sa, c0, cx = self.coefficients(t)
        x0 = ((np.asarray(sample, F32) - sb * np.asarray(model_output, F32)) / sa).astype(F32)
        return (c0 * x0 + cx * np.asarray(model_output, F32)).astype(F32)


def factor_table(weights, guidance_scale, N, B):
    """float32 [N, B, 8]: float32(guidance_scale * w_c) in columns 1 - 6 (tests/modality_ref.weight_table on constant weights)."""
    from tests.modality_ref import weight_table
    return weight_table(np.broadcast_to(np.asarray(weights, np.float64), (N, B, 6)), guidance_scale)


def _combine(noise_pred, factors, i, guidance_scale):
    return cfg_combine_weighted(noise_pred, factors[i]) if factors is not None else cfg_combine(noise_pred, guidance_scale)


def invert(denoise_fn, scheduler, encoder_hidden_states, cond_masks, source, num_inference_steps, factors=None, guidance_scale=1.0):
    """denoise_fn(sample[7B, L, 128], t, enc, masks) -> (eps[7B, L, 128], att).  scheduler: DDIMInverseRef; source [B, L, 128];
    factors: float32 [N, B, 8] (``factor_table``) or None (the reference's combine at guidance_scale).  Returns (inverted latents,
    trajectory [N + 1, B, L, 128])."""
    scheduler.set_timesteps(num_inference_steps)
    x = np.asarray(source, F32).copy()
    traj = [x.copy()]
    for i, t in enumerate(scheduler.timesteps):
        noise_pred, _ = denoise_fn(np.concatenate([x] * CFG_CHUNKS, axis=0), int(t), encoder_hidden_states, cond_masks)
        x = scheduler.step(_combine(noise_pred, factors, i, guidance_scale), int(t), x)
        traj.append(x.copy())
    return x, np.stack(traj)


def anchored_reverse(denoise_fn, scheduler, encoder_hidden_states, cond_masks, ring, keep, num_inference_steps, factors=None,
                     guidance_scale=7.5, keep_steps=()):
    """The DDIM loop (scheduler: DDIMSchedulerRef with clip_sample off; eta 0) from ring[N], with the tokens of keep [B, L] set to
    ring[N - i] at the start of iteration i.  Returns (latents [B, L, 128], {iterations: latents after them} for keep_steps)."""
    scheduler.set_timesteps(num_inference_steps)
    N = len(scheduler.timesteps)
    ring = np.asarray(ring, F32)
    if ring.shape[0] != N + 1:
        raise ValueError(f"the ring has {ring.shape[0]} slots for {N} iterations")
    keep = np.asarray(keep, bool)
    x = ring[N].copy()
    snaps = {}
    for i, t in enumerate(scheduler.timesteps):
        x = x.copy()
        x[keep] = ring[N - i][keep]
        noise_pred, _ = denoise_fn(np.concatenate([x] * CFG_CHUNKS, axis=0), int(t), encoder_hidden_states, cond_masks)
        x = scheduler.step(_combine(noise_pred, factors, i, guidance_scale), int(t), x)
        if i + 1 in keep_steps:
            snaps[i + 1] = x.copy()
    return x, snaps
