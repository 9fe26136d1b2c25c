"""Restated edit loop -- token-masked in-painting from a start iteration k0 (img2img strength) -- TEST INFRASTRUCTURE (numpy, float32 like
the reference).

Modelled on oracle.sampler_ref.diffusion_reverse (the reference loop, convofusion.py:391-549) with the rollout's in-painting block
(unbounded_synthesis.py:70-76) generalised: at the start of iteration i the tokens with keep = 1 are set to add_noise(source, eps, t_i),
where eps is the run's initial N(0,1) draw (never rewritten: the rollout's i == 0 aliasing is not part of an edit).  The loop starts at
iteration k0 of the scheduler's FULL table (set_timesteps(N)), with every token at add_noise(source, eps, t_k0) when k0 > 0 and at eps when
k0 = 0; iteration i keeps its full-table index (step noise i).  The oracle loop has no start offset, so it is restated here rather than
hooked.

DPM-Solver++ (2M): diffusers 0.14.0 picks the order of a step from its ``lower_order_nums`` counter (0 after set_timesteps), so the first
EXECUTED step is first order whatever its index, and ``lower_order_final`` from the full table's length.  tests/dpmsolver_ref.py's
``coefficients`` keys the order on the step index (i == 0), right only for a loop that starts at 0; ``dpmpp_step`` restates the step with
the counter.
"""
import numpy as np

from oracle.sampler_ref import CFG_CHUNKS, cfg_combine

F32 = np.float32


def add_noise(sched, source, eps, t):
    """diffusers' add_noise in float32: sqrt(abar_t) * source + sqrt(1 - abar_t) * eps, every product and the sum rounded on their own."""
    ac = sched.alphas_cumprod[int(t)]
    sa, sb = F32(np.sqrt(ac)), F32(np.sqrt(F32(1.0) - ac))
    return (sa * np.asarray(source, F32) + sb * np.asarray(eps, F32)).astype(F32)


def strength_first_iteration(N, strength):
    """diffusers' img2img ``get_timesteps``: init_timestep = min(int(N * strength), N), t_start = max(N - init_timestep, 0)."""
    init_timestep = min(int(N * strength), N)
    return max(N - init_timestep, 0)


class DpmState:
    """The multistep state of diffusers 0.14.0's DPMSolverMultistepScheduler (reset by set_timesteps)."""

    def __init__(self):
        self.model_outputs = [None, None]
        self.lower_order_nums = 0


def dpmpp_order(state, i, n):
    """Order of the step at full-table index i of n: 1 while the counter is 0 or at lower_order_final, else 2."""
    lower_order_final = i == n - 1 and n < 15
    return 1 if (state.lower_order_nums < 1 or lower_order_final) else 2


def dpmpp_step(sched, state, model_output, i, sample):
    """One DPM-Solver++ (2M) step at full-table index i (sched: tests.dpmsolver_ref.DPMSolverMultistepRef, for its float32 tables)."""
    ts, n = sched.timesteps, len(sched.timesteps)
    t = int(ts[i])
    prev_t = 0 if i == n - 1 else int(ts[i + 1])
    order = dpmpp_order(state, i, n)
    x0 = ((sample - sched.sigma_t[t] * model_output) / sched.alpha_t[t]).astype(F32)
    state.model_outputs = [state.model_outputs[1], x0]
    lam_t, lam_s0 = sched.lambda_t[prev_t], sched.lambda_t[t]
    h = F32(lam_t - lam_s0)
    ratio = F32(sched.sigma_t[prev_t] / sched.sigma_t[t])
    ca = F32(sched.alpha_t[prev_t] * F32(np.exp(-h) - F32(1.0)))
    if order == 1:
        prev = (ratio * sample - ca * x0).astype(F32)
    else:
        m0, m1 = state.model_outputs[1], state.model_outputs[0]
        h0 = F32(lam_s0 - sched.lambda_t[int(ts[i - 1])])     # the previous executed step's timestep
        r0 = F32(h0 / h)
        d1 = (F32(F32(1.0) / r0) * (m0 - m1)).astype(F32)
        prev = ((ratio * sample - ca * m0) - F32(F32(0.5) * ca) * d1).astype(F32)
    state.lower_order_nums = min(state.lower_order_nums + 1, 2)
    return prev


def edit_reverse(denoise_fn, scheduler, encoder_hidden_states, cond_masks, init_noise, step_noise, source, keep, k0,
                 guidance_scale=7.5, num_inference_steps=20, eta=0.0, keep_steps=()):
    """denoise_fn(sample[7B, L, 128], t, enc, masks) -> (eps[7B, L, 128], att).  init_noise: the run's N(0,1) draw [B, L, 128];
    step_noise(i, t): the [B, L, 128] draw of full-table iteration i; source [B, L, 128]; keep bool [B, L]; k0: the first iteration.
    Returns (latents [B, L, 128], {executed iterations: latents after them} for the counts in keep_steps)."""
    eps0 = (np.asarray(init_noise, dtype=F32) * F32(scheduler.init_noise_sigma)).astype(F32)
    src = np.asarray(source, dtype=F32)
    keep = np.asarray(keep, dtype=bool)
    scheduler.set_timesteps(num_inference_steps)
    ts = scheduler.timesteps
    is_ddim = hasattr(scheduler, "final_alpha_cumprod")
    is_dpm = hasattr(scheduler, "lambda_t")
    state = DpmState()
    latents = add_noise(scheduler, src, eps0, ts[k0]) if k0 > 0 else eps0.copy()
    snaps = {}
    for i in range(k0, len(ts)):
        t = int(ts[i])
        latents = latents.copy()
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
        if (i + 1 - k0) in keep_steps:
            snaps[i + 1 - k0] = latents.copy()
    return latents, snaps
