"""The optimisation loop of ``convofusion_amd.fit.fit_conditioning`` on the CPU in float64 -- TEST INFRASTRUCTURE.

The same steps -- a timestep, seeded noise, ``x_t = add_noise(latents, noise, t)`` (``oracle.scheduler_ref``), the mean-squared error of
one conditional forward against the noise or the clean latents, a plain gradient-descent update of the fitted memories, each ONE tensor
shared by all rows -- with the gradient from torch autograd through ``oracle.denoiser_torch`` (the reference's unfolded formulation) at
float64.  Inputs taken in float32 and cast: weights, latents, memories, noise, the sinusoid row of the timestep.  Plain SGD only: Adam's
first steps are sign-like and flip on components whose gradient is rounding noise, so it has no parity leg.
"""
import contextlib

import numpy as np
import torch

from oracle import denoiser_torch, scheduler_ref
from oracle.denoiser_ref import MEM_NAMES


@contextlib.contextmanager
def _float64_time_rows():
    """oracle.denoiser_torch with the timestep's float32 sinusoid row cast to float64 (an input, like the weights)."""
    orig = denoiser_torch.timestep_embedding
    denoiser_torch.timestep_embedding = lambda t, dim=denoiser_torch.D: orig(t, dim).double()
    try:
        yield
    finally:
        denoiser_torch.timestep_embedding = orig


def noise_draws(shape, steps, seed):
    """The noise of ``fit_conditioning``'s steps when ``timesteps`` is given: standard normal float32 from one CPU generator."""
    gen = torch.Generator(device="cpu").manual_seed(int(seed))
    return [torch.randn(tuple(shape), generator=gen, dtype=torch.float32).numpy() for _ in range(steps)]


def loss_at(sd, sched_kw, latents, memories, masks, fitted, t, noise, prediction_type="epsilon"):
    """The loss of one step at given (t, noise) with the memories of ``fitted`` ({name: [1, S, 512]}) shared by all rows, float64."""
    return _loss(_sd64(sd), sched_kw, latents, memories, masks, {k: torch.from_numpy(np.asarray(v, dtype=np.float64)) for k, v in fitted.items()}, t,
                 noise, prediction_type).item()


def _sd64(sd):
    return {k: v.double() for k, v in denoiser_torch.to_torch(sd).items()}


def _loss(sd64, sched_kw, latents, memories, masks, params, t, noise, prediction_type):
    B = latents.shape[0]
    sch = scheduler_ref.DDPMSchedulerRef(**sched_kw)
    xt = torch.from_numpy(sch.add_noise(latents, noise, [t] * B)).double()
    target = torch.from_numpy(noise if prediction_type == "epsilon" else latents).double()
    mems = [params[k].expand(B, -1, -1) if k in params else torch.from_numpy(m).double() for k, m in zip(MEM_NAMES, memories)]
    mk = {}
    for k, v in (masks or {}).items():
        v = None if v is None else torch.from_numpy(np.asarray(v).astype(bool))
        mk[k] = v if v is None or k not in params else v[:1].expand(B, -1)
    with _float64_time_rows():
        out, _ = denoiser_torch.denoiser_forward.__wrapped__(sd64, xt, int(t), mems, mk)
    return ((out - target) ** 2).mean()


def fit_conditioning_ref(sd, sched_kw, latents, memories, masks, fit, init, steps, lr, timesteps, seed=0, prediction_type="epsilon"):
    """({name: fitted [1, S, 512] float64}, losses) of ``steps`` plain SGD steps from ``init`` ({name: [1, S, 512]})."""
    sd64 = _sd64(sd)
    params = {k: torch.from_numpy(np.asarray(init[k], dtype=np.float64)).clone().requires_grad_(True) for k in fit}
    losses = []
    for i, noise in enumerate(noise_draws(latents.shape, steps, seed)):
        with torch.enable_grad():
            loss = _loss(sd64, sched_kw, latents, memories, masks, params, timesteps[i], noise, prediction_type)
            grads = torch.autograd.grad(loss, [params[k] for k in fit])
        losses.append(loss.item())
        with torch.no_grad():
            for k, g in zip(fit, grads):
                params[k] -= lr * g
    return {k: v.detach().numpy() for k, v in params.items()}, losses
