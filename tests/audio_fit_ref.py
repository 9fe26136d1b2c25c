"""The optimisation loop of ``convofusion_amd.fit.fit_audio_encoder`` on the CPU in float64 -- TEST INFRASTRUCTURE.

The same steps as the product's -- a timestep, seeded noise, ``x_t = add_noise(latents, noise, t)`` (``oracle.scheduler_ref``), the audio
memory from the encoder, the mean-squared error of one conditional forward with every example's own memories against the noise or the
clean latents, a plain gradient-descent update of the trained parameters -- with the gradient from torch autograd through a plain
``nn.Sequential``-equivalent of the encoder (Linear, LeakyReLU(0.1), Linear, LeakyReLU(0.1), Linear; no dropout) and
``oracle.denoiser_torch`` at float64.  Inputs taken in float32 and cast.  Plain SGD only, as tests/fit_ref.py explains.
"""
import numpy as np
import torch
import torch.nn.functional as F

from oracle import denoiser_torch, scheduler_ref
from oracle.denoiser_ref import MEM_NAMES
from tests.audio_enc_vjp_ref import KEYS
from tests.fit_ref import _float64_time_rows, _sd64, noise_draws


def encode(params, mel):
    h = F.leaky_relu(F.linear(mel, params[KEYS[0]], params[KEYS[1]]), 0.1)
    h = F.leaky_relu(F.linear(h, params[KEYS[2]], params[KEYS[3]]), 0.1)
    return F.linear(h, params[KEYS[4]], params[KEYS[5]])


def _loss(sd64, sched_kw, latents, mel, memories, masks, params, t, noise, prediction_type):
    B = latents.shape[0]
    sch = scheduler_ref.DDPMSchedulerRef(**sched_kw)
    xt = torch.from_numpy(sch.add_noise(latents, noise, [t] * B)).double()
    target = torch.from_numpy(noise if prediction_type == "epsilon" else latents).double()
    alsn = encode(params, torch.from_numpy(mel).double())
    mems = [alsn if k == "alsn" else torch.from_numpy(m).double() for k, m in zip(MEM_NAMES, memories)]
    mk = {k: (None if v is None else torch.from_numpy(np.asarray(v).astype(bool))) for k, v in (masks or {}).items()}
    with _float64_time_rows():
        out, _ = denoiser_torch.denoiser_forward.__wrapped__(sd64, xt, int(t), mems, mk)
    return ((out - target) ** 2).mean()


def _params64(enc_params):
    return {k: torch.from_numpy(np.asarray(enc_params[k], dtype=np.float64)).clone() for k in KEYS}


def loss_at(sd, sched_kw, latents, mel, memories, masks, enc_params, t, noise, prediction_type="epsilon"):
    """The loss of one step at given (t, noise) with the encoder's parameters ``enc_params`` ({key: array}), float64."""
    with torch.no_grad():
        return _loss(_sd64(sd), sched_kw, latents, mel, memories, masks, _params64(enc_params), t, noise, prediction_type).item()


def fit_audio_encoder_ref(sd, sched_kw, latents, mel, memories, masks, enc_params, train, steps, lr, timesteps, seed=0, prediction_type="epsilon"):
    """({key: parameter after ``steps`` plain SGD steps, float64}, losses); the keys outside ``train`` come back unchanged."""
    sd64 = _sd64(sd)
    params = _params64(enc_params)
    for k in train:
        params[k].requires_grad_(True)
    losses = []
    for i, noise in enumerate(noise_draws(latents.shape, steps, seed)):
        with torch.enable_grad():
            loss = _loss(sd64, sched_kw, latents, mel, memories, masks, params, timesteps[i], noise, prediction_type)
            grads = torch.autograd.grad(loss, [params[k] for k in train])
        losses.append(loss.item())
        with torch.no_grad():
            for k, g in zip(train, grads):
                params[k] -= lr * g
    return {k: v.detach().numpy() for k, v in params.items()}, losses
