"""GPU: ``convofusion_amd.fit`` -- conditioning fitted through the memory gradient (``Denoiser.vjp_memories``) against the same loop on
the CPU at float64 with torch autograd through ``oracle.denoiser_torch`` (tests/fit_ref.py).

Set-up: B = 2 examples of L = 4 tokens, S = (3, 5, 6, 2, 1), timesteps [613, 37, 981], three steps of plain SGD.  The learning rate
(50: the seeded weights give gradients of order 1e-3) is chosen on the CPU so that the reference moves every fitted tensor by at least
1e-2 of its norm -- asserted.  Gates: the movement ``|(fitted - init) - (fitted_ref - init)| / |fitted_ref - init| < 1e-3`` and every
recorded loss within 1e-3 relative, the project's loop gate.  Adam has no parity leg (tests/fit_ref.py): its run asserts only that the
loss at a fixed (t, noise) falls.
"""
import functools

import numpy as np
import pytest

from oracle import inputs
from tests import fit_ref
from tests.helpers import state_dict

pytestmark = pytest.mark.gpu

MEM_NAMES = inputs.MEM_NAMES
B, L, S, PAD = 2, 4, (3, 5, 6, 2, 1), (1, 0, 2, 0, 0)
TIMESTEPS, LR, SEED = [613, 37, 981], 50.0, 5
SCHED = dict(num_train_timesteps=1000, beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear")


@functools.lru_cache(maxsize=None)
def examples():
    inp = inputs.make_plain_batch(seed=81, Be=B, L=L, S=S, pad_tail=PAD)
    latents = np.random.Generator(np.random.PCG64(82)).standard_normal((B, L, 128), dtype=np.float32)
    return inp, latents


def start(fit):
    inp, _ = examples()
    return {k: inp["memories"][MEM_NAMES.index(k)].mean(axis=0, keepdims=True).astype(np.float32) for k in fit}


@functools.lru_cache(maxsize=None)
def reference(fit, prediction_type):
    inp, latents = examples()
    return fit_ref.fit_conditioning_ref(state_dict(1234, 1.0), SCHED, latents, inp["memories"], inp["masks"], fit, start(fit), len(TIMESTEPS), LR,
                                        TIMESTEPS, SEED, prediction_type)


@pytest.mark.parametrize("fit,prediction_type", [(("lsnemb",), "epsilon"), (("spkemb", "lsnemb"), "epsilon"), (("lsnemb",), "sample")])
def test_sgd_fit_matches_the_float64_loop_driven_by_torch_autograd(fit, prediction_type):
    import torch
    from convofusion_amd import fit as cfit, scheduler
    from tests.gpu_helpers import dev_inputs, hip_denoiser, to_dev
    inp, latents = examples()
    init = start(fit)
    want, want_losses = reference(fit, prediction_type)
    for k in fit:      # the reference moves every fitted tensor far beyond the gate below
        assert np.linalg.norm(want[k] - init[k]) >= 1e-2 * np.linalg.norm(init[k]), k
    m = hip_denoiser(1234, 1.0)
    mems, masks = dev_inputs(inp)
    sch = scheduler.DDPMScheduler(variance_type="fixed_small", clip_sample=True, prediction_type=prediction_type, **SCHED)
    got, losses = cfit.fit_conditioning(m, sch, to_dev(latents), mems, masks, fit=fit, init={k: to_dev(v) for k, v in init.items()},
                                        steps=len(TIMESTEPS), lr=LR, optimizer=lambda p: torch.optim.SGD(p, lr=LR), timesteps=TIMESTEPS, seed=SEED)
    assert sorted(got) == sorted(fit) and len(losses) == len(TIMESTEPS)
    for k in fit:
        assert tuple(got[k].shape) == (1, S[MEM_NAMES.index(k)], 512)
        move, move_ref = got[k].cpu().numpy().astype(np.float64) - init[k], want[k] - init[k]
        e = np.linalg.norm(move - move_ref) / np.linalg.norm(move_ref)
        print(f"fit={fit} {prediction_type}: {k} moved {np.linalg.norm(move_ref) / np.linalg.norm(init[k]):.3f} of its norm; movement vs float64 {e:.2e}")
        assert e < 1e-3, k
    rel = [abs(a - b) / abs(b) for a, b in zip(losses, want_losses)]
    print(f"fit={fit} {prediction_type}: losses {losses} (float64 {want_losses}), relative {max(rel):.2e}")
    assert max(rel) < 1e-3


def test_adam_fit_of_an_identity_lowers_the_loss_at_a_fixed_draw():
    """Five Adam steps of ``fit_identity`` from its default start (the mean of the given rows), timesteps drawn from the seed: the loss
    at one fixed (t, noise), measured by the float64 reference, falls."""
    from convofusion_amd import fit as cfit, scheduler
    from tests.gpu_helpers import dev_inputs, hip_denoiser, to_dev
    inp, latents = examples()
    m = hip_denoiser(1234, 1.0)
    mems, masks = dev_inputs(inp)
    sch = scheduler.DDPMScheduler(variance_type="fixed_small", clip_sample=True, **SCHED)
    ident, losses = cfit.fit_identity(m, sch, to_dev(latents), mems, masks, steps=5, lr=0.05, timesteps=[500] * 5, seed=9)
    assert tuple(ident.shape) == (1, 1, 512) and len(losses) == 5
    noise = fit_ref.noise_draws(latents.shape, 1, 1234)[0]
    sd = state_dict(1234, 1.0)
    before = fit_ref.loss_at(sd, SCHED, latents, inp["memories"], inp["masks"], start(("lsnemb",)), 500, noise)
    after = fit_ref.loss_at(sd, SCHED, latents, inp["memories"], inp["masks"], {"lsnemb": ident.cpu().numpy()}, 500, noise)
    print(f"Adam, 5 steps: loss at the fixed draw {before:.6f} -> {after:.6f}; step losses {losses}")
    assert after < before
    # drawn timesteps: the same seed gives the same fit, bit for bit
    a, la = cfit.fit_identity(m, sch, to_dev(latents), mems, masks, steps=2, lr=0.05, seed=3)
    b, lb = cfit.fit_identity(m, sch, to_dev(latents), mems, masks, steps=2, lr=0.05, seed=3)
    assert la == lb and bool((a == b).all())
