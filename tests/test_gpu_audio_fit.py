"""-m gpu: ``fit.fit_audio_encoder`` -- the audio encoder trained against the frozen HIP denoiser -- against the same loop on the CPU at
float64 with torch autograd through the encoder and ``oracle.denoiser_torch`` (tests/audio_fit_ref.py).

Set-up, as tests/test_gpu_fit.py: B = 2 examples of L = 4 tokens, S = (3, 5, 6, 2, 1), timesteps [613, 37, 981], three steps of plain SGD;
the Mel rows are [2, 5, 80] around -20 dB, the encoder 80 / 256 / 512 with seeded weights (nn.Linear's default init).  The learning rate
(2) is chosen on the CPU so that the reference moves every trained tensor by at least 2e-3 of its norm -- some 3e4 float32 ulps; the
first layer's bias moves least, 4.6e-3 -- asserted.  Gates, the project's loop gate: the movement
``|(fitted - init) - (fitted_ref - init)| / |fitted_ref - init| < 1e-3`` per tensor and every recorded loss within 1e-3 relative.
Adam has no parity leg (tests/fit_ref.py): its run asserts only that the loss at a fixed (t, noise) falls.
"""
import functools

import numpy as np
import pytest

from oracle import inputs
from tests import audio_enc_vjp_ref as R
from tests import audio_fit_ref, fit_ref
from tests.helpers import state_dict

pytestmark = pytest.mark.gpu

B, L, S, PAD = 2, 4, (3, 5, 6, 2, 1), (1, 0, 2, 0, 0)
TIMESTEPS, LR, SEED = [613, 37, 981], 2.0, 5
SCHED = dict(num_train_timesteps=1000, beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear")


@functools.lru_cache(maxsize=None)
def examples():
    inp = inputs.make_plain_batch(seed=81, Be=B, L=L, S=S, pad_tail=PAD)
    latents = np.random.Generator(np.random.PCG64(82)).standard_normal((B, L, 128), dtype=np.float32)
    params = R.seeded_params(80, 256, 512, seed=91)
    mel = ((R.seeded_inputs(B * S[1], 80, 512, seed=92)[0].reshape(B, S[1], 80) + 40.0) / 25.0 * 10.0 - 20.0).astype(np.float32)
    return inp, latents, params, mel


@functools.lru_cache(maxsize=None)
def reference(train, prediction_type):
    inp, latents, params, mel = examples()
    return audio_fit_ref.fit_audio_encoder_ref(state_dict(1234, 1.0), SCHED, latents, mel, inp["memories"], inp["masks"], params, train, len(TIMESTEPS),
                                               LR, TIMESTEPS, SEED, prediction_type)


def device_encoder():
    from tests.test_gpu_audio_enc_vjp import encoder_of
    return encoder_of(examples()[2])


def device_state(enc):
    return {k: v.detach().cpu().numpy() for k, v in enc.state_dict().items()}


def run(enc, train=None, prediction_type="epsilon", **kw):
    import torch
    from convofusion_amd import fit as cfit, scheduler
    from tests.gpu_helpers import dev_inputs, hip_denoiser, to_dev
    inp, latents, _, mel = examples()
    mems, masks = dev_inputs(inp)
    mems[1] = None                                                      # not read: the audio memory is the encoder's
    sch = scheduler.DDPMScheduler(variance_type="fixed_small", clip_sample=True, prediction_type=prediction_type, **SCHED)
    args = dict(steps=len(TIMESTEPS), lr=LR, optimizer=lambda p: torch.optim.SGD(p, lr=LR), timesteps=TIMESTEPS, seed=SEED, train=train)
    args.update(kw)
    return cfit.fit_audio_encoder(hip_denoiser(1234, 1.0), sch, enc, to_dev(latents), to_dev(mel), mems, masks, **args)


@pytest.mark.parametrize("prediction_type", ["epsilon", "sample"])
def test_sgd_fit_matches_the_float64_loop_driven_by_torch_autograd(prediction_type):
    init = examples()[2]
    want, want_losses = reference(R.KEYS, prediction_type)
    for k in R.KEYS:      # the reference moves every trained tensor far beyond float32 resolution
        assert np.linalg.norm(want[k] - init[k]) >= 2e-3 * np.linalg.norm(init[k]), k
    enc = device_encoder()
    losses = run(enc, prediction_type=prediction_type)
    got = device_state(enc)
    assert len(losses) == len(TIMESTEPS)
    worst = []
    for k in R.KEYS:
        move, move_ref = got[k].astype(np.float64) - init[k], want[k] - init[k]
        e = np.linalg.norm(move - move_ref) / np.linalg.norm(move_ref)
        print(f"{prediction_type}: {k} moved {np.linalg.norm(move_ref) / np.linalg.norm(init[k]):.4f} of its norm; movement vs float64 {e:.2e}")
        worst.append((e, k))
    rel = [abs(a - b) / abs(b) for a, b in zip(losses, want_losses)]
    print(f"{prediction_type}: losses {losses} (float64 {want_losses}), relative {max(rel):.2e}")
    assert max(worst)[0] < 1e-3, max(worst)
    assert max(rel) < 1e-3


def test_adam_lowers_the_loss_at_a_fixed_draw_and_a_seed_gives_the_same_bits():
    import torch
    inp, latents, params, mel = examples()
    enc = device_encoder()
    losses = run(enc, steps=5, lr=1e-3, optimizer=None, timesteps=[500] * 5, seed=9)
    assert len(losses) == 5
    noise = fit_ref.noise_draws(latents.shape, 1, 1234)[0]
    sd = state_dict(1234, 1.0)
    before = audio_fit_ref.loss_at(sd, SCHED, latents, mel, inp["memories"], inp["masks"], params, 500, noise)
    after = audio_fit_ref.loss_at(sd, SCHED, latents, mel, inp["memories"], inp["masks"], device_state(enc), 500, noise)
    print(f"Adam, 5 steps: loss at the fixed draw {before:.6f} -> {after:.6f}; step losses {losses}")
    assert after < before
    # drawn timesteps: the same seed gives the same fit, bit for bit
    a, b = device_encoder(), device_encoder()
    la = run(a, steps=2, lr=1e-3, optimizer=None, timesteps=None, seed=3)
    lb = run(b, steps=2, lr=1e-3, optimizer=None, timesteps=None, seed=3)
    assert la == lb
    for (k, u), v in zip(a.state_dict().items(), b.state_dict().values()):
        assert torch.equal(u, v), k


def test_train_names_the_only_tensor_that_moves():
    init = examples()[2]
    enc = device_encoder()
    run(enc, train=("out_net.weight",), steps=1)
    got = device_state(enc)
    for k in R.KEYS:
        same = np.array_equal(got[k], init[k])
        assert same == (k != "out_net.weight"), k     # (a subset's parity is the all-keys leg's: a gradient's bits do not depend on what else is asked for)
