#!/usr/bin/env python
"""Golden trajectories of the loop with per-modality guidance weights, generated from the REFERENCE ``Denoiser`` (imported from the
reference checkout by make_golden.py; build container only -- the tests read the .npz files alone).

The restated loop (oracle.sampler_ref.diffusion_reverse) drives the reference denoiser; while it runs, its module-level ``cfg_combine``
is replaced by tests/modality_ref.cfg_combine_weighted with iteration i's row of the weight table (oracle/ itself is not changed).
Weights: tests/modality_ref.golden_weights -- utterance 0 on an interval schedule, utterance 1 on a ramp, apb 0 throughout.

  traj_modality_ddpm20.npz    : DDPM, B = 2, L = 16, 20 steps, Philox step noise; snapshots after steps 1, 8 and 14
  traj_modality_dpmpp10.npz   : DPM-Solver++ (2M), B = 2, L = 16, 10 steps; snapshots after steps 1, 4 and 7
  traj_modality_inpaint20.npz : the DDPM rollout window (8 in-painted tokens re-noised every step), 20 steps; snapshots after 1, 8, 14

Each file holds the weights [N, 2, 6] (float64) it was made with.

Usage:  python tests/golden/make_golden_modality.py
"""
import os
import sys
import time

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)

from make_golden import build_reference, ref_forward  # noqa: E402  (imports the reference Denoiser)
from oracle import inputs, philox_ref, sampler_ref, scheduler_ref, weights  # noqa: E402
from tests import modality_ref  # noqa: E402
from tests.dpmsolver_ref import DPMSolverMultistepRef  # noqa: E402

torch.set_grad_enabled(False)

DPM_KW = dict(num_train_timesteps=1000, beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear")
SEED = 2025
G_SCALE = 7.5


def weighted_loop(table, **kw):
    """sampler_ref.diffusion_reverse with cfg_combine replaced by the weighted combine of iteration i (i = the call's index)."""
    calls = [0]

    def combine(noise_pred, guidance_scale):
        i = calls[0]
        calls[0] += 1
        return modality_ref.cfg_combine_weighted(noise_pred, table[i])

    original = sampler_ref.cfg_combine
    sampler_ref.cfg_combine = combine
    try:
        out = sampler_ref.diffusion_reverse(**kw)
    finally:
        sampler_ref.cfg_combine = original
    assert calls[0] == len(table), (calls[0], len(table))
    return out


def main():
    ref = build_reference(weights.make_state_dict(seed=1234))
    fn = lambda x, t, e, m: ref_forward(ref, x, t, e, m)   # noqa: E731
    B, L, S, pad = 2, 16, (6, 20, 6, 8, 1), (2, 0, 1, 0, 0)
    for name, sched, n, keep, inpaint in [
        ("ddpm20", scheduler_ref.DDPMSchedulerRef(), 20, (1, 8, 14), False),
        ("dpmpp10", DPMSolverMultistepRef(**DPM_KW), 10, (1, 4, 7), False),
        ("inpaint20", scheduler_ref.DDPMSchedulerRef(), 20, (1, 8, 14), True),
    ]:
        seed = SEED + (1 if inpaint else 0)
        cb = inputs.make_cfg_batch(seed=seed, B=B, L=L, S=S, pad_tail=pad)
        init = philox_ref.normal_tensor(seed, 0, range(B), 1, L)
        preseq = (0.5 * philox_ref.normal_tensor(seed, 7, range(B), 2, 8)).astype(np.float32) if inpaint else None
        w = modality_ref.golden_weights(n)
        noise = None if "dpmpp" in name else (lambda i, t: philox_ref.normal_tensor(seed, i, range(B), 0, L))
        t0 = time.time()
        lat, snaps, _ = weighted_loop(modality_ref.weight_table(w, G_SCALE), denoise_fn=fn, scheduler=sched,
                                      encoder_hidden_states=cb["memories"], cond_masks=cb["masks"], init_latents=init,
                                      step_noise=noise or (lambda i, t: None), guidance_scale=G_SCALE, num_inference_steps=n,
                                      preseq=preseq, keep_steps=keep)
        print(f"traj_modality_{name}: {time.time() - t0:.1f}s |lat| {np.abs(lat).mean():.3f}", flush=True)
        extra = dict(preseq=preseq) if inpaint else {}
        np.savez_compressed(os.path.join(HERE, f"traj_modality_{name}.npz"), latents=lat, weights=w, **extra,
                            **{f"step{k}": v for k, v in snaps.items()}, meta=np.array([B, L, *S, *pad, n, seed], dtype=np.int64))
    print("done")


if __name__ == "__main__":
    main()
