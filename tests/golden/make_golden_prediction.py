#!/usr/bin/env python
"""Golden trajectories of the loop for an x0-predicting denoiser (``prediction_type="sample"``, the reference's
TRAIN.ABLATION.PREDICT_EPSILON: False), generated from the REFERENCE ``Denoiser`` (imported from the reference checkout by
make_golden.py; build container only -- the tests read the .npz files alone).

The restated loop (oracle.sampler_ref.diffusion_reverse) drives the reference denoiser -- seeded weights, its output read as x0 -- with
the restated steps of tests/prediction_ref.py.  The 7-way combine is the loop's own: the reference applies the same combine to whatever
the denoiser returns (convofusion.py:527-541).

  traj_pred_ddpm20.npz          : DDPM, clip_sample on, Philox step noise, B = 2, L = 16, memories (24, 161, 24, 8, 1), pads
                                  (4, 0, 6, 0, 0), 20 steps; snapshots after steps 1, 2 and 10
  traj_pred_ddim10.npz          : DDIM, eta 0, clip_sample on, B = 2, memories (6, 20, 6, 8, 1), 10 steps; snapshots after 1, 5 and 9
  traj_pred_dpmpp10.npz         : DPM-Solver++ (2M), 10 steps (N < 15: the last step is first order again); snapshots after 1, 5 and 9
  traj_pred_inpaint20.npz       : the DDPM rollout window (8 in-painted tokens re-noised every step), 20 steps; snapshots after 1, 2, 20
  traj_pred_modality_ddpm20.npz : DDPM, 20 steps, the per-utterance weight schedule of tests/modality_ref.golden_weights (apb 0
                                  throughout: a chunk a pruned run drops); snapshots after 1, 8 and 14; holds its weights [N, 2, 6]

Usage:  python tests/golden/make_golden_prediction.py
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
from make_golden_modality import weighted_loop  # noqa: E402
from oracle import inputs, philox_ref, sampler_ref, weights  # noqa: E402
from tests import modality_ref  # noqa: E402
from tests.prediction_ref import DDIMSampleRef, DDPMSampleRef, DPMSolverSampleRef  # noqa: E402

torch.set_grad_enabled(False)

DPM_KW = dict(num_train_timesteps=1000, beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear")
SEED = 2026
G_SCALE = 7.5


def save(name, lat, snaps, meta, **extra):
    print(f"traj_pred_{name}: |lat| {np.abs(lat).mean():.3f}, clipped {float((np.abs(lat) >= 1).mean()):.3f}", flush=True)
    np.savez_compressed(os.path.join(HERE, f"traj_pred_{name}.npz"), latents=lat, **extra, **{f"step{k}": v for k, v in snaps.items()},
                        meta=np.array(meta, dtype=np.int64))


def main():
    ref = build_reference(weights.make_state_dict(seed=1234))
    fn = lambda x, t, e, m: ref_forward(ref, x, t, e, m)   # noqa: E731
    for name, sched, n, B, L, S, pad, keep, noisy in [
        ("ddpm20", DDPMSampleRef(), 20, 2, 16, (24, 161, 24, 8, 1), (4, 0, 6, 0, 0), (1, 2, 10), True),
        ("ddim10", DDIMSampleRef(), 10, 2, 16, (6, 20, 6, 8, 1), (2, 0, 1, 0, 0), (1, 5, 9), False),
        ("dpmpp10", DPMSolverSampleRef(**DPM_KW), 10, 2, 16, (6, 20, 6, 8, 1), (2, 0, 1, 0, 0), (1, 5, 9), False),
    ]:
        cb = inputs.make_cfg_batch(seed=SEED, B=B, L=L, S=S, pad_tail=pad)
        init = philox_ref.normal_tensor(SEED, 0, range(B), 1, L)
        noise = (lambda i, t: philox_ref.normal_tensor(SEED, i, range(B), 0, L)) if noisy else (lambda i, t: None)
        t0 = time.time()
        lat, snaps, _ = sampler_ref.diffusion_reverse(fn, sched, cb["memories"], cb["masks"], init, noise, guidance_scale=G_SCALE,
                                                      num_inference_steps=n, eta=0.0, keep_steps=keep)
        print(f"{time.time() - t0:.1f}s", end=" ")
        save(name, lat, snaps, [B, L, *S, *pad, n, SEED])
    # the rollout window (unbounded_synthesis.py:28-187), as traj_inpaint25.npz: 8 preseq tokens
    B, L, S, pad, n, seed = 2, 16, (6, 20, 6, 8, 1), (2, 0, 1, 0, 0), 20, SEED + 1
    cb = inputs.make_cfg_batch(seed=seed, B=B, L=L, S=S, pad_tail=pad)
    init = philox_ref.normal_tensor(seed, 0, range(B), 1, L)
    preseq = (0.5 * philox_ref.normal_tensor(seed, 7, range(B), 2, 8)).astype(np.float32)
    lat, snaps, _ = sampler_ref.diffusion_reverse(fn, DDPMSampleRef(), cb["memories"], cb["masks"], init,
                                                  lambda i, t: philox_ref.normal_tensor(seed, i, range(B), 0, L), guidance_scale=G_SCALE,
                                                  num_inference_steps=n, preseq=preseq, keep_steps=(1, 2, 20))
    save("inpaint20", lat, snaps, [B, L, *S, *pad, n, seed], preseq=preseq)
    # per-utterance weights, one chunk pruned (tests/golden/make_golden_modality.py's loop and schedule)
    seed = SEED + 2
    cb = inputs.make_cfg_batch(seed=seed, B=B, L=L, S=S, pad_tail=pad)
    init = philox_ref.normal_tensor(seed, 0, range(B), 1, L)
    w = modality_ref.golden_weights(n)
    lat, snaps, _ = weighted_loop(modality_ref.weight_table(w, G_SCALE), denoise_fn=fn, scheduler=DDPMSampleRef(),
                                  encoder_hidden_states=cb["memories"], cond_masks=cb["masks"], init_latents=init,
                                  step_noise=lambda i, t: philox_ref.normal_tensor(seed, i, range(B), 0, L), guidance_scale=G_SCALE,
                                  num_inference_steps=n, keep_steps=(1, 8, 14))
    save("modality_ddpm20", lat, snaps, [B, L, *S, *pad, n, seed], weights=w)
    print("done")


if __name__ == "__main__":
    main()
