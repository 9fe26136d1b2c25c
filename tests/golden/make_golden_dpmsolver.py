#!/usr/bin/env python
"""Golden trajectories of the DPM-Solver++ (2M) loop, generated from the REFERENCE ``Denoiser`` (imported from the reference checkout
by make_golden.py; build container only -- the tests read the .npz files alone).

The restated loop (oracle.sampler_ref) drives the reference denoiser with tests/dpmsolver_ref.py (restated diffusers 0.14.0
DPMSolverMultistepScheduler, default configuration) and oracle.philox_ref initial latents:

  traj_dpmpp20_b2.npz      : B = 2, L = 16, 20 steps (first order at step 0 only); snapshots after steps 1, 2 and 10
  traj_dpmpp10.npz         : B = 2, 10 steps: N < 15, so the last step is first order again; snapshots after 1, 5 and 9
  traj_inpaint_dpmpp20.npz : the rollout window (8 in-painted tokens re-noised every step with add_noise on the same betas' table)
  traj_c2_dpmpp20.npz      : utterance 17 of the headline shape's seeded B = 32 batch (as make_golden_c2full.py), 20 steps;
                             snapshots after 1, 2 and 10 (~25 s on CPU)

Usage:  python tests/golden/make_golden_dpmsolver.py [small] [c2]
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
from make_golden_c2rows import B as C2_B, L as C2_L, S as C2_S, PAD as C2_PAD, SEED as C2_SEED, utterance_rows  # noqa: E402
from oracle import inputs, philox_ref, sampler_ref, weights  # noqa: E402
from tests.dpmsolver_ref import DPMSolverMultistepRef  # noqa: E402

torch.set_grad_enabled(False)

SCHED_KW = dict(num_train_timesteps=1000, beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear")
SEED = 2024


def small(ref):
    fn = lambda x, t, e, m: ref_forward(ref, x, t, e, m)   # noqa: E731
    for name, n, B, L, S, pad, keep in [
        ("dpmpp20_b2", 20, 2, 16, (24, 161, 24, 8, 1), (4, 0, 6, 0, 0), (1, 2, 10)),
        ("dpmpp10", 10, 2, 16, (6, 20, 6, 8, 1), (2, 0, 1, 0, 0), (1, 5, 9)),
    ]:
        cb = inputs.make_cfg_batch(seed=SEED, B=B, L=L, S=S, pad_tail=pad)
        init = philox_ref.normal_tensor(SEED, 0, range(B), 1, L)
        t0 = time.time()
        lat, snaps, _ = sampler_ref.diffusion_reverse(fn, DPMSolverMultistepRef(**SCHED_KW), cb["memories"], cb["masks"], init,
                                                      lambda i, t: None, guidance_scale=7.5, num_inference_steps=n, keep_steps=keep)
        print(f"traj_{name}: {time.time() - t0:.1f}s |lat| {np.abs(lat).mean():.3f}", flush=True)
        np.savez_compressed(os.path.join(HERE, f"traj_{name}.npz"), latents=lat, **{f"step{k}": v for k, v in snaps.items()},
                            meta=np.array([B, L, *S, *pad, n, SEED], dtype=np.int64))
    # the rollout window (unbounded_synthesis.py:28-187), as traj_inpaint25.npz: 8 preseq tokens
    B, L, S, pad, n, seed = 2, 16, (6, 20, 6, 8, 1), (2, 0, 1, 0, 0), 20, SEED + 1
    cb = inputs.make_cfg_batch(seed=seed, B=B, L=L, S=S, pad_tail=pad)
    init = philox_ref.normal_tensor(seed, 0, range(B), 1, L)
    preseq = (0.5 * philox_ref.normal_tensor(seed, 7, range(B), 2, 8)).astype(np.float32)
    lat, snaps, _ = sampler_ref.diffusion_reverse(fn, DPMSolverMultistepRef(**SCHED_KW), cb["memories"], cb["masks"], init,
                                                  lambda i, t: None, guidance_scale=7.5, num_inference_steps=n, preseq=preseq,
                                                  keep_steps=(1, 2, 20))
    print(f"traj_inpaint_dpmpp20: |lat| {np.abs(lat).mean():.3f}", flush=True)
    np.savez_compressed(os.path.join(HERE, "traj_inpaint_dpmpp20.npz"), latents=lat, preseq=preseq,
                        **{f"step{k}": v for k, v in snaps.items()}, meta=np.array([B, L, *S, *pad, n, seed], dtype=np.int64))


def c2():
    U, n = 17, 20
    ref = build_reference(weights.make_state_dict(seed=1234), mem_len=1536)
    cb = inputs.make_cfg_batch(seed=C2_SEED, B=C2_B, L=C2_L, S=C2_S, pad_tail=C2_PAD, uncond_pad_tail=C2_PAD)
    mems, masks = utterance_rows(cb, U)
    init = philox_ref.normal_tensor(C2_SEED, 0, [U], 1, C2_L)
    t0 = time.time()
    lat, snaps, _ = sampler_ref.diffusion_reverse(lambda x, t, e, m: ref_forward(ref, x, t, e, m), DPMSolverMultistepRef(**SCHED_KW),
                                                  mems, masks, init, lambda i, t: None, guidance_scale=7.5, num_inference_steps=n,
                                                  keep_steps=(1, 2, 10))
    print(f"traj_c2_dpmpp20: {time.time() - t0:.1f}s |lat| {np.abs(lat).mean():.3f}", flush=True)
    np.savez_compressed(os.path.join(HERE, "traj_c2_dpmpp20.npz"), latents=lat, **{f"step{k}": v for k, v in snaps.items()},
                        meta=np.array([C2_B, C2_L, *C2_S, *C2_PAD, n, C2_SEED, U], dtype=np.int64))


def main():
    which = [a for a in sys.argv[1:] if a in ("small", "c2")] or ["small", "c2"]
    if "small" in which:
        small(build_reference(weights.make_state_dict(seed=1234)))
    if "c2" in which:
        c2()
    print("done")


if __name__ == "__main__":
    main()
