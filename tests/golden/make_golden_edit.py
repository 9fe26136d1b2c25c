#!/usr/bin/env python
"""Golden trajectories of the edit loop (token-masked in-painting from a start iteration k0), generated from the REFERENCE ``Denoiser``
(imported from the reference checkout by make_golden.py; build container only -- the tests read the .npz files alone).

The restated edit loop (tests/edit_ref.edit_reverse) drives the reference denoiser.  B = 2 with a different keep mask per utterance,
L = 16, small memories; the source latents are 0.8 x a Philox draw (stream 2), the run's noise Philox stream 1, DDPM step noise Philox
stream 0 at the full-table iteration index.

  traj_edit_hands_ddpm20.npz   : DDPM-20, strength 1 (k0 = 0): the body tokens kept (utterance 1: chunks 0 - 5 only), hands regenerated;
                                 snapshots after 1, 8 and 14 executed iterations
  traj_edit_between_ddpm20.npz : DDPM-20, strength 0.6 (k0 = 8): in-betweening, chunks 0 - 1 and 6 - 7 kept (utterance 1: 0 - 2 and 7);
                                 snapshots after 1, 5 and 9
  traj_edit_dpmpp10.npz        : DPM-Solver++ (2M) 10, strength 0.7 (k0 = 3, a first-order first step): the hands kept (utterance 1:
                                 chunks 2 - 7 only); snapshots after 1, 3 and 5

Each file holds source [B, L, 128], keep [B, L], strength and k0 next to the latents and snapshots.

Usage:  python tests/golden/make_golden_edit.py
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
from oracle import inputs, philox_ref, scheduler_ref, weights  # noqa: E402
from tests import edit_ref  # noqa: E402
from tests.dpmsolver_ref import DPMSolverMultistepRef  # noqa: E402

torch.set_grad_enabled(False)

DPM_KW = dict(num_train_timesteps=1000, beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear")
SEED = 2026
G_SCALE = 7.5


def chunk_mask(chunks, part):
    """[16] keep row: the tokens of `part` (0 body, 1 hands, None both) in the given chunks (token 2c + p)."""
    m = np.zeros((8, 2), dtype=bool)
    for c in chunks:
        if part is None:
            m[c] = True
        else:
            m[c, part] = True
    return m.reshape(16)


CASES = [
    ("hands_ddpm20", "ddpm", 20, 1.0, (1, 8, 14), [chunk_mask(range(8), 0), chunk_mask(range(6), 0)]),
    ("between_ddpm20", "ddpm", 20, 0.6, (1, 5, 9), [chunk_mask((0, 1, 6, 7), None), chunk_mask((0, 1, 2, 7), None)]),
    ("dpmpp10", "dpmpp", 10, 0.7, (1, 3, 5), [chunk_mask(range(8), 1), chunk_mask(range(2, 8), 1)]),
]


def main():
    ref = build_reference(weights.make_state_dict(seed=1234))
    fn = lambda x, t, e, m: ref_forward(ref, x, t, e, m)   # noqa: E731
    B, L, S, pad = 2, 16, (6, 20, 6, 8, 1), (2, 0, 1, 0, 0)
    for k, (name, kind, n, strength, snaps_at, rows) in enumerate(CASES):
        seed = SEED + k
        cb = inputs.make_cfg_batch(seed=seed, B=B, L=L, S=S, pad_tail=pad)
        init = philox_ref.normal_tensor(seed, 0, range(B), 1, L)
        source = (0.8 * philox_ref.normal_tensor(seed, 0, range(B), 2, L)).astype(np.float32)
        keep = np.stack(rows)
        k0 = edit_ref.strength_first_iteration(n, strength)
        sched = DPMSolverMultistepRef(**DPM_KW) if kind == "dpmpp" else scheduler_ref.DDPMSchedulerRef()
        t0 = time.time()
        lat, snaps = edit_ref.edit_reverse(fn, sched, cb["memories"], cb["masks"], init,
                                           lambda i, t: philox_ref.normal_tensor(seed, i, range(B), 0, L), source, keep, k0,
                                           guidance_scale=G_SCALE, num_inference_steps=n, keep_steps=snaps_at)
        print(f"traj_edit_{name}: k0 {k0}, {time.time() - t0:.1f}s |lat| {np.abs(lat).mean():.3f}", flush=True)
        np.savez_compressed(os.path.join(HERE, f"traj_edit_{name}.npz"), latents=lat, source=source, keep=keep.astype(np.uint8),
                            strength=np.float64(strength), k0=np.int64(k0), **{f"step{s}": v for s, v in snaps.items()},
                            meta=np.array([B, L, *S, *pad, n, seed], dtype=np.int64))
    print("done")


if __name__ == "__main__":
    main()
