#!/usr/bin/env python
"""Golden trajectories of the tied loop (long-form synthesis: half-overlapping windows as rows of one run), generated from the REFERENCE
``Denoiser`` (imported from the reference checkout by make_golden.py; build container only -- the tests read the .npz files alone).

The restated tied loop (tests/longform_ref.tied_reverse) drives the reference denoiser.  L = 16, small memories that differ per row; the
tie table is ``convofusion_amd.longform.window_ties`` (token l < 8 of window w > 0 tied to token l + 8 of window w - 1); a row's noise is
Philox on its global row index u * W + w (stream 1 the initial draw, stream 0 the DDPM step noise).  Snapshots are the latents as the
scheduler step left them; `latents` has the final copy.

  traj_longform_ddpm20.npz       : U = 2 utterances x W = 3 windows = 6 rows, DDPM-20; snapshots after 1, 8 and 14 iterations
  traj_longform_dpmpp10.npz      : the same rows, DPM-Solver++ (2M) 10; snapshots after 1, 3 and 5
  traj_longform_carry_ddim10.npz : U = 1, W = 4 in two runs of 2 windows (max_rows = 2), DDIM-10: window 1 tied to window 0; window 2
                                   keeps its first 8 tokens from the finished last 8 of window 1 (source / keep of the edit), window 3 tied
                                   to window 2.  Per run g: tie{g}, keep{g}, source{g}, step{k}_{g}, latents{g}; `latents` = all 4 rows.

Usage:  python tests/golden/make_golden_longform.py
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
from convofusion_amd.longform import group_ties, window_groups, window_ties  # noqa: E402
from oracle import inputs, philox_ref, scheduler_ref, weights  # noqa: E402
from tests import longform_ref  # noqa: E402
from tests.dpmsolver_ref import DPMSolverMultistepRef  # noqa: E402

torch.set_grad_enabled(False)

DPM_KW = dict(num_train_timesteps=1000, beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear")
SEED = 2031
G_SCALE = 7.5
L, S, PAD = 16, (6, 20, 6, 8, 1), (2, 0, 1, 0, 0)


def rows_of(cb, start, stop, B):
    """Rows [start, stop) of a chunk-major guidance batch (memories and masks)."""
    cut = lambda x: None if x is None else np.ascontiguousarray(x.reshape(7, B, *x.shape[1:])[:, start:stop].reshape(7 * (stop - start), *x.shape[1:]))  # noqa: E731
    return [cut(m) for m in cb["memories"]], {k: cut(v) for k, v in cb["masks"].items()}


def main():
    ref = build_reference(weights.make_state_dict(seed=1234))
    fn = lambda x, t, e, m: ref_forward(ref, x, t, e, m)   # noqa: E731
    for k, (name, kind, n, snaps_at) in enumerate([("ddpm20", "ddpm", 20, (1, 8, 14)), ("dpmpp10", "dpmpp", 10, (1, 3, 5))]):
        U, W, seed = 2, 3, SEED + k
        B = U * W
        cb = inputs.make_cfg_batch(seed=seed, B=B, L=L, S=S, pad_tail=PAD)
        tie = window_ties(U, W, L).numpy()
        sched = DPMSolverMultistepRef(**DPM_KW) if kind == "dpmpp" else scheduler_ref.DDPMSchedulerRef()
        t0 = time.time()
        lat, snaps = longform_ref.tied_reverse(fn, sched, cb["memories"], cb["masks"], philox_ref.normal_tensor(seed, 0, range(B), 1, L),
                                               lambda i, t: philox_ref.normal_tensor(seed, i, range(B), 0, L), tie,
                                               guidance_scale=G_SCALE, num_inference_steps=n, keep_steps=snaps_at)
        print(f"traj_longform_{name}: {time.time() - t0:.1f}s |lat| {np.abs(lat).mean():.3f}", flush=True)
        np.savez_compressed(os.path.join(HERE, f"traj_longform_{name}.npz"), latents=lat, tie=tie.astype(np.int32),
                            **{f"step{s}": v for s, v in snaps.items()}, meta=np.array([U, W, L, *S, *PAD, n, seed], dtype=np.int64))

    U, W, n, seed, max_rows, snaps_at = 1, 4, 10, SEED + 2, 2, (1, 3, 5)
    B = U * W
    cb = inputs.make_cfg_batch(seed=seed, B=B, L=L, S=S, pad_tail=PAD)
    out = np.zeros((B, L, 128), dtype=np.float32)
    files = {}
    for g, (start, stop) in enumerate(window_groups(U, W, max_rows)):
        tie, carried = (x.numpy() for x in group_ties(start, stop, W, L))
        source = np.zeros((stop - start, L, 128), dtype=np.float32)
        for b in range(stop - start):
            if carried[b].any():
                source[b, :L // 2] = out[start + b - 1, L // 2:]
        mems, masks = rows_of(cb, start, stop, B)
        lat, snaps = longform_ref.tied_reverse(fn, scheduler_ref.DDIMSchedulerRef(), mems, masks,
                                               philox_ref.normal_tensor(seed, 0, range(start, stop), 1, L), lambda i, t: None, tie,
                                               source=source, keep=carried, guidance_scale=G_SCALE, num_inference_steps=n,
                                               keep_steps=snaps_at)
        out[start:stop] = lat
        files.update({f"tie{g}": tie.astype(np.int32), f"keep{g}": carried.astype(np.uint8), f"source{g}": source, f"latents{g}": lat,
                      **{f"step{s}_{g}": v for s, v in snaps.items()}})
    print(f"traj_longform_carry_ddim10: |lat| {np.abs(out).mean():.3f}", flush=True)
    np.savez_compressed(os.path.join(HERE, "traj_longform_carry_ddim10.npz"), latents=out, max_rows=np.int64(max_rows), **files,
                        meta=np.array([U, W, L, *S, *PAD, n, seed], dtype=np.int64))
    print("done")


if __name__ == "__main__":
    main()
