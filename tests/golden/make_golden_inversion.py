#!/usr/bin/env python
"""Golden trajectories of DDIM inversion and of the anchored DDIM regeneration, generated from the REFERENCE ``Denoiser`` (imported from
the reference checkout by make_golden.py; build container only -- the tests read the .npz files alone).

The restated loops (tests/inversion_ref) drive the reference denoiser.  B = 2, L = 16, small memories, 7-way guidance batch; the
source latents are 0.8 x a Philox draw (stream 2).  The inversion guides with the conditional prediction alone (w_all = 1 at guidance
scale 1); the regeneration runs under another conditioning batch with the reference's combine at guidance scale 7.5.

  traj_invert_ddim10.npz   : N = 10 inversion: the whole trajectory [11, B, L, 128]
  traj_invert_ddim50.npz   : N = 50 inversion: trajectory slots 1, 10, 25, 40 and 50
  traj_anchored_ddim10.npz : the N = 10 regeneration from traj_invert_ddim10's ring under the target conditioning, a partial keep mask
                             (utterance 0: the body tokens; utterance 1: chunks 0 - 1 and 6 - 7); snapshots after 1, 5 and 10

Usage:  python tests/golden/make_golden_inversion.py
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
from tests import inversion_ref  # noqa: E402

torch.set_grad_enabled(False)

SEED = 3031
B, L, S, PAD = 2, 16, (6, 20, 6, 8, 1), (2, 0, 1, 0, 0)
SNAPS50 = (1, 10, 25, 40, 50)


def keep_rows():
    body = np.zeros((8, 2), bool)
    body[:, 0] = True
    ends = np.zeros((8, 2), bool)
    ends[[0, 1, 6, 7]] = True
    return np.stack([body.reshape(16), ends.reshape(16)])


def main():
    ref = build_reference(weights.make_state_dict(seed=1234))
    fn = lambda x, t, e, m: ref_forward(ref, x, t, e, m)   # noqa: E731
    src_cb = inputs.make_cfg_batch(seed=SEED, B=B, L=L, S=S, pad_tail=PAD)
    tgt_cb = inputs.make_cfg_batch(seed=SEED + 1, B=B, L=L, S=S, pad_tail=PAD)
    source = (0.8 * philox_ref.normal_tensor(SEED, 0, range(B), 2, L)).astype(np.float32)
    meta = np.array([B, L, *S, *PAD, SEED], dtype=np.int64)
    rings = {}
    for n in (10, 50):
        t0 = time.time()
        lat, ring = inversion_ref.invert(fn, inversion_ref.DDIMInverseRef(), src_cb["memories"], src_cb["masks"], source, n,
                                         factors=inversion_ref.factor_table(inversion_ref.COND_ONLY, 1.0, n, B))
        rings[n] = ring
        print(f"traj_invert_ddim{n}: {time.time() - t0:.1f}s |lat| {np.abs(lat).mean():.3f}", flush=True)
        slots = range(n + 1) if n == 10 else SNAPS50
        np.savez_compressed(os.path.join(HERE, f"traj_invert_ddim{n}.npz"), latents=lat, source=source, n=np.int64(n),
                            **{f"slot{j}": ring[j] for j in slots}, meta=meta)
    keep = keep_rows()
    t0 = time.time()
    lat, snaps = inversion_ref.anchored_reverse(fn, scheduler_ref.DDIMSchedulerRef(clip_sample=False), tgt_cb["memories"], tgt_cb["masks"],
                                                rings[10], keep, 10, guidance_scale=7.5, keep_steps=(1, 5, 10))
    print(f"traj_anchored_ddim10: {time.time() - t0:.1f}s |lat| {np.abs(lat).mean():.3f}", flush=True)
    np.savez_compressed(os.path.join(HERE, "traj_anchored_ddim10.npz"), latents=lat, keep=keep.astype(np.uint8), n=np.int64(10),
                        **{f"step{s}": v for s, v in snaps.items()}, meta=np.array([B, L, *S, *PAD, SEED + 1], dtype=np.int64))
    print("done")


if __name__ == "__main__":
    main()
