#!/usr/bin/env python
"""Heavy-tailed stress weights at the HEADLINE shape, 50 guided DDPM steps, from the REFERENCE itself (build container only):
tests/golden/heavy_c2_ddpm50.npz.  The trajectory part of make_golden_heavy_c2.py with the DDPM scheduler -- the regime where the DDPM
runs' default operand policy (single-fp16 attention against the audio memory) is 2.9e-3 off -- for the attention-concentration census
and ``operands="auto"``:

  traj_step{1,25,50}  (and latents, [L, 1, 128]: the final ones) the restated loop driving the REFERENCE denoiser for utterance 5 alone (outlier factor 8, outlier-token memories of
                      make_golden_heavy_c2.heavy_batch), Philox step noise of global utterance 5: pins row 5 of the B = 32 HIP loop
  peak_it{0,25,49}    the numpy oracle's largest audio-attention probability per layer (over the 7 guidance rows and 196 queries) at
                      those iterations of the ORACLE's own trajectory: what the census of a run on these inputs measures
The oracle-vs-reference distance of the two trajectories is printed: the loop's conditioning on record.
Usage:  python tests/golden/make_golden_heavy_c2_ddpm.py"""
import os
import sys
import time

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
from make_golden import build_reference, ref_forward, rel  # noqa: E402
from make_golden_c2rows import utterance_rows  # noqa: E402
from make_golden_heavy_c2 import B, L, S, PAD, SEED, U, heavy_batch  # noqa: E402

from oracle import denoiser_ref, philox_ref, sampler_ref, scheduler_ref, weights  # noqa: E402

torch.set_grad_enabled(False)
N, KEEP, PEAK_AT, GAIN = 50, (1, 25, 50), (0, 25, 49), 8.0


def main():
    cb = heavy_batch()
    mems, masks = utterance_rows(cb, U)
    init = philox_ref.normal_tensor(SEED, 0, [U], 1, L)
    noise = lambda i, t: philox_ref.normal_tensor(SEED, i, [U], 0, L)   # noqa: E731
    ref8 = build_reference(weights.make_state_dict_heavy(seed=777, gain=GAIN), mem_len=1536)
    t0 = time.time()
    lat, snaps, _ = sampler_ref.diffusion_reverse(
        lambda xx, t, e, mk: ref_forward(ref8, xx, t, e, mk), scheduler_ref.DDPMSchedulerRef(), mems, masks, init, noise,
        guidance_scale=7.5, num_inference_steps=N, keep_steps=KEEP)
    print(f"reference trajectory: {time.time() - t0:.0f}s")
    sd8 = weights.extend_pe(weights.make_state_dict_heavy(seed=777, gain=GAIN), 1536)
    calls, peaks = [0], {}

    def oracle(xx, t, e, mk):
        out, att = denoiser_ref.denoiser_forward(sd8, xx, t, e, mk)
        if calls[0] in PEAK_AT:
            peaks[f"peak_it{calls[0]}"] = att[1].max(axis=(0, 2, 3)).astype(np.float32)   # memory 1: the audio memory
        calls[0] += 1
        return out, att
    _, s_orc, _ = sampler_ref.diffusion_reverse(oracle, scheduler_ref.DDPMSchedulerRef(), mems, masks, init, noise,
                                                guidance_scale=7.5, num_inference_steps=N, keep_steps=KEEP)
    print(f"oracle trajectory: {time.time() - t0:.0f}s; numpy oracle vs torch reference (both float32) after "
          + ", ".join(f"{k}: {rel(s_orc[k], snaps[k]):.1e}" for k in KEEP) + " steps")
    for k, v in sorted(peaks.items()):
        print(k, "per layer:", " ".join(f"{p:.3f}" for p in v))
    out = {f"traj_step{k}": v for k, v in snaps.items()}
    out["latents"] = lat
    out.update(peaks)
    out["meta"] = np.array([B, L, *S, *PAD, N, SEED, U], dtype=np.int64)
    np.savez_compressed(os.path.join(HERE, "heavy_c2_ddpm50.npz"), **out)
    print("wrote heavy_c2_ddpm50.npz")


if __name__ == "__main__":
    main()
