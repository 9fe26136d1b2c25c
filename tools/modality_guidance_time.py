"""Developer tool (GPU box): per-modality guidance weights at the headline shape (B = 32, L = 196, 1500 audio tokens, DDPM-1000; bench.py's
model and seeded inputs), in one process:

  default          today's path as bench.py runs it: SamplingRun() with the reference's weights, 7 chunks evaluated
  default_skip     the same with skip_zero_weight_chunks=True (6 chunks): what the weighted path is bit-identical to
  weighted_ref     modality_weights = the reference's 1, 1, 1, 1, 1, 0 (cfd_sample_begin_weighted; pruned to 6 chunks)
  text_audio       modality_weights = text 1, audio 1, all others 0 (pruned to 3 chunks)
  interval         the reference's weights inside iterations [0.3 N, 0.7 N), 0 outside ([N, 1, 6]; 6 chunks evaluated)

Per repeat and variant: open a run, WARM iterations, then K iterations timed with the host clock between two waits for the run's stream
(the captured iteration replays on the library's own stream, which torch's events cannot bracket; bench.py times the same way, and at K = 50
iterations of ~12 ms the wait's few microseconds are far below the run-to-run spread).  The variants alternate within every repeat; medians
of REPS repeats.

Usage:  python tools/modality_guidance_time.py [REPS] [OUT.json]      (default 5, profiles/r08_modality_guidance_time.json)
"""
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from convofusion_amd import scheduler  # noqa: E402
from convofusion_amd.sampler import REFERENCE_MODALITY_WEIGHTS, SamplingRun  # noqa: E402

B, N, WARM, K = 32, 1000, 5, 50


def variants():
    ref = np.array([1.0, 1, 1, 1, 1, 0])
    interval = np.zeros((N, 1, 6))
    interval[int(np.ceil(0.3 * N)):int(np.ceil(0.7 * N)), 0] = ref
    return [
        ("default", {}),
        ("default_skip", dict(skip_zero_weight_chunks=True)),
        ("weighted_ref", dict(modality_weights=dict(REFERENCE_MODALITY_WEIGHTS))),
        ("text_audio", dict(modality_weights=dict(text=1, audio=1, spk=0, apb=0, lsnid=0, all=0))),
        ("interval", dict(modality_weights=interval)),
    ]


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 5
    out = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "r08_modality_guidance_time.json")
    dev = torch.device("cuda", 0)
    model = bench.make_model(dev)
    mems, masks = bench.make_inputs(B, dev, seed=1234)
    sch = scheduler.DDPMScheduler(num_train_timesteps=1000, beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear",
                                  variance_type="fixed_small", clip_sample=True)
    times = {name: [] for name, _ in variants()}
    chunks = {}
    for rep in range(reps + 1):                           # repeat 0: warm-up of every variant, not counted
        for name, kw in variants():
            with SamplingRun(model, sch, mems, masks, B, bench.L, N, guidance_scale=7.5, seed=0, **kw) as run:
                chunks[name] = run.chunks_evaluated
                run.steps(WARM)
                run.read()
                t0 = time.perf_counter()
                run.steps(K)
                lat = run.read()
                dt = time.perf_counter() - t0
                assert torch.isfinite(lat).all(), name
            if rep > 0:
                times[name].append(1e3 * dt / K)
        if rep > 0:
            print(f"repeat {rep}: " + ", ".join(f"{n} {times[n][-1]:.3f}" for n in times) + " ms / iteration", flush=True)
    base = statistics.median(times["default"])
    res = {"shape": dict(B=B, L=bench.L, S=list(bench.S), scheduler="DDPM", iterations=N), "reps": reps, "warm_iterations": WARM,
           "timed_iterations": K, "device": torch.cuda.get_device_name(dev),
           "timer": "host clock between two waits for the run's stream (as bench.py); variants alternate within each repeat"}
    for name, _ in variants():
        med = statistics.median(times[name])
        res[name] = dict(chunks_evaluated=chunks[name], ms_per_iteration=med, ms_per_iteration_all=times[name], vs_default=med / base)
        print(f"{name}: {chunks[name]} chunks, {med:.3f} ms / iteration ({med / base:.3f} of default)")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", out)


if __name__ == "__main__":
    main()
