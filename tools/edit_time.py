"""Developer tool (GPU box): the cost of an edit iteration (cfd_sample_begin_edit: the edit instance of begin_step_kernel reads the keep mask,
the source and the run's noise) against a plain one, in one process, at two shapes with bench.py's model and seeded inputs (DDPM-1000):

  headline   B = 32, L = 196, 1500 audio tokens (bench.py's headline)
  product    B = 32, L = 16 (test.py's batch: 32 utterances x 16 tokens)

Variants: plain (SamplingRun as bench.py opens it), edit (a random half of the tokens kept, strength 1), edit_k0 (the same at strength 0.5:
the run starts at iteration 500).  Per repeat and variant: open a run, WARM iterations, then K iterations timed with the host clock between
two waits for the run's stream (as bench.py and tools/modality_guidance_time.py); the variants alternate within every repeat; medians of
REPS repeats.

Usage:  python tools/edit_time.py [REPS] [OUT.json]      (default 5, profiles/r09_edit_time.json)
"""
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from convofusion_amd import scheduler  # noqa: E402
from convofusion_amd.sampler import SamplingRun  # noqa: E402

B, N, WARM = 32, 1000, 5
SHAPES = [("headline", 196, 50), ("product", 16, 200)]     # (name, L, timed iterations K)


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 5
    out = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "r09_edit_time.json")
    dev = torch.device("cuda", 0)
    model = bench.make_model(dev)
    mems, masks = bench.make_inputs(B, dev, seed=1234)
    sch = scheduler.DDPMScheduler(num_train_timesteps=1000, beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear",
                                  variance_type="fixed_small", clip_sample=True)
    g = torch.Generator().manual_seed(5)
    res = {"reps": reps, "warm_iterations": WARM, "iterations": N, "device": torch.cuda.get_device_name(dev), "scheduler": "DDPM",
           "memories": list(bench.S), "timer": "host clock between two waits for the run's stream (as bench.py); variants alternate within "
           "each repeat"}
    for shape, L, K in SHAPES:
        src = torch.randn((B, L, 128), generator=g).to(dev)
        keep = (torch.rand((B, L), generator=g) < 0.5).to(dev)
        variants = [("plain", {}), ("edit", dict(source_latents=src, keep_mask=keep)),
                    ("edit_k0", dict(source_latents=src, keep_mask=keep, strength=0.5))]
        times = {name: [] for name, _ in variants}
        for rep in range(reps + 1):                       # repeat 0: warm-up of every variant, not counted
            for name, kw in variants:
                with SamplingRun(model, sch, mems, masks, B, L, N, guidance_scale=7.5, seed=0, **kw) as run:
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
                print(f"{shape} repeat {rep}: " + ", ".join(f"{n} {times[n][-1]:.4f}" for n in times) + " ms / iteration", flush=True)
        base = statistics.median(times["plain"])
        res[shape] = {"B": B, "L": L, "timed_iterations": K}
        for name, _ in variants:
            med = statistics.median(times[name])
            res[shape][name] = dict(ms_per_iteration=med, ms_per_iteration_all=times[name], vs_plain=med / base)
            print(f"{shape} {name}: {med:.4f} ms / iteration ({med / base:.4f} of plain)")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", out)


if __name__ == "__main__":
    main()
