"""Developer tool (GPU box): the cost of DDIM inversion iterations (scheduler kind 3, with and without the trajectory ring) and of an
anchored iteration (cfd_sample_begin_anchored) against a plain DDIM iteration and a plain edit iteration, in one process, at two shapes with
bench.py's model and seeded inputs (N = 50):

  headline   B = 32, L = 196, 1500 audio tokens (bench.py's headline)
  product    B = 32, L = 16 (test.py's batch: 32 utterances x 16 tokens)

Variants: ddim (the reference's guidance, DDIMScheduler), invert / invert_ring (DDIMInverseScheduler with the same guidance, without and
with the trajectory), edit (DDIMScheduler with a random half of the tokens kept, strength 1), anchored (the same mask anchored to a
trajectory).  Every variant evaluates the same chunks (the reference's guidance with the zero-weight chunk skipped), so the differences are
the step's extra store and the kept-token reads.  Per repeat and variant: open a run, WARM iterations, then K iterations timed with the
host clock between two waits for the run's stream (as bench.py and tools/edit_time.py); the variants alternate within every repeat;
medians of REPS repeats.

Usage:  python tools/inversion_time.py [REPS] [OUT.json]      (default 5, profiles/r10_inversion_time.json)
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

B, N, WARM = 32, 50, 3
SHAPES = [("headline", 196, 40), ("product", 16, 40)]     # (name, L, timed iterations K)
SCHED_KW = dict(num_train_timesteps=1000, beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear", clip_sample=False)


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 5
    out = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "r10_inversion_time.json")
    dev = torch.device("cuda", 0)
    model = bench.make_model(dev)
    mems, masks = bench.make_inputs(B, dev, seed=1234)
    ddim = scheduler.DDIMScheduler(**SCHED_KW)
    inv = scheduler.DDIMInverseScheduler(**SCHED_KW)
    g = torch.Generator().manual_seed(5)
    res = {"reps": reps, "warm_iterations": WARM, "iterations": N, "device": torch.cuda.get_device_name(dev),
           "memories": list(bench.S), "guidance": "reference combine at 7.5, zero-weight chunk skipped (6 of 7 chunks)",
           "timer": "host clock between two waits for the run's stream (as bench.py); variants alternate within each repeat"}
    for shape, L, K in SHAPES:
        src = torch.randn((B, L, 128), generator=g).to(dev)
        keep = (torch.rand((B, L), generator=g) < 0.5).to(dev)
        ring = torch.randn((N + 1, B, L, 128), generator=g).to(dev)
        variants = [("ddim", ddim, dict(init_latents=src)), ("invert", inv, dict(init_latents=src)),
                    ("invert_ring", inv, dict(init_latents=src, trajectory=True)),
                    ("edit", ddim, dict(source_latents=src, keep_mask=keep)),
                    ("anchored", ddim, dict(init_latents=src, anchor_trajectory=ring, keep_mask=keep))]
        times = {name: [] for name, _, _ in variants}
        for rep in range(reps + 1):                       # repeat 0: warm-up of every variant, not counted
            for name, sch, kw in variants:
                with SamplingRun(model, sch, mems, masks, B, L, N, guidance_scale=7.5, seed=0, skip_zero_weight_chunks=True, **kw) as run:
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
        res[shape] = {"B": B, "L": L, "timed_iterations": K, "ring_bytes": 4 * (N + 1) * B * L * 128,
                      "ring_bytes_written_per_iteration": 4 * B * L * 128}
        for name, _, _ in variants:
            med = statistics.median(times[name])
            base = statistics.median(times["edit" if name == "anchored" else "ddim"])
            res[shape][name] = dict(ms_per_iteration=med, ms_per_iteration_all=times[name],
                                    vs=("edit" if name == "anchored" else "ddim"), ratio=med / base)
            print(f"{shape} {name}: {med:.4f} ms / iteration ({med / base:.4f} of {'edit' if name == 'anchored' else 'ddim'})")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", out)


if __name__ == "__main__":
    main()
