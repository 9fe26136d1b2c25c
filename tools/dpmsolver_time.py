"""Developer tool (GPU box): DPM-Solver++ (2M) against DDIM and DDPM at the headline shape (B = 32, L = 196, 1500 audio tokens, 7-way
guidance; bench.py's model and seeded inputs).

For DPM++-20, DDIM-50 and DDPM-1000 on the same inputs: the end-to-end time of ``sample()`` (run set-up, capture, every iteration,
read-back) and, on a separately opened run, the time of the iterations alone (``SamplingRun.steps`` between two device
synchronisations) divided by the iteration count.  One warm-up of each first; medians of REPS repeats (default 5).

Usage:  python tools/dpmsolver_time.py [REPS] [OUT.json]      (default profiles/r07_dpmsolver_time.json)
        python tools/dpmsolver_time.py --one dpmpp20|ddim50       (one sample() of that case: the subject of a kernel-trace run)
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
from convofusion_amd.sampler import SamplingRun, sample  # noqa: E402

KW = dict(num_train_timesteps=1000, beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear")
CASES = [
    ("dpmpp20", lambda: scheduler.DPMSolverMultistepScheduler(**KW), 20),
    ("ddim50", lambda: scheduler.DDIMScheduler(clip_sample=True, **KW), 50),
    ("ddpm1000", lambda: scheduler.DDPMScheduler(variance_type="fixed_small", clip_sample=True, **KW), 1000),
]


def one(name):
    dev = torch.device("cuda", 0)
    model = bench.make_model(dev)
    mems, masks = bench.make_inputs(32, dev, seed=1234)
    make, n = {c[0]: (c[1], c[2]) for c in CASES}[name]
    lat = sample(model, make(), mems, masks, B=32, L=bench.L, num_inference_steps=n, seed=3)
    torch.cuda.synchronize()
    print(name, "finite:", bool(torch.isfinite(lat).all()))


def main():
    if len(sys.argv) > 2 and sys.argv[1] == "--one":
        return one(sys.argv[2])
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 5
    out = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "r07_dpmsolver_time.json")
    dev = torch.device("cuda", 0)
    B = 32
    model = bench.make_model(dev)
    mems, masks = bench.make_inputs(B, dev, seed=1234)
    init = torch.randn((B, bench.L, 128), generator=torch.Generator().manual_seed(7)).to(dev)
    res = {"shape": dict(B=B, L=bench.L, S=list(bench.S), guidance_chunks=7), "reps": reps, "device": torch.cuda.get_device_name(dev)}
    for name, make, n in CASES:
        def once():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            lat = sample(model, make(), mems, masks, B=B, L=bench.L, num_inference_steps=n, init_latents=init, seed=3)
            torch.cuda.synchronize()
            return time.perf_counter() - t0, lat
        _, lat = once()                                   # warm-up
        e2e = [once()[0] for _ in range(reps)]
        per_it = []
        for _ in range(reps + 1):
            with SamplingRun(model, make(), mems, masks, B, bench.L, n, init_latents=init, seed=3) as run:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                run.steps(run.N)
                run.read()
                torch.cuda.synchronize()
                per_it.append((time.perf_counter() - t0) / run.N)
        per_it = per_it[1:]                               # (the first opened run is the warm-up)
        res[name] = dict(iterations=n, end_to_end_s=statistics.median(e2e), end_to_end_all_s=e2e,
                         per_iteration_ms=1e3 * statistics.median(per_it), per_iteration_all_ms=[1e3 * v for v in per_it],
                         finite=bool(torch.isfinite(lat).all()))
        print(f"{name}: end to end {res[name]['end_to_end_s']:.3f} s, {res[name]['per_iteration_ms']:.3f} ms / iteration", flush=True)
    res["dpmpp20_vs_ddim50_per_iteration"] = res["dpmpp20"]["per_iteration_ms"] / res["ddim50"]["per_iteration_ms"]
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", out)


if __name__ == "__main__":
    main()
