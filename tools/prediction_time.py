"""Developer tool (GPU box): what an iteration of a ``prediction_type="sample"`` DDPM run costs against an epsilon DDPM run of the same
build -- the same rows, both on ``operands=0`` (split pairs), so that the only difference is the instance of cfg_step_kernel.  Shapes:
the headline shape (B = 32, L = 196, 1500 audio tokens; bench.py's model and seeded inputs) and the product shape (L = 16, memories
(24, 161, 24, 8, 1)) with one and with eight utterances.

Per repeat and variant: open a run, WARM iterations, then K iterations timed with the host clock between two waits for the run's stream
(as tools/modality_guidance_time.py).  The variants alternate within every repeat; repeat 0 is a warm-up; medians of REPS repeats, and the
spread (max - min over the repeats) of each variant next to them: the margin the two medians are compared with.

Usage:  python tools/prediction_time.py [REPS] [OUT.json]      (default 5, profiles/r19_prediction_time.json)
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

KW = dict(num_train_timesteps=1000, beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear", variance_type="fixed_small",
          clip_sample=True)
# (name, B, L, memories, warm iterations, timed iterations)
SHAPES = [("headline", 32, 196, (32, 1500, 32, 8, 1), 5, 50), ("product_b1", 1, 16, (24, 161, 24, 8, 1), 20, 400),
          ("product_b8", 8, 16, (24, 161, 24, 8, 1), 20, 400)]
VARIANTS = ("epsilon", "sample")


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 5
    out = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "r19_prediction_time.json")
    dev = torch.device("cuda", 0)
    model = bench.make_model(dev)
    res = {"reps": reps, "device": torch.cuda.get_device_name(dev), "scheduler": "DDPM-1000", "operands": 0,
           "timer": "host clock between two waits for the run's stream (as bench.py); variants alternate within each repeat"}
    for name, B, L, S, warm, K in SHAPES:
        bench.S = S
        mems, masks = bench.make_inputs(B, dev, seed=1234)
        times = {v: [] for v in VARIANTS}
        for rep in range(reps + 1):
            for v in VARIANTS:
                with SamplingRun(model, scheduler.DDPMScheduler(prediction_type=v, **KW), mems, masks, B, L, 1000, guidance_scale=7.5, seed=0,
                                 operands=0) as run:
                    run.steps(warm)
                    run.read()
                    t0 = time.perf_counter()
                    run.steps(K)
                    lat = run.read()
                    dt = time.perf_counter() - t0
                    assert torch.isfinite(lat).all(), (name, v)
                if rep > 0:
                    times[v].append(1e3 * dt / K)
        med = {v: statistics.median(times[v]) for v in VARIANTS}
        res[name] = dict(B=B, L=L, S=list(S), warm_iterations=warm, timed_iterations=K, sample_vs_epsilon=med["sample"] / med["epsilon"],
                         **{v: dict(ms_per_iteration=med[v], ms_per_iteration_all=times[v], spread_ms=max(times[v]) - min(times[v]))
                            for v in VARIANTS})
        print(f"{name}: epsilon {med['epsilon']:.4f} ms, sample {med['sample']:.4f} ms / iteration ({med['sample'] / med['epsilon']:.4f}); "
              f"spread {res[name]['epsilon']['spread_ms']:.4f} / {res[name]['sample']['spread_ms']:.4f} ms", flush=True)
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", out)


if __name__ == "__main__":
    main()
