"""Developer tool (GPU box): what the edit-friendly DDPM inversion costs, in one process, at the product shape (L = 16, bench.py's model,
seeded inputs and memory lengths 24 / 161 / 24 / 8 / 1), N = 1000, INVERSION_WEIGHTS (2 of the 7 chunks evaluated), 1 and 8 utterances.

  invert          ``invert_ddpm`` end to end (host clock around the call; the call ends in its own wait), with levels_per_batch from the
                  default budget and at the values LEVELS, and per level batch (seconds / ceil(N / J))
  sequential      the comparison point: a plain ``sample()`` of N = 1000 with the same rows and weights -- what any inversion of N
                  DEPENDENT evaluations must at least cost.  Taken at THIS commit; the plain run's kernels are instruction for
                  instruction those of the commit before the feature (tools/isa_same.py: profiles/r13_ddpm_inversion_isa_same.txt).
                  PARENT.json (optional): {"1": {"seconds": ..}, "8": {..}} of the same call timed in a checkout of that commit on the
                  same box, in the same job; stored next to it as sequential_sample_parent
  per iteration   a replay run (``SamplingRun(noise_space=)``, operands 0) against a plain DDPM run of the same rows (operands 0), K
                  iterations between two waits for the run's stream (as bench.py)

The variants alternate within every repeat; medians of REPS repeats; repeat 0 warms every variant up and is not counted.

Usage:  python tools/ddpm_inversion_time.py [REPS] [OUT.json] [PARENT.json]      (default 5, profiles/r13_ddpm_inversion_time.json)
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
from convofusion_amd.sampler import INVERSION_WEIGHTS, SamplingRun, invert_ddpm, sample  # noqa: E402

L, N, WARM, K = 16, 1000, 5, 200
PRODUCT_S = (24, 161, 24, 8, 1)
UTTERANCES = (1, 8)
LEVELS = (8, 40, 100)


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 5
    out = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "r13_ddpm_inversion_time.json")
    parent = json.load(open(sys.argv[3])) if len(sys.argv) > 3 else {}
    dev = torch.device("cuda", 0)
    bench.S = PRODUCT_S
    model = bench.make_model(dev)
    sch = scheduler.DDPMScheduler(num_train_timesteps=1000, beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear",
                                  variance_type="fixed_small", clip_sample=True)
    res = {"reps": reps, "iterations": N, "L": L, "device": torch.cuda.get_device_name(dev), "scheduler": "DDPM", "memories": list(PRODUCT_S),
           "weights": "INVERSION_WEIGHTS (2 chunks evaluated)", "timer": "host clock; variants alternate within each repeat; repeat 0 not counted",
           "utterances": {}}
    for B in UTTERANCES:
        mems, masks = bench.make_inputs(B, dev, seed=1234)
        src = 0.8 * torch.randn((B, L, 128), device=dev, generator=torch.Generator(dev).manual_seed(1))
        kw = dict(source_latents=src, num_inference_steps=N, seed=0)
        ways = [("invert_default", lambda: invert_ddpm(model, sch, mems, masks, **kw))]
        ways += [(f"invert_J{J}", (lambda J: lambda: invert_ddpm(model, sch, mems, masks, levels_per_batch=J, **kw))(J)) for J in LEVELS]
        ways.append(("sequential_sample", lambda: sample(model, sch, mems, masks, B=B, L=L, num_inference_steps=N, guidance_scale=1.0,
                                                         modality_weights=INVERSION_WEIGHTS, seed=0)))
        secs, used = {n: [] for n, _ in ways}, {}
        space = None
        for rep in range(reps + 1):
            for name, fn in ways:
                torch.cuda.synchronize(dev)
                t0 = time.perf_counter()
                r = fn()
                torch.cuda.synchronize(dev)
                dt = time.perf_counter() - t0
                if name.startswith("invert"):
                    used[name] = invert_ddpm.last["levels_per_batch"]
                    assert torch.isfinite(r[1]).all(), name
                    space = r
                if rep > 0:
                    secs[name].append(dt)
            if rep > 0:
                print(f"B={B} repeat {rep}: " + ", ".join(f"{n} {secs[n][-1]:.3f}" for n in secs) + " s", flush=True)
        seq = statistics.median(secs["sequential_sample"])
        entry = {"sequential_sample": dict(seconds=seq, seconds_all=secs["sequential_sample"])}
        if str(B) in parent:
            entry["sequential_sample_parent"] = parent[str(B)]
            print(f"B={B} sequential run: {seq:.3f} s here, {parent[str(B)]['seconds']:.3f} s in the parent checkout")
        for name, _ in ways[:-1]:
            med, J = statistics.median(secs[name]), used[name]
            nb = -(-N // J)
            entry[name] = dict(seconds=med, seconds_all=secs[name], levels_per_batch=J, batches=nb, ms_per_batch=1e3 * med / nb,
                               vs_sequential=med / seq)
            print(f"B={B} {name}: {med:.3f} s (J = {J}, {1e3 * med / nb:.2f} ms / batch; {med / seq:.3f} of the sequential run's {seq:.3f} s)")
        variants = [("plain", dict(seed=0)), ("replay", dict(noise_space=space))]
        it = {n: [] for n, _ in variants}
        for rep in range(reps + 1):
            for name, vkw in variants:
                with SamplingRun(model, sch, mems, masks, B, L, N, guidance_scale=1.0, modality_weights=INVERSION_WEIGHTS, operands=0,
                                 **vkw) as run:
                    run.steps(WARM)
                    run.read()
                    t0 = time.perf_counter()
                    run.steps(K)
                    lat = run.read()
                    dt = time.perf_counter() - t0
                    assert torch.isfinite(lat).all(), name
                if rep > 0:
                    it[name].append(1e3 * dt / K)
        base = statistics.median(it["plain"])
        entry["per_iteration"] = {n: dict(ms_per_iteration=statistics.median(it[n]), ms_per_iteration_all=it[n],
                                          vs_plain=statistics.median(it[n]) / base) for n, _ in variants}
        print(f"B={B} per iteration: plain {base:.4f} ms, replay {statistics.median(it['replay']):.4f} ms")
        res["utterances"][str(B)] = entry
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", out)


if __name__ == "__main__":
    main()
