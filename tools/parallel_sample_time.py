"""Developer tool (GPU box): what parallel-in-time DDPM sampling costs and how its Picard sweeps converge, in one process, at the product
shape (L = 16, bench.py's model with its seeded weights, seeded inputs and memory lengths 24 / 161 / 24 / 8 / 1), DDPM-1000, the
reference's guidance (scale 7.5, 6 of the 7 chunks evaluated), 1 and 8 utterances.

  sequential      the comparison point, not the code under test: a plain ``sample()`` with the same rows, initial latents and step noise on
                  split-pair operands (operands=0).  Its kernels are instruction for instruction those of the commit before the feature
                  (tools/isa_same.py: profiles/r14_parallel_sample_isa_same.txt)
  parallel        ``sample_parallel`` end to end at tolerance tau in TAUS, with levels_per_batch from the default budget and at the values
                  LEVELS: sweeps, mean stride, seconds, ms per sweep, and the relative L2 of the final latents from the sequential run

The variants alternate within every repeat; medians of REPS repeats; repeat 0 warms every variant up and is not counted.  Host clock
between two waits for the stream.  The seeded weights are no trained checkpoint: sample quality at tau > 0 is not measured here.

Usage:  python tools/parallel_sample_time.py [REPS] [OUT.json] [UTTERANCES,..]      (default 5, profiles/r14_parallel_sample_time.json, 1,8)
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
from convofusion_amd.sampler import sample, sample_parallel  # noqa: E402

L, N = 16, 1000
PRODUCT_S = (24, 161, 24, 8, 1)
TAUS = (0.0, 0.05, 0.1, 0.2, 0.5)
LEVELS = {1: (None, 16, 48), 8: (None, 8, 16)}     # None: the default budget


def rel_l2(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 5
    out = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "r14_parallel_sample_time.json")
    utterances = tuple(int(v) for v in sys.argv[3].split(",")) if len(sys.argv) > 3 else (1, 8)
    dev = torch.device("cuda", 0)
    bench.S = PRODUCT_S
    model = bench.make_model(dev)
    sch = scheduler.DDPMScheduler(num_train_timesteps=1000, beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear",
                                  variance_type="fixed_small", clip_sample=True)
    res = json.load(open(out)) if os.path.exists(out) else {}     # (one shape per call: the other's entry is kept)
    res = {**res, "reps": reps, "iterations": N, "L": L, "device": torch.cuda.get_device_name(dev), "scheduler": "DDPM", "memories": list(PRODUCT_S),
           "guidance": "reference (scale 7.5, 6 chunks evaluated)", "weights": "seeded (bench.py), no trained checkpoint",
           "timer": "host clock between two stream waits; variants alternate within each repeat; repeat 0 not counted",
           "utterances": dict(res.get("utterances", {}))}
    for B in utterances:
        mems, masks = bench.make_inputs(B, dev, seed=1234)
        gen = torch.Generator(dev).manual_seed(1)
        init = torch.randn((B, L, 128), device=dev, generator=gen)
        noise = torch.randn((N, B, L, 128), device=dev, generator=gen)
        kw = dict(B=B, L=L, num_inference_steps=N, guidance_scale=7.5, init_latents=init, step_noise=noise)
        ways = [("sequential", lambda: (sample(model, sch, mems, masks, operands=0, skip_zero_weight_chunks=True, **kw), None))]
        for J in LEVELS.get(B, (None,)):
            for tau in TAUS:
                ways.append((f"parallel_J{J or 'default'}_tau{tau:g}",
                             (lambda J, tau: lambda: sample_parallel(model, sch, mems, masks, tolerance=tau, levels_per_batch=J, **kw))(J, tau)))
        secs, last = {n: [] for n, _ in ways}, {}
        for rep in range(reps + 1):
            for name, fn in ways:
                torch.cuda.synchronize(dev)
                t0 = time.perf_counter()
                r = fn()
                torch.cuda.synchronize(dev)
                dt = time.perf_counter() - t0
                assert torch.isfinite(r[0]).all(), name
                last[name] = r
                if rep > 0:
                    secs[name].append(dt)
            if rep > 0:
                print(f"B={B} repeat {rep}: " + ", ".join(f"{n} {secs[n][-1]:.3f}" for n in secs) + " s", flush=True)
        seq = statistics.median(secs["sequential"])
        want = last["sequential"][0]
        entry = {"sequential": dict(seconds=seq, seconds_all=secs["sequential"])}
        for name, _ in ways[1:]:
            lat, st = last[name]
            med = statistics.median(secs[name])
            entry[name] = dict(seconds=med, seconds_all=secs[name], levels_per_batch=st.levels_per_batch, sweeps=st.sweeps,
                               mean_stride=N / st.sweeps, ms_per_sweep=1e3 * med / st.sweeps, vs_sequential=med / seq,
                               rel_l2_vs_sequential=rel_l2(lat, want))
            print(f"B={B} {name}: J = {st.levels_per_batch}, {st.sweeps} sweeps (mean stride {N / st.sweeps:.2f}), {med:.3f} s "
                  f"({1e3 * med / st.sweeps:.2f} ms / sweep; {med / seq:.2f} of the sequential run's {seq:.3f} s), "
                  f"rel L2 vs sequential {entry[name]['rel_l2_vs_sequential']:.2e}", flush=True)
        res["utterances"][str(B)] = entry
        os.makedirs(os.path.dirname(out), exist_ok=True)
        with open(out, "w") as f:      # (after every shape: a run cut short keeps what it measured)
            json.dump(res, f, indent=1)
    print("wrote", out)


if __name__ == "__main__":
    main()
