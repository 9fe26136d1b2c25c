"""Developer tool (GPU box): what tied tokens cost and what long-form synthesis gains, in one process, at the product shape (L = 16,
bench.py's model, seeded inputs and memory lengths), DDPM-1000.

  per iteration   a tied run (cfd_sample_begin_tied, the table of ``longform.window_ties(1, rows)``) against a plain run of the same rows,
                  at 8, 15 and 32 rows.  Per repeat and variant: open a run, WARM iterations, then K iterations timed with the host clock
                  between two waits for the run's stream (as bench.py and tools/edit_time.py).
  end to end      one utterance of 15 half-overlapping windows (a 40-second turn), 1000 iterations, three ways: `rollout` = 15 one-row
                  runs in a row, each in-painting its first 8 tokens from the window before (``sample(preseq=)``: what patch_rollout
                  does today); `tied` = one 15-row tied run (``synthesize_latents``); `groups5` = three runs of 5 (max_rows = 5: tied
                  inside, kept carry between).  Host clock around the whole call, run set-up included, ending in the wait of the last read.

The variants alternate within every repeat; medians of REPS repeats; repeat 0 warms every variant up and is not counted.

Usage:  python tools/longform_time.py [REPS] [OUT.json]      (default 5, profiles/r11_longform_time.json)
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
from convofusion_amd.distributed import shard_cfg_batch  # noqa: E402
from convofusion_amd.longform import synthesize_latents, window_ties  # noqa: E402
from convofusion_amd.sampler import SamplingRun, sample  # noqa: E402

L, N, WARM, K = 16, 1000, 5, 200
PRODUCT_S = (24, 161, 24, 8, 1)     # the memory lengths of bench.py's product-shape entries (one 128-frame window of audio and text)
ROWS = (8, 15, 32)
WINDOWS = 15


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 5
    out = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "r11_longform_time.json")
    dev = torch.device("cuda", 0)
    bench.S = PRODUCT_S                 # (bench.make_inputs reads the module's lengths, as bench.py's own product-shape entries set them)
    model = bench.make_model(dev)
    sch = scheduler.DDPMScheduler(num_train_timesteps=1000, beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear",
                                  variance_type="fixed_small", clip_sample=True)
    res = {"reps": reps, "warm_iterations": WARM, "iterations": N, "L": L, "device": torch.cuda.get_device_name(dev), "scheduler": "DDPM",
           "memories": list(bench.S), "timer": "host clock between two waits for the run's stream (as bench.py); variants alternate within "
           "each repeat; end to end: around the whole call, run set-up included", "per_iteration": {}, "end_to_end": {}}
    for rows in ROWS:
        mems, masks = bench.make_inputs(rows, dev, seed=1234)
        variants = [("plain", {}), ("tied", dict(tie=window_ties(1, rows, L).to(dev)))]
        times = {name: [] for name, _ in variants}
        for rep in range(reps + 1):
            for name, kw in variants:
                with SamplingRun(model, sch, mems, masks, rows, L, N, guidance_scale=7.5, seed=0, **kw) as run:
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
                print(f"{rows} rows repeat {rep}: " + ", ".join(f"{n} {times[n][-1]:.4f}" for n in times) + " ms / iteration", flush=True)
        base = statistics.median(times["plain"])
        res["per_iteration"][str(rows)] = {"rows": rows, "timed_iterations": K}
        for name, _ in variants:
            med = statistics.median(times[name])
            res["per_iteration"][str(rows)][name] = dict(ms_per_iteration=med, ms_per_iteration_all=times[name], vs_plain=med / base,
                                                         spread=(max(times[name]) - min(times[name])) / med)
            print(f"{rows} rows {name}: {med:.4f} ms / iteration ({med / base:.4f} of plain)")

    W = WINDOWS
    mems, masks = bench.make_inputs(W, dev, seed=1234)
    kw = dict(L=L, num_inference_steps=N, guidance_scale=7.5, seed=0, skip_zero_weight_chunks=True)

    def rollout():
        prev, wins = None, []
        for w in range(W):
            enc = [shard_cfg_batch(m, w, w + 1, W) for m in mems]
            mk = {k: shard_cfg_batch(v, w, w + 1, W) for k, v in masks.items()}
            wins.append(sample(model, sch, enc, mk, B=1, first_utterance=w, preseq=prev, **kw))
            prev = wins[-1][:, L // 2:].contiguous()
        return torch.cat(wins)

    def tied(max_rows=None):
        return synthesize_latents(model, sch, mems, masks, n_utterances=1, n_windows=W, max_rows=max_rows, **kw)[0][0]

    ways = [("rollout", rollout), ("tied", tied), ("groups5", lambda: tied(5))]
    secs = {name: [] for name, _ in ways}
    for rep in range(reps + 1):
        for name, fn in ways:
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            lat = fn()
            torch.cuda.synchronize(dev)
            dt = time.perf_counter() - t0
            assert tuple(lat.shape) == (W, L, 128) and torch.isfinite(lat).all(), name
            if rep > 0:
                secs[name].append(dt)
        if rep > 0:
            print(f"{W} windows repeat {rep}: " + ", ".join(f"{n} {secs[n][-1]:.3f}" for n in secs) + " s", flush=True)
    base = statistics.median(secs["rollout"])
    res["end_to_end"] = {"windows": W, "frames": (W + 1) * 64}
    for name, _ in ways:
        med = statistics.median(secs[name])
        res["end_to_end"][name] = dict(seconds=med, seconds_all=secs[name], speedup_vs_rollout=base / med)
        print(f"{W} windows {name}: {med:.3f} s ({base / med:.2f}x the rollout's speed)")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", out)


if __name__ == "__main__":
    main()
