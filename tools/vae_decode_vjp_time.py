"""Developer tool (GPU box): what the differentiable VAE decode costs.

1. ``ConvoFusionVae.decode_vjp`` (cfd_vae_decode_vjp: forward with saves + reverse sweep, csrc/vae_dec.hpp) at 128 frames / 8 chunks for
   bs 1, 6 and 32, next to today's ``decode`` (the ~190-launch float32 forward) at the same shapes: milliseconds per call and the launches
   of one decode_vjp call ("vae.info").
2. One guided iteration of ``sampler.sample_with_loss_guidance`` (B = 1, L = 16, DDIM, the product-shape memories of the tests) with
   ``edit.pose_keyframe_loss`` -- denoiser VJP + decode + decode_vjp -- against one with ``edit.keyframe_loss`` -- denoiser VJP alone; the
   latter runs unchanged on the parent commit.  Per iteration = (time of the guided run - time of the same run with no guided iteration) / N.

``decode_vjp`` is a blocking Python call (it waits for the device before its launches and for its stream after them), so its figure is a
host round trip per call, not the cost of an enqueue.  The kernels' own times: tools/vae_decode_vjp_prof.py.

Seeded weights (oracle.vae_weights, tests.gpu_helpers.hip_denoiser) and inputs.  Timer: the host clock around work that ends in a device
synchronise; every shape and variant is warmed up first; the variants alternate within each repeat; medians of REPS repeats, with the
spread (min .. max).

Usage:  python tools/vae_decode_vjp_time.py [REPS] [OUT.json]      (default 7, profiles/vae_decode_vjp_time.json)
"""
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from convofusion_amd import _lib, edit, sampler, scheduler  # noqa: E402
from convofusion_amd.conditioning import _engine_handle  # noqa: E402
from convofusion_amd.vae import ConvoFusionVae  # noqa: E402
from oracle import inputs, vae_weights  # noqa: E402
from tests.gpu_helpers import SCHED_KW, hip_denoiser, to_dev  # noqa: E402
from tests.test_oracle_vae import ABL, KW  # noqa: E402

CALLS = 200         # calls per timed window of part 1 (about half a second)
N_IT = 40           # iterations per timed run of part 2


def stats(v):
    return {"median_ms": round(1e3 * statistics.median(v), 4), "min_ms": round(1e3 * min(v), 4), "max_ms": round(1e3 * max(v), 4)}


def timed(fn, calls):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(calls):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / calls


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 7
    out = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "vae_decode_vjp_time.json")
    dev = torch.device("cuda", 0)
    vae = ConvoFusionVae(ablation=ABL, **KW)
    vae.load_state_dict({k: torch.from_numpy(v) for k, v in vae_weights.make_state_dict().items()}, strict=True)
    vae = vae.to(dev).eval()
    res = {"device": torch.cuda.get_device_name(dev), "reps": reps, "timer": "host clock around CALLS calls (part 1) / one run (part 2) ending in a "
           "device synchronise; variants alternate within each repeat; repeat 0 is warm-up", "calls_per_window": CALLS, "decode": {}}
    g = torch.Generator().manual_seed(11)
    for bs in (1, 6, 32):
        z = torch.randn((2, bs, 8, 128), generator=g).to(dev)
        d = torch.randn((bs, 128, 189), generator=g).to(dev)
        lens = [128] * bs
        t = {"decode_vjp": [], "decode_vjp_no_out": [], "decode": []}
        for rep in range(reps + 1):
            a = timed(lambda: vae.decode_vjp(z, lens, d), CALLS)
            b = timed(lambda: vae.decode_vjp(z, lens, d, want_out=False), CALLS)
            c = timed(lambda: vae.decode(z, lens), CALLS)
            if rep:
                t["decode_vjp"].append(a), t["decode_vjp_no_out"].append(b), t["decode"].append(c)
        info = torch.empty(2, device=dev)
        vae.decode_vjp(z, lens, d)
        _lib.check(_lib.load().cfd_debug_read(_engine_handle(dev), b"vae.info", C.c_void_p(info.data_ptr()), 2))
        res["decode"][f"bs{bs}"] = {"nframes": 128, "n_chunks": 8, "decode_vjp_launches": int(info[0].item()),
                                    **{k: stats(v) for k, v in t.items()}}
        print(f"bs {bs}: " + ", ".join(f"{k} {res['decode'][f'bs{bs}'][k]['median_ms']} ms" for k in t), f"({int(info[0].item())} launches)", flush=True)

    # ---- one guided iteration
    m = hip_denoiser(1234, 1.0)
    cb = inputs.make_cfg_batch(seed=43, B=1, L=16, S=(24, 161, 24, 8, 1), pad_tail=(5, 0, 7, 0, 0))
    mems = [to_dev(v) for v in cb["memories"]]
    masks = {k: to_dev(v) for k, v in cb["masks"].items()}
    sch = scheduler.DDIMScheduler(**SCHED_KW)
    rng = np.random.Generator(np.random.PCG64(4343))
    fmask = np.zeros((1, 128), dtype=bool)
    fmask[0, [5, 73, 127]] = True
    pose = edit.pose_keyframe_loss(vae, to_dev(rng.standard_normal((1, 128, 189), dtype=np.float32)), to_dev(fmask))
    tmask = np.zeros((1, 16), dtype=bool)
    tmask[0, [3, 9]] = True
    token = edit.keyframe_loss(to_dev(rng.standard_normal((1, 16, 128), dtype=np.float32)), to_dev(tmask))
    kw = dict(B=1, L=16, num_inference_steps=N_IT, guidance_scale=7.5, eta=0.0, init_latents=to_dev(cb["init"]))

    def run(loss, step, **more):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        lat = sampler.sample_with_loss_guidance(m, sch, mems, masks, loss, step, **kw, **more)
        torch.cuda.synchronize()
        assert torch.isfinite(lat).all()
        return time.perf_counter() - t0

    variants = [("pose_keyframe_loss", pose, 1.0, {}), ("keyframe_loss", token, 0.05, {}), ("unguided", token, 0.05, dict(guided_iterations=()))]
    t = {name: [] for name, _, _, _ in variants}
    for rep in range(reps + 1):
        for name, loss, step, more in variants:
            dt = run(loss, step, **more)
            if rep:
                t[name].append(dt)
    base = statistics.median(t["unguided"])
    res["guided_iteration"] = {"B": 1, "L": 16, "iterations": N_IT, "scheduler": "DDIM",
                               "run_ms": {k: stats(v) for k, v in t.items()},
                               "per_iteration_over_unguided_ms": {k: round(1e3 * (statistics.median(t[k]) - base) / N_IT, 4)
                                                                  for k in ("pose_keyframe_loss", "keyframe_loss")}}
    print(json.dumps(res["guided_iteration"]), flush=True)
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("wrote", out)


if __name__ == "__main__":
    main()
