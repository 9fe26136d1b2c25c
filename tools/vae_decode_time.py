"""Developer tool (GPU box): what the fused VAE decode costs next to the launch sequence it replaces.

1. At 128 frames / 8 chunks for bs 1, 6, 32 and 120 (a long-form call's worth of windows), milliseconds per call of
     ``decode``                ``ConvoFusionVae.decode(z, lengths)``: the ~190-launch float32 forward (the default; its code and kernels are the
                               parent commit's, so this is also the parent's figure, measured in the same session)
     ``decode_fused``          ``decode(z, lengths, fused=True)`` without grad: one forward-only cfd_vae_decode
     ``decode_vjp``            forward with saves + reverse sweep in one call
     ``fused_round_trip``      ``decode(z.requires_grad_(), lengths, fused=True)`` and ``torch.autograd.grad`` of it: kept forward, then the sweep
   and the workspace bytes of a forward-only call against a saving one (fresh handles).
2. One guided iteration of ``sampler.sample_with_loss_guidance`` (B = 1, L = 16, DDIM, the product-shape memories of the tests) with
   ``edit.pose_keyframe_loss`` fused off (the parent's path) and on, and with ``edit.keyframe_loss`` (denoiser VJP alone).  Per iteration =
   (time of the guided run - time of the same run with no guided iteration) / N.

Every call is a blocking Python call (it waits for the device before its launches and for its stream after them), so a figure is a host
round trip per call, not the cost of an enqueue.  Method as tools/vae_decode_vjp_time.py: seeded weights and inputs; the host clock around
work that ends in a device synchronise; every shape and variant is warmed up first; the variants alternate within each repeat; medians of
REPS repeats, with the spread (min .. max).

Usage:  python tools/vae_decode_time.py [REPS] [OUT.json]      (default 7, profiles/vae_decode_time.json)
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
from convofusion_amd.vae import ConvoFusionVae  # noqa: E402
from oracle import inputs, vae_weights  # noqa: E402
from tests.gpu_helpers import SCHED_KW, hip_denoiser, to_dev  # noqa: E402
from tests.test_oracle_vae import ABL, KW  # noqa: E402

CALLS = {1: 200, 6: 200, 32: 100, 120: 40}     # calls per timed window, by bs (about half a second each)
N_IT = 40                                      # iterations per timed run of part 2


def stats(v):
    return {"median_ms": round(1e3 * statistics.median(v), 4), "min_ms": round(1e3 * min(v), 4), "max_ms": round(1e3 * max(v), 4)}


def timed(fn, calls):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(calls):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / calls


def workspace_bytes(vae, z, lens, keep):
    """The VAE workspace a fresh handle allocates for one cfd_vae_decode of this shape."""
    lib, h = _lib.load(), _lib.create_handle()
    try:
        pack = vae._decoder_pack(z.device)
        lens_d = torch.tensor(lens, dtype=torch.int32, device=z.device)
        feats = torch.empty(z.shape[1], max(lens), 189, device=z.device)
        args = _lib.VaeDecodeArgs(C.c_void_p(pack.data_ptr()), 128, 2, 1024, vae.num_layers, z.shape[1], max(lens), z.shape[2],
                                  C.c_void_p(z.data_ptr()), C.c_void_p(lens_d.data_ptr()))
        t, n = C.c_uint64(0), C.c_longlong(0)
        torch.cuda.synchronize()
        _lib.check(lib.cfd_vae_decode(h, C.byref(args), C.c_void_p(feats.data_ptr()), C.byref(t) if keep else None, None))
        torch.cuda.synchronize()
        _lib.check(lib.cfd_debug_vae_workspace(h, C.byref(n)))
        return n.value
    finally:
        lib.cfd_destroy(h)


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 7
    out = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "vae_decode_time.json")
    dev = torch.device("cuda", 0)
    vae = ConvoFusionVae(ablation=ABL, **KW)
    vae.load_state_dict({k: torch.from_numpy(v) for k, v in vae_weights.make_state_dict().items()}, strict=True)
    vae = vae.to(dev).eval()
    res = {"device": torch.cuda.get_device_name(dev), "reps": reps, "timer": "host clock around CALLS calls (part 1) / one run (part 2) ending in a "
           "device synchronise; variants alternate within each repeat; repeat 0 is warm-up", "decode": {}}
    g = torch.Generator().manual_seed(11)

    def round_trip(z, lens, d):
        zg = z.detach().requires_grad_()
        torch.autograd.grad(vae.decode(zg, lens, fused=True), zg, d)

    for bs, calls in CALLS.items():
        z = torch.randn((2, bs, 8, 128), generator=g).to(dev)
        d = torch.randn((bs, 128, 189), generator=g).to(dev)
        lens = [128] * bs
        fns = {"decode": lambda: vae.decode(z, lens), "decode_fused": lambda: vae.decode(z, lens, fused=True),
               "decode_vjp": lambda: vae.decode_vjp(z, lens, d), "fused_round_trip": lambda: round_trip(z, lens, d)}
        t = {k: [] for k in fns}
        with torch.no_grad():
            diff = float((vae.decode(z, lens, fused=True) - vae.decode(z, lens)).abs().max())
        for rep in range(reps + 1):
            for k, fn in fns.items():
                if k == "fused_round_trip":
                    dt = timed(fn, calls)
                else:
                    with torch.no_grad():
                        dt = timed(fn, calls)
                if rep:
                    t[k].append(dt)
        row = {"nframes": 128, "n_chunks": 8, "calls_per_window": calls, "fused_vs_default_max_abs": diff,
               "workspace_bytes": {"forward_only": workspace_bytes(vae, z, lens, False), "saving": workspace_bytes(vae, z, lens, True)},
               **{k: stats(v) for k, v in t.items()}}
        res["decode"][f"bs{bs}"] = row
        print(f"bs {bs}: " + ", ".join(f"{k} {row[k]['median_ms']} ms" for k in t), row["workspace_bytes"], flush=True)

    # ---- one guided iteration
    m = hip_denoiser(1234, 1.0)
    cb = inputs.make_cfg_batch(seed=43, B=1, L=16, S=(24, 161, 24, 8, 1), pad_tail=(5, 0, 7, 0, 0))
    mems = [to_dev(v) for v in cb["memories"]]
    masks = {k: to_dev(v) for k, v in cb["masks"].items()}
    sch = scheduler.DDIMScheduler(**SCHED_KW)
    rng = np.random.Generator(np.random.PCG64(4343))
    fmask = np.zeros((1, 128), dtype=bool)
    fmask[0, [5, 73, 127]] = True
    target = to_dev(rng.standard_normal((1, 128, 189), dtype=np.float32))
    pose = edit.pose_keyframe_loss(vae, target, to_dev(fmask))
    pose_fused = edit.pose_keyframe_loss(vae, target, to_dev(fmask), fused=True)
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

    variants = [("pose_keyframe_loss", pose, 1.0, {}), ("pose_keyframe_loss_fused", pose_fused, 1.0, {}), ("keyframe_loss", token, 0.05, {}),
                ("unguided", token, 0.05, dict(guided_iterations=()))]
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
                                                                  for k in t if k != "unguided"},
                               "per_iteration_spread_ms": {k: [round(1e3 * (min(t[k]) - base) / N_IT, 4), round(1e3 * (max(t[k]) - base) / N_IT, 4)]
                                                           for k in t if k != "unguided"}}
    print(json.dumps(res["guided_iteration"]), flush=True)
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("wrote", out)


if __name__ == "__main__":
    main()
