"""Developer tool (GPU box): what the audio encoder's backward pass costs, next to the memory gradient it follows.

At B = 1, 8 and 43 examples of 161 Mel frames (161, 1 288 and 6 923 rows; encoder 80 / 256 / 512, seeded weights):
  enc_vjp_all         one ``cfd_audio_encoder_vjp`` with all six parameter gradients (``conditioning.audio_encoder_vjp``)
  enc_vjp_all_dx      the same with ``d_x`` and ``out`` too: every launch the call has
  enc_forward         the plain three-launch forward, for scale
  vjp_mem_alsn        the ``cfd_denoise_vjp_mem`` call in front of it: B rows of L = 16, every example's own memories,
                      S = (24, 161, 24, 8, 1), ``wrt=("alsn",)``, no sample gradient
and at B = 8, L = 16:
  fit_audio_encoder_step   one step of ``fit.fit_audio_encoder`` (encoder forward + denoiser forward + memory gradient + encoder
                           backward + Adam), whole call of STEPS steps / STEPS
  fit_identity_step        one step of ``fit.fit_identity`` on the same examples, same session
with the launches of each encoder call ("audio_enc_vjp.info").

Timer: hipEvents (torch.cuda.Event) around one call, medians of 30 with the spread; every variant is warmed up first.  The encoder
call only enqueues; the events bracket its launches on the stream.

Usage:  python tools/audio_enc_vjp_time.py [--out OUT.json]      (default profiles/audio_enc_vjp_time.json)
"""
import argparse
import json
import os
import statistics
import sys

N = 30
S_PRODUCT = (24, 161, 24, 8, 1)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def stats(v):
    return {"median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v), "n": len(v)}


def timed(torch, fn, n=N, warm=3):
    for _ in range(warm):
        fn()
    out = []
    for _ in range(n):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b))
    return stats(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "audio_enc_vjp_time.json"))
    a = ap.parse_args()
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch
    from convofusion_amd import conditioning, fit, scheduler
    from oracle import inputs
    from tests import audio_enc_vjp_ref as R
    from tests.gpu_helpers import SCHED_KW, hip_denoiser, to_dev
    from tests.test_gpu_audio_enc_vjp import encoder_of

    res = {"what": "hipEvent times on one MI355X, seeded weights; ms, medians of 30.  B examples of 161 Mel frames, encoder 80 / 256 / 512; "
                   "vjp_mem_alsn: cfd_denoise_vjp_mem at B rows of L = 16, S = (24, 161, 24, 8, 1), wrt alsn only; the fit steps at B = 8, "
                   "L = 16, whole call of 10 Adam steps / 10.",
           "device": torch.cuda.get_device_name(0)}
    params = R.seeded_params(80, 256, 512, seed=91)
    enc = encoder_of(params)
    m = hip_denoiser(1234, 1.0)
    for B in (1, 8, 43):
        x, d = R.seeded_inputs(B * 161, 80, 512, seed=100 + B)
        mel, dd = to_dev(x).reshape(B, 161, 80), to_dev(d).reshape(B, 161, 512)
        out = torch.empty_like(dd)
        r = {"rows": B * 161}
        r["enc_vjp_all"] = timed(torch, lambda: conditioning.audio_encoder_vjp(enc, mel, dd))
        r["enc_vjp_all"]["launches"], _, r["segments"], r["workspace_bytes"] = conditioning.audio_enc_vjp_info("cuda")
        r["enc_vjp_all_dx"] = timed(torch, lambda: conditioning.audio_encoder_vjp(enc, mel, dd, want_dx=True, out=out))
        r["enc_vjp_all_dx"]["launches"] = conditioning.audio_enc_vjp_info("cuda")[0]
        r["enc_vjp_dx_only"] = timed(torch, lambda: conditioning.audio_encoder_vjp(enc, mel, dd, want=(), want_dx=True))
        r["enc_vjp_dx_only"]["launches"] = conditioning.audio_enc_vjp_info("cuda")[0]
        with torch.no_grad():
            r["enc_forward"] = timed(torch, lambda: enc(mel))
        inp = inputs.make_plain_batch(seed=45, Be=B, L=16, S=S_PRODUCT, pad_tail=(5, 0, 7, 0, 0))
        lat = to_dev(np.random.Generator(np.random.PCG64(46)).standard_normal((B, 16, 128), dtype=np.float32))
        fm, fk = [to_dev(v) for v in inp["memories"]], {k: to_dev(v) for k, v in inp["masks"].items()}
        c = torch.ones_like(lat)
        r["vjp_mem_alsn"] = timed(torch, lambda: m.vjp_memories(lat, 433, fm, fk, c, wrt=("alsn",), want_out=False, want_grad=False))
        res[f"B{B}"] = r
        if B == 8:
            steps = 10
            sch = scheduler.DDPMScheduler(variance_type="fixed_small", **SCHED_KW)
            one = timed(torch, lambda: fit.fit_identity(m, sch, lat, fm, fk, steps=steps, lr=0.01, seed=1), n=10, warm=1)
            res["fit_identity_step"] = {k: (v / steps if k.endswith("_ms") else v) for k, v in one.items()}
            fenc = encoder_of(params)
            one = timed(torch, lambda: fit.fit_audio_encoder(m, sch, fenc, lat, mel, fm, fk, steps=steps, lr=1e-5, seed=1), n=10, warm=1)
            res["fit_audio_encoder_step"] = {k: (v / steps if k.endswith("_ms") else v) for k, v in one.items()}
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
