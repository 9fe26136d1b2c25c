"""Developer tool (GPU box): what the speed-for-accuracy switches cost in the paper's own units.  ``sample()`` + ``vae.decode`` twice per
row of the table, on bench.py's model with its seeded weights at the product shape (L = 16: 128 frames), the seeded VAE of the tests and a
SEEDED FGD net, scored by ``convofusion_amd.metrics.MotionEvaluator`` on the device:

  operands 15      the DDPM default operand policy against policy 0 (fp16 split pairs everywhere)
  parallel tau     ``sample_parallel`` at tolerance 0.05, 0.2 and 0.5 against tolerance 0

The first of each pair is the "target" set, the second the "pred" set: FGD between the two sets, SRGR (semantic weight 0.165 on every
frame, so the rate is the plain success rate) and jitter against the paired motion, diversity and L1div of each set.  No trained
checkpoint is involved: with a seeded FGD net the FGD is a random-feature Frechet distance -- it orders the switches by how far they move
the motions, and says nothing about perceptual quality.  No audio: the alignment is not in the table.

Usage:  python tools/metrics_table.py [UTTERANCES] [STEPS] [FEATURE_LENGTH] [OUT.json]     (default 64, 1000, 32, profiles/metrics_table.json)
"""
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from convofusion_amd import scheduler  # noqa: E402
from convofusion_amd.edit import loop_to_vae  # noqa: E402
from convofusion_amd.metrics import FGDNet, MotionEvaluator  # noqa: E402
from convofusion_amd.sampler import sample, sample_parallel  # noqa: E402
from convofusion_amd.vae import ConvoFusionVae  # noqa: E402
from oracle import vae_weights  # noqa: E402
from tests.test_oracle_vae import ABL, KW  # noqa: E402

L = 16
PRODUCT_S = (24, 161, 24, 8, 1)
CHUNK = 16          # utterances per sampling run


def main():
    B = int(sys.argv[1]) if len(sys.argv) > 1 else 64
    N = int(sys.argv[2]) if len(sys.argv) > 2 else 1000
    F = int(sys.argv[3]) if len(sys.argv) > 3 else 32
    out = sys.argv[4] if len(sys.argv) > 4 else os.path.join(ROOT, "profiles", "metrics_table.json")
    dev = torch.device("cuda", 0)
    bench.S = PRODUCT_S
    model = bench.make_model(dev)
    vae = ConvoFusionVae(ablation=ABL, **KW)
    vae.load_state_dict({k: torch.from_numpy(v) for k, v in vae_weights.make_state_dict().items()}, strict=True)
    vae = vae.to(dev).eval()
    torch.manual_seed(11)
    fgd = FGDNet(128, 189, F)
    for m in fgd.modules():
        if isinstance(m, torch.nn.BatchNorm1d):
            m.running_var.uniform_(0.5, 1.5)
            m.running_mean.normal_(0, 0.1)
    fgd.eval()
    sch = scheduler.DDPMScheduler(num_train_timesteps=1000, beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear",
                                  variance_type="fixed_small", clip_sample=True)

    def motions(run):
        parts = []
        for c0 in range(0, B, CHUNK):
            n = min(CHUNK, B - c0)
            mems, masks = bench.make_inputs(n, dev, seed=1234 + c0)
            gen = torch.Generator(dev).manual_seed(1 + c0)
            init = torch.randn((n, L, 128), device=dev, generator=gen)
            noise = torch.randn((N, n, L, 128), device=dev, generator=gen)
            lat = run(mems, masks, dict(B=n, L=L, num_inference_steps=N, guidance_scale=7.5, init_latents=init, step_noise=noise))
            parts.append(vae.decode(loop_to_vae(lat), [128] * n))
        return torch.cat(parts)

    def seq(policy):
        return lambda mems, masks, kw: sample(model, sch, mems, masks, operands=policy, skip_zero_weight_chunks=True, **kw)

    def par(tau):
        return lambda mems, masks, kw: sample_parallel(model, sch, mems, masks, tolerance=tau, **kw)[0]

    rows = [("operands 15 against 0", seq(0), seq(15))] + [(f"parallel tolerance {tau:g} against 0", par(0.0), par(tau)) for tau in (0.05, 0.2, 0.5)]
    sem = torch.full((B, 128), 0.165, device=dev)
    cache, table = {}, {}
    for name, base, variant in rows:
        key = "par0" if name.startswith("parallel") else "seq0"
        if key not in cache:
            cache[key] = motions(base)
        target, t0 = cache[key], time.perf_counter()
        pred = motions(variant)
        torch.cuda.synchronize(dev)
        t1 = time.perf_counter()
        ev = MotionEvaluator(fgd)
        ev.update(pred, target, sem)
        r = ev.compute()
        torch.cuda.synchronize(dev)
        r["rel_l2_motion"] = float((pred.double() - target.double()).norm() / target.double().norm())
        r["seconds_sampling"], r["seconds_metrics"] = t1 - t0, time.perf_counter() - t1
        table[name] = r
        print(f"{name}: " + ", ".join(f"{k} {v:.6g}" for k, v in r.items() if v is not None), flush=True)
    res = {"utterances": B, "iterations": N, "feature_length": F, "device": torch.cuda.get_device_name(dev),
           "weights": "seeded (bench.py denoiser, the tests' VAE, a seeded FGD net): a random-feature Frechet distance, no trained checkpoint",
           "table": table}
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", out)


if __name__ == "__main__":
    main()
