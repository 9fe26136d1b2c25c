#!/usr/bin/env python
"""Generate tests/golden/vae_encode.npz from the REFERENCE ``ConvoFusionVae.encode`` (build container only: needs /root/reference on
disk; the class is imported, never copied).

The reference module is built with the configs/modules/motion_vae.yaml values (as make_golden_vae.py), loaded STRICTLY with
oracle.vae_weights' seeded state dict, and ``encode`` is run on seeded features.  Stored per case: mu, logvar and std of the returned
distribution, and the first 3 columns of the returned features (the root-subtracted ones: every other column is the input itself, which
the tests regenerate from the seed).  The case "reseed" runs the "single" features through a second seeded state dict.

Usage:  python tests/golden/make_golden_vae_encode.py
"""
import os
import sys
from types import SimpleNamespace

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, "/root/reference")

from convofusion.models.architectures.vae import ConvoFusionVae  # noqa: E402  (the reference)

from oracle import vae_weights  # noqa: E402
from tests import vae_encode_ref  # noqa: E402
from tests.vae_encode_ref import RESEED, golden_cases as cases  # noqa: E402

torch.set_grad_enabled(False)
def reference(sd_np):
    abl = SimpleNamespace(MLP_DIST=False, PE_TYPE="convofusion")
    m = ConvoFusionVae(ablation=abl, nfeats=189, latent_dim=[1, 128], ff_size=1024, num_layers=5, num_heads=2, dropout=0.1,
                       arch="encoder_decoder", normalize_before=True, activation="gelu", position_embedding="sine").eval()
    m.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in sd_np.items()}, strict=True)
    return m


def main():
    out = {}
    runs = [(name, vae_weights.make_state_dict(), f, lens) for name, (f, lens) in cases().items()]
    runs.append(("reseed", vae_weights.make_state_dict(seed=RESEED), *cases()["single"]))
    for name, sd_np, f, lens in runs:
        m = reference(sd_np)
        latent, dist, feats = m.encode(torch.from_numpy(f), lens)
        mu, std, feats = dist.mean.numpy(), dist.stddev.numpy(), feats.numpy()
        logvar = np.log(std.astype(np.float64) ** 2)
        want_mu, want_lv, want_feats = vae_encode_ref.encode(sd_np, f, lens)
        err = max(float(np.abs(mu - want_mu).max()), float(np.abs(logvar - want_lv).max()))
        print(name, tuple(latent.shape), tuple(mu.shape), tuple(feats.shape), "ref vs float64 restatement max abs", err,
              "std range", float(std.min()), float(std.max()))
        assert np.array_equal(feats, want_feats) and np.array_equal(feats[..., 3:], f[..., 3:])
        assert err < 1e-5, err
        out[name + "_mu"], out[name + "_logvar"], out[name + "_std"] = mu, dist.scale.log().mul(2).numpy(), std
        out[name + "_root"] = feats[..., :3]
    np.savez_compressed(os.path.join(HERE, "vae_encode.npz"), **out)
    print("wrote vae_encode.npz", os.path.getsize(os.path.join(HERE, "vae_encode.npz")), "bytes")


if __name__ == "__main__":
    main()
