#!/usr/bin/env python
"""Generate tests/golden/vae_depths.npz from the REFERENCE ``ConvoFusionVae`` at num_layers 1 and 9 (build container only: needs
/root/reference on disk; the class is imported, never copied).

The reference module is built as in make_golden_vae.py (configs/modules/motion_vae.yaml values, 2 heads) but with ``num_layers`` 1 and 9
-- no input / output blocks at all, and four of each -- and loaded STRICTLY with ``oracle.vae_weights.make_state_dict(num_layers=...)``.
Every input is regenerated from a seed by the tests (tests/vae_encode_ref.shape_cases, tests/vae_vjp_ref.depth_case_inputs); per depth
<nl> the file stores numbers only:
  enc<nl>.mu, enc<nl>.logvar  float32 [2, 9, 128]: ``encode`` of the shape case "mix" (mean and 2 log(std) of the returned distribution)
  enc<nl>.root                float32 [3, 48, 3]: the first 3 columns of the returned, root-subtracted features
  dec<nl>.feats               float32 [2, 40, 189]: ``decode`` of the depth case
  dec<nl>.grad                float64 [2, 2, 3, 128]: torch.autograd.grad(decode(z, lengths), z, d_feats) of ``module.double()``

Usage:  python tests/golden/make_golden_vae_depths.py
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
from tests import vae_encode_ref, vae_vjp_ref  # noqa: E402

DEPTHS = (1, 9)


def module(sd_np, num_layers, dtype=torch.float32):
    abl = SimpleNamespace(MLP_DIST=False, PE_TYPE="convofusion")
    m = ConvoFusionVae(ablation=abl, nfeats=189, latent_dim=[1, 128], ff_size=1024, num_layers=num_layers, num_heads=2, dropout=0.1,
                       arch="encoder_decoder", normalize_before=True, activation="gelu", position_embedding="sine").eval()
    m.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in sd_np.items()}, strict=True)
    return m.to(dtype)


def main():
    out = {}
    f, lens = vae_encode_ref.shape_cases()[vae_encode_ref.DEPTH_CASE]
    z, zlens, d = vae_vjp_ref.depth_case_inputs()
    for nl in DEPTHS:
        sd_np = vae_weights.make_state_dict(num_layers=nl)
        m = module(sd_np, nl)
        with torch.no_grad():
            _, dist, feats = m.encode(torch.from_numpy(f), lens)
            dec = m.decode(torch.from_numpy(z), zlens).numpy()
        mu, logvar, feats = dist.mean.numpy(), dist.scale.log().mul(2).numpy(), feats.numpy()
        want_mu, want_lv, want_feats = vae_encode_ref.encode(sd_np, f, lens, num_layers=nl)
        e_enc = max(float(np.abs(mu - want_mu).max()), float(np.abs(logvar - want_lv).max()))
        assert np.array_equal(feats, want_feats) and np.array_equal(feats[..., 3:], f[..., 3:])
        zt = torch.from_numpy(z).double().requires_grad_(True)
        (g64,) = torch.autograd.grad(module(sd_np, nl, torch.float64).decode(zt, zlens), zt, torch.from_numpy(d).double())
        want_dec, want_g, _ = vae_vjp_ref.decode_vjp(sd_np, z, zlens, d, num_layers=nl)
        e_dec = float(np.abs(dec - want_dec).max())
        print(f"num_layers {nl}: {len(sd_np)} keys; encode ref vs float64 restatement max abs {e_enc:.3e}; decode {e_dec:.3e}; "
              "sweep restatement vs float64 autograd rel L2 %.3e worst row %.3e" % vae_vjp_ref.errors(want_g, g64.numpy()))
        assert e_enc < 1e-5 and e_dec < 1e-5, (e_enc, e_dec)
        out[f"enc{nl}.mu"], out[f"enc{nl}.logvar"], out[f"enc{nl}.root"] = mu, logvar, feats[..., :3]
        out[f"dec{nl}.feats"], out[f"dec{nl}.grad"] = dec, g64.numpy()
    path = os.path.join(HERE, "vae_depths.npz")
    np.savez_compressed(path, **out)
    print("wrote vae_depths.npz", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
