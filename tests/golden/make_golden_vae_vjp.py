#!/usr/bin/env python
"""Generate tests/golden/vae_decode_vjp.npz from the REFERENCE ``ConvoFusionVae`` (build container only: needs /root/reference on
disk; the class is imported, never copied).

The reference module is built as in make_golden_vae.py (configs/modules/motion_vae.yaml values, oracle.vae_weights' seeded state dict,
loaded strictly).  Its ``decode`` is an ordinary differentiable module; per case of tests/vae_vjp_ref.CASES (latents and cotangent
regenerated from seeds by the tests) the file stores numbers only:
  <case>.grad      float64 [2, bs, n_chunks, 128]: torch.autograd.grad(decode(z, lengths), z, d_feats) of ``module.double()``
  <case>.yard      float64 [2]: how far the reference's own float32 autograd gradient lies from that one -- relative L2 over the gradient,
                   and the worst 128-wide row (tests/vae_vjp_ref.errors)
  <case>.fwd_diff  float64 [1]: max abs difference of the float32 and float64 forwards

Usage:  python tests/golden/make_golden_vae_vjp.py
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
from tests import vae_vjp_ref  # noqa: E402


def module(sd_np, dtype):
    abl = SimpleNamespace(MLP_DIST=False, PE_TYPE="convofusion")
    m = ConvoFusionVae(ablation=abl, nfeats=189, latent_dim=[1, 128], ff_size=1024, num_layers=5, num_heads=2, dropout=0.1,
                       arch="encoder_decoder", normalize_before=True, activation="gelu", position_embedding="sine").eval()
    m.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in sd_np.items()}, strict=True)
    return m.to(dtype)


def grad(m, z, lengths, d, dtype):
    zt = torch.from_numpy(z).to(dtype).requires_grad_(True)
    feats = m.decode(zt, lengths)
    (g,) = torch.autograd.grad(feats, zt, torch.from_numpy(d).to(dtype))
    return feats.detach().numpy(), g.numpy()


def main():
    sd_np = vae_weights.make_state_dict()
    m64, m32 = module(sd_np, torch.float64), module(sd_np, torch.float32)
    out = {}
    for name in vae_vjp_ref.CASES:
        z, lengths, d = vae_vjp_ref.case_inputs(name)
        f64, g64 = grad(m64, z, lengths, d, torch.float64)
        f32, g32 = grad(m32, z, lengths, d, torch.float32)
        assert np.isfinite(g64).all() and np.isfinite(g32).all()
        yard = vae_vjp_ref.errors(g32, g64)
        mine = vae_vjp_ref.decode_vjp(sd_np, z, lengths, d)[1]
        print(name, g64.shape, "float32 vs float64 autograd: rel L2 %.3e worst row %.3e" % yard, "forward max abs %.3e" % np.abs(f32 - f64).max(),
              "restatement vs float64 autograd: rel L2 %.3e worst row %.3e" % vae_vjp_ref.errors(mine, g64))
        out[name + ".grad"] = g64
        out[name + ".yard"] = np.asarray(yard, np.float64)
        out[name + ".fwd_diff"] = np.asarray([np.abs(f32 - f64).max()], np.float64)
    np.savez_compressed(os.path.join(HERE, "vae_decode_vjp.npz"), **out)
    print("wrote vae_decode_vjp.npz")


if __name__ == "__main__":
    main()
