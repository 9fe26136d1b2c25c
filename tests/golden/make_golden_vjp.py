#!/usr/bin/env python
"""Generate tests/golden/vjp.npz from the REFERENCE itself (build container only; /root/reference is imported, never copied): torch
autograd through the reference ``Denoiser`` from a seeded cotangent at its output back to its sample,
``torch.autograd.grad(out, sample, d_out)`` -- what a latent-space guidance loss of the reference's loop differentiates through.
The weights and inputs of the WEG cases (make_golden_weg.CASES: plain, sharp and heavy weight sets) are regenerated from their seeds
by the tests, the cotangent by ``tests.vjp_ref.golden_cotangent``; only ``out`` and ``grad`` are stored.

Usage:  python tests/golden/make_golden_vjp.py
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, "/root/reference")
sys.path.insert(0, HERE)

from make_golden import build_reference, rel  # noqa: E402
from make_golden_weg import case_inputs  # noqa: E402
from tests import vjp_ref  # noqa: E402


def main():
    out = {}
    for name in vjp_ref.GOLDEN_CASES:
        sd, inp, t, _, _ = case_inputs(name)
        m = build_reference(sd)
        lat = torch.from_numpy(inp["sample"]).clone().requires_grad_(True)
        masks = {k: (torch.from_numpy(v) if v is not None else None) for k, v in inp["masks"].items()}
        c = vjp_ref.golden_cotangent(name, inp["sample"].shape)
        with torch.enable_grad():
            o, _ = m(sample=lat, timestep=torch.tensor(t), encoder_hidden_states=[torch.from_numpy(x) for x in inp["memories"]],
                     mem_mask_dict=masks)
            grad = torch.autograd.grad(o, [lat], grad_outputs=[torch.from_numpy(c)])[0]
        out[name + ".out"] = o.detach().numpy()
        out[name + ".grad"] = grad.numpy()
        # the float64 restatement against the reference
        o64, g64, _ = vjp_ref.out_and_vjp(sd, inp["sample"], t, inp["memories"], inp["masks"], c)
        print(f"{name}: out rel {rel(o64.astype(np.float32), out[name + '.out']):.2e}  grad rel {rel(g64.astype(np.float32), grad.numpy()):.2e}  "
              f"|grad| {np.abs(grad.numpy()).max():.3e}")
    np.savez_compressed(os.path.join(HERE, "vjp.npz"), **out)
    print("done")


if __name__ == "__main__":
    main()
