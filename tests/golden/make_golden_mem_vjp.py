#!/usr/bin/env python
"""Generate tests/golden/mem_vjp.npz and tests/golden/mem_vjp_heavy.npz from the REFERENCE itself (build container only; /root/reference is imported, never copied): torch
autograd through the reference ``Denoiser`` from the seeded cotangent of ``tests.vjp_ref.golden_cotangent`` at its output back to its
five MEMORIES, ``torch.autograd.grad(out, encoder_hidden_states, d_out)`` -- what fitting a conditioning tensor differentiates through.
The weights and inputs of the WEG cases (make_golden_weg.CASES: plain, sharp and heavy weight sets) are regenerated from their seeds
by the tests; only the five gradients per case are stored, as float32.  Prints the float64 restatement (tests/mem_vjp_ref.py) against
the reference per memory.

Usage:  python tests/golden/make_golden_mem_vjp.py
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
from oracle.denoiser_ref import MEM_NAMES  # noqa: E402
from tests import mem_vjp_ref, vjp_ref  # noqa: E402


def main():
    out = {}
    for name in vjp_ref.GOLDEN_CASES:
        sd, inp, t, _, _ = case_inputs(name)
        m = build_reference(sd)
        mems = [torch.from_numpy(x).clone().requires_grad_(True) for x in inp["memories"]]
        masks = {k: (torch.from_numpy(v) if v is not None else None) for k, v in inp["masks"].items()}
        c = vjp_ref.golden_cotangent(name, inp["sample"].shape)
        with torch.enable_grad():
            o, _ = m(sample=torch.from_numpy(inp["sample"]), timestep=torch.tensor(t), encoder_hidden_states=mems, mem_mask_dict=masks)
            grads = torch.autograd.grad(o, mems, grad_outputs=[torch.from_numpy(c)])
        d64 = mem_vjp_ref.out_and_vjp_mem(sd, inp["sample"], t, inp["memories"], inp["masks"], c)[2]
        for k, g, g64 in zip(MEM_NAMES, grads, d64):
            out[f"{name}.{k}"] = g.numpy().astype(np.float32)
            print(f"{name}.{k}: restatement vs reference rel {rel(g64.astype(np.float32), g.numpy()):.2e}  |grad| {np.abs(g.numpy()).max():.3e}")
    # two files, each below the size limit of a committed file: the heavy-tailed case on its own
    for fname, keep in (("mem_vjp.npz", lambda k: not k.startswith("b1_heavy.")), ("mem_vjp_heavy.npz", lambda k: k.startswith("b1_heavy."))):
        np.savez_compressed(os.path.join(HERE, fname), **{k: v for k, v in out.items() if keep(k)})
    print("done:", sum(v.nbytes for v in out.values()), "bytes uncompressed")


if __name__ == "__main__":
    main()
