#!/usr/bin/env python
"""Generate tests/golden/audio_enc_vjp.npz from the REFERENCE class (build container only: needs /root/reference on disk; the reference
is imported, never copied).

``convofusion.models.architectures.audioenc.AudioConvEncoder`` in eval mode (its two Dropout(0.1) are the identity), cast to float64,
at 2 x 5 Mel rows: torch autograd gives the gradients of its six parameters and of its input for a seeded cotangent.  Widths
80 / 48 / 40, not the shipped 80 / 256 / 512, so that weights and float64 gradients stay far below the size limit of a committed file;
the shipped widths are covered by the numpy restatement (tests/audio_enc_vjp_ref.py).  As in make_golden_conditioning.py, an empty
placeholder stands in for ``convofusion.config`` (omegaconf is not installed here), which the class does not use.

The file holds numbers only: the float32 parameters (torch's default init under a fixed seed), the float32 input and cotangent, the
float64 output and gradients.

Usage:  python tests/golden/make_golden_audio_enc_vjp.py
"""
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, "/root/reference")
if "convofusion.config" not in sys.modules:
    try:
        import convofusion.config  # noqa: F401
    except Exception:
        ph = types.ModuleType("convofusion.config")
        ph.instantiate_from_config = lambda *a, **k: (_ for _ in ()).throw(RuntimeError("placeholder"))
        sys.modules["convofusion.config"] = ph

from convofusion.models.architectures.audioenc import AudioConvEncoder  # noqa: E402  (the reference)

IN_DIM, HIDDEN, LATENT = 80, 48, 40
torch.manual_seed(4321)
g = torch.Generator().manual_seed(77)
enc = AudioConvEncoder(input_size=IN_DIM, hidden_size=HIDDEN, latent_dim=LATENT, max_seq_len=128, fps=25, sample_rate=16000, hop_length=160).eval()
params32 = {k: v.detach().clone().numpy() for k, v in enc.state_dict().items()}
enc = enc.double()
mel = (-40.0 + 25.0 * torch.randn((2, 5, IN_DIM), generator=g)).float()
d_out = (torch.randn((2, 5, LATENT), generator=g) / (10 * LATENT)).float()

x = mel.double().requires_grad_(True)
y = enc(x)
names = [k for k, _ in enc.named_parameters()]
grads = torch.autograd.grad(y, [x] + [p for _, p in enc.named_parameters()], d_out.double())

out = {"mel": mel.numpy(), "d_out": d_out.numpy(), "out": y.detach().numpy(), "grad.d_x": grads[0].numpy()}
for k, v in params32.items():
    out["param." + k] = v
for k, gk in zip(names, grads[1:]):
    out["grad." + k] = gk.numpy()
np.savez_compressed(os.path.join(HERE, "audio_enc_vjp.npz"), **out)
print("wrote audio_enc_vjp.npz:", {k: (v.shape, str(v.dtype)) for k, v in out.items()})
