"""float64 torch restatement of ``ConvoFusionVae.encode`` from a state dict -- TEST INFRASTRUCTURE (CPU only).

Reference: convofusion/models/architectures/vae.py:162-266 (arch 'encoder_decoder', PE_TYPE 'convofusion', MLP_DIST False),
SkipTransformerEncoder cross_attention.py:18-64, TransformerEncoderLayer.forward_pre :288-300, nn.MultiheadAttention with a key-padding
mask, PositionEmbeddingSine1D position_encoding.py:113-136.  The root subtraction is done in float32 exactly as the reference does it (its
result is compared bit for bit); everything after it runs in float64.  Pinned against the imported reference class by
tests/golden/vae_encode.npz (tests/golden/make_golden_vae_encode.py); used by the GPU tests for shapes too large for a fixture.
"""
import math

import numpy as np
import torch

BODY, HANDS, D = 23 * 3, 40 * 3, 128
RESEED = 99   # the second state dict of the golden case "reseed" (vae_weights.make_state_dict(seed=RESEED))


def golden_cases():
    """name -> (features [bs, nframes, 189] float32, lengths) of tests/golden/vae_encode.npz; "reseed" reuses "single"'s features"""
    rng = np.random.Generator(np.random.PCG64(2024))
    off = rng.standard_normal((2, 64, 189), dtype=np.float32)
    off[0, :, 0] += 50.0
    off[0, :, 2] -= 50.0
    off[1, :, 0] -= 50.0
    off[1, :, 2] += 50.0
    off[:, :, 1] += 1.0
    return {
        "ragged": (rng.standard_normal((3, 128, 189), dtype=np.float32), [128, 100, 37]),
        "single": (rng.standard_normal((1, 32, 189), dtype=np.float32), [32]),
        "long": (rng.standard_normal((2, 256, 189), dtype=np.float32), [200, 256]),
        "offset": (off, [64, 49]),
    }


def root_subtract(features):
    """features [bs, nframes, 189] float32 -> the same with frame 0's root x / z of every 16-frame chunk subtracted (vae.py:176-187)."""
    f = torch.as_tensor(np.asarray(features, np.float32)).clone()
    bs, nframes, nf = f.shape
    m = f.reshape(bs * (nframes // 16), 16, nf)
    root_xz = m[:, :1, :3] * torch.tensor([1, 0, 1])
    m[:, :, :3] = m[:, :, :3] - root_xz
    return m.reshape(bs, nframes, nf)


def _t(sd, k):
    return torch.as_tensor(np.asarray(sd[k])).to(torch.float64)


def _ln(x, sd, pre):
    return torch.nn.functional.layer_norm(x, (x.shape[-1],), _t(sd, pre + ".weight"), _t(sd, pre + ".bias"), 1e-5)


def _lin(x, sd, pre):
    return x @ _t(sd, pre + ".weight").T + _t(sd, pre + ".bias")


def _mha(x, sd, pre, nhead, kpm):
    """self-attention of x [L, N, E] with key_padding_mask kpm [N, L] (True = ignore)."""
    L, N, E = x.shape
    W, B = _t(sd, pre + "in_proj_weight"), _t(sd, pre + "in_proj_bias")
    q, k, v = (x @ W[i * E:(i + 1) * E].T + B[i * E:(i + 1) * E] for i in range(3))
    hd = E // nhead
    sh = lambda t: t.reshape(L, N, nhead, hd).permute(1, 2, 0, 3)         # [N, H, L, hd]
    s = sh(q) @ sh(k).transpose(-1, -2) / math.sqrt(hd)
    s = s.masked_fill(kpm[:, None, None, :], -math.inf)
    o = (torch.softmax(s, -1) @ sh(v)).permute(2, 0, 1, 3).reshape(L, N, E)
    return o @ _t(sd, pre + "out_proj.weight").T + _t(sd, pre + "out_proj.bias")


def _layer(x, sd, pre, nhead, kpm):
    x = x + _mha(_ln(x, sd, pre + "norm1"), sd, pre + "self_attn.", nhead, kpm)
    h = _lin(_ln(x, sd, pre + "norm2"), sd, pre + "linear1")
    return x + _lin(0.5 * h * (1.0 + torch.erf(h / math.sqrt(2.0))), sd, pre + "linear2")


def _skip_encoder(x, sd, pre, num_layers, nhead, kpm):
    nb = (num_layers - 1) // 2
    xs = []
    for i in range(nb):
        x = _layer(x, sd, f"{pre}input_blocks.{i}.", nhead, kpm)
        xs.append(x)
    x = _layer(x, sd, pre + "middle_block.", nhead, kpm)
    for i in range(nb):
        x = _lin(torch.cat([x, xs.pop()], -1), sd, f"{pre}linear_blocks.{i}")
        x = _layer(x, sd, f"{pre}output_blocks.{i}.", nhead, kpm)
    return _ln(x, sd, pre + "norm")


def encode(sd, features, lengths, num_layers=5, nhead=2):
    """-> mu, logvar (float64 numpy [2, bs * nframes / 16, 128], body then hands), root-subtracted features (float32 numpy)."""
    feats = root_subtract(features)
    bs, nframes, _ = feats.shape
    n_chunks = nframes // 16
    n = bs * n_chunks
    x = feats.reshape(n, 16, -1).to(torch.float64)
    valid = (torch.arange(nframes)[None, :] < torch.as_tensor(list(lengths))[:, None]).reshape(n, 16)
    kpm = ~torch.cat([torch.ones(n, 2, dtype=torch.bool), valid], 1)
    pe = _t(sd, "query_pos_encoder.pe")[:18]                                 # [18, 1, D]
    mus, lvs = [], []
    for name, cols in (("body", slice(0, BODY)), ("hands", slice(BODY, BODY + HANDS))):
        emb = _lin(x[:, :, cols], sd, f"{name}_skel_embedding").permute(1, 0, 2)               # [16, n, D]
        tok = _t(sd, f"{name}_global_motion_token")[:, None, :].expand(2, n, D)
        seq = torch.cat([tok, emb], 0) + pe
        out = _skip_encoder(seq, sd, f"{name}_encoder.", num_layers, nhead, kpm)
        mus.append(out[0])
        lvs.append(out[1])
    return torch.stack(mus).numpy(), torch.stack(lvs).numpy(), feats.numpy()
