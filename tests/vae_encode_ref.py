"""float64 torch restatement of ``ConvoFusionVae.encode`` from a state dict -- TEST INFRASTRUCTURE (CPU only).

Reference: convofusion/models/architectures/vae.py:162-266 (arch 'encoder_decoder', PE_TYPE 'convofusion', MLP_DIST False),
SkipTransformerEncoder cross_attention.py:18-64, TransformerEncoderLayer.forward_pre :288-300, nn.MultiheadAttention with a key-padding
mask, PositionEmbeddingSine1D position_encoding.py:113-136.  The root subtraction is done in float32 exactly as the reference does it (its
result is compared bit for bit); everything after it runs in float64 (or in the ``dtype`` the caller names).  Pinned against the imported reference class by
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


DEPTH_CASE = "mix"   # the shape case tests/golden/vae_depths.npz holds at num_layers 1 and 9


def shape_cases():
    """name -> (features [bs, nframes, 189] float32, lengths): the small cases of tests/test_gpu_vae_encode_shapes.py, chosen by how their
    bs * nframes / 16 sequences fall into workgroups of 1, 2 or 3 sequences (csrc/vae_enc.hpp):
      one    1 sequence: a partial group at 2 and at 3 per group
      span   4 sequences, valid frames 16, 16, 5, 0: at 3 per group the first group spans both batch items
      mix    9 sequences, valid frames 16, 16, 16 | 16, 1, 0 | 0, 0, 0 (one batch item is empty); root x / z offset by +-50
      seven  7 sequences of one chunk: the last group holds one sequence at 2 and at 3 per group"""
    rng = np.random.Generator(np.random.PCG64(2025))
    one = rng.standard_normal((1, 16, 189), dtype=np.float32)
    span = rng.standard_normal((2, 32, 189), dtype=np.float32)
    mix = rng.standard_normal((3, 48, 189), dtype=np.float32)
    mix[0, :, 0] += 50.0
    mix[0, :, 2] -= 50.0
    mix[1, :, 0] -= 50.0
    mix[1, :, 2] += 50.0
    seven = rng.standard_normal((7, 16, 189), dtype=np.float32)
    return {"one": (one, [16]), "span": (span, [32, 5]), "mix": (mix, [48, 17, 0]), "seven": (seven, [16, 15, 1, 16, 8, 16, 2])}


def root_subtract(features):
    """features [bs, nframes, 189] float32 -> the same with frame 0's root x / z of every 16-frame chunk subtracted (vae.py:176-187)."""
    f = torch.as_tensor(np.asarray(features, np.float32)).clone()
    bs, nframes, nf = f.shape
    m = f.reshape(bs * (nframes // 16), 16, nf)
    root_xz = m[:, :1, :3] * torch.tensor([1, 0, 1])
    m[:, :, :3] = m[:, :, :3] - root_xz
    return m.reshape(bs, nframes, nf)


def _cast(sd, dtype):
    """the encoder's entries of a float32 numpy state dict as tensors of ``dtype`` (what ``_t`` reads)"""
    return {k: torch.as_tensor(np.asarray(v)).to(dtype) for k, v in sd.items() if "decoder" not in k and "final_layer" not in k}


def _t(sd, k):
    return sd[k]


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


def encode(sd, features, lengths, num_layers=5, nhead=2, dtype=torch.float64):
    """-> mu, logvar (numpy of ``dtype`` [2, bs * nframes / 16, 128], body then hands), root-subtracted features (float32 numpy).
    dtype=torch.float32: everything behind the root subtraction in float32 (the yardstick of a float32 kernel's distance from float64)."""
    sd = _cast(sd, dtype)
    feats = root_subtract(features)
    bs, nframes, _ = feats.shape
    n_chunks = nframes // 16
    n = bs * n_chunks
    x = feats.reshape(n, 16, -1).to(dtype)
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
