"""High-precision restatement of ``ConvoFusionVae.decode`` and its reverse sweep with taps -- TEST INFRASTRUCTURE.

The forward of ``oracle/vae_ref.py`` (reference vae.py:268-372, cross_attention.py:66-125,361-382) written again in ONE numpy dtype chosen
by the caller, keeping what a reverse sweep needs, and the sweep from a cotangent at the 189 output features back to the latents, built
from the blocks of ``tests/weg_bwd_ref.py`` (LayerNorm / softmax / GELU backward).  float64 is what the HIP sweep (csrc/vae_dec.hpp) is
measured against stage by stage; nothing here looks at the kernels.  Weights, latents and the cotangent are float32 inputs and are cast.

Layout: activations and gradients are [F, bs, C] (sequence first, as the reference's decoder).

Taps (``s`` = stack 0 body / 1 hands, ``l`` = layer in the order input_blocks, middle_block, output_blocks):
  x.s.l    the forward's stream at layer l's input (behind the skip linear); x.s.(num_layers) the last layer's output
  g.s.l    the running gradient at layer l's output as it enters the layer's backward (the skip tensor's share included)
  dz.s.l   layer l's memory-side contribution to d_z[s], [bs, n_chunks, 128]: dK_l . W_k,l + dV_l . W_v,l
"""
import math

import numpy as np

from tests.weg_bwd_ref import _Net, _gelu, _gelu_grad, _lin, _ln, _ln_bwd, _softmax, _softmax_bwd

D, NHEAD = 128, 2
BODY, HANDS = 69, 120
PARTS = ("body", "hands")


def layer_prefixes(pre, num_layers):
    nb = (num_layers - 1) // 2
    return [f"{pre}input_blocks.{i}." for i in range(nb)] + [pre + "middle_block."] + [f"{pre}output_blocks.{i}." for i in range(nb)]


def _heads(a, bs):
    """[n, bs, D] -> [bs * H, n, hd]"""
    return a.reshape(a.shape[0], bs * NHEAD, D // NHEAD).transpose(1, 0, 2)


def _unheads(a, bs):
    return a.transpose(1, 0, 2).reshape(a.shape[1], bs, D)


def _attn_fwd(P, pre, xq, xkv, bs, key_mask):
    """nn.MultiheadAttention (packed in-projection, q scaled before the product); key_mask bool [bs, Lk] True = masked, or None.
    Returns (output behind out_proj, saved)."""
    W, B = P(pre + "in_proj_weight"), P(pre + "in_proj_bias")
    qs = xq.dtype.type(math.sqrt(1.0 / (D // NHEAD)))
    q = _heads(_lin(xq, W[:D], B[:D]), bs) * qs
    k = _heads(_lin(xkv, W[D:2 * D], B[D:2 * D]), bs)
    v = _heads(_lin(xkv, W[2 * D:], B[2 * D:]), bs)
    sc = np.matmul(q, k.transpose(0, 2, 1))
    if key_mask is not None:
        sc = np.where(np.repeat(key_mask, NHEAD, axis=0)[:, None, :], xq.dtype.type(-np.inf), sc)
    p = _softmax(sc)
    out = _lin(_unheads(np.matmul(p, v), bs), P(pre + "out_proj.weight"), P(pre + "out_proj.bias"))
    return out, (q, k, v, p)


def _attn_bwd(P, pre, saved, g, bs):
    """Gradient at the attention's output -> (at the query-side input, at the key / value-side input), both in front of the in-projection."""
    q, k, v, p = saved
    W = P(pre + "in_proj_weight")
    qs = g.dtype.type(math.sqrt(1.0 / (D // NHEAD)))
    do = _heads(np.matmul(g, P(pre + "out_proj.weight")), bs)
    ds = _softmax_bwd(p, np.matmul(do, v.transpose(0, 2, 1)))
    dq = _unheads(np.matmul(ds, k), bs) * qs
    dk = _unheads(np.matmul(ds.transpose(0, 2, 1), q), bs)
    dv = _unheads(np.matmul(p.transpose(0, 2, 1), do), bs)
    return np.matmul(dq, W[:D]), np.matmul(dk, W[D:2 * D]) + np.matmul(dv, W[2 * D:])


def decode_forward(sd, z, lengths, num_layers=5, dtype=np.float64):
    """(feats [bs, nframes, 189], saved state for ``decode_sweep``, taps)."""
    P = _Net(sd, dtype)
    z = np.asarray(z, dtype=dtype)
    _, bs, n_chunks, _ = z.shape
    lengths = np.asarray(lengths)
    nframes = int(lengths.max())
    mask = np.arange(nframes)[None, :] < lengths[:, None]
    nb = (num_layers - 1) // 2
    taps, stacks, outs = {}, [], []
    queries = np.zeros((nframes, bs, D), dtype) + P("query_pos_decoder.pe")[:nframes].reshape(nframes, 1, D)
    for s, part in enumerate(PARTS):
        pre = part + "_decoder."
        mem = z[s].transpose(1, 0, 2) + P("mem_pos_decoder.pe")[:n_chunks].reshape(n_chunks, 1, D)
        x, xs, layers = queries, [], []
        for l, p in enumerate(layer_prefixes(pre, num_layers)):
            if l > nb:
                j = l - nb - 1
                x = _lin(np.concatenate([x, xs.pop()], axis=-1), P(f"{pre}linear_blocks.{j}.weight"), P(f"{pre}linear_blocks.{j}.bias"))
            taps[f"x.{s}.{l}"] = x
            sv = {"x0": x}
            n1 = _ln(x, P(p + "norm1.weight"), P(p + "norm1.bias"))
            o, sv["self"] = _attn_fwd(P, p + "self_attn.", n1, n1, bs, ~mask)
            x = x + o
            sv["x1"] = x
            o, sv["cross"] = _attn_fwd(P, p + "multihead_attn.", _ln(x, P(p + "norm2.weight"), P(p + "norm2.bias")), mem, bs, None)
            x = x + o
            sv["x2"] = x
            sv["pre"] = _lin(_ln(x, P(p + "norm3.weight"), P(p + "norm3.bias")), P(p + "linear1.weight"), P(p + "linear1.bias"))
            x = x + _lin(_gelu(sv["pre"]), P(p + "linear2.weight"), P(p + "linear2.bias"))
            if l < nb:
                xs.append(x)
            layers.append(sv)
        taps[f"x.{s}.{num_layers}"] = x
        outs.append(_lin(_ln(x, P(pre + "norm.weight"), P(pre + "norm.bias")), P(part + "_final_layer.weight"), P(part + "_final_layer.bias")))
        stacks.append((layers, x))
    out = np.concatenate(outs, axis=-1)
    out[~mask.T] = 0
    state = dict(P=P, stacks=stacks, mask=mask, bs=bs, n_chunks=n_chunks, num_layers=num_layers, dtype=dtype)
    return np.ascontiguousarray(out.transpose(1, 0, 2)), state, taps


def decode_sweep(state, d_feats, taps=None):
    """d_z [2, bs, n_chunks, 128] for the cotangent d_feats [bs, nframes, 189] at decode's output; fills ``taps`` when given."""
    P, mask, bs, nl, dtype = state["P"], state["mask"], state["bs"], state["num_layers"], state["dtype"]
    nb = (nl - 1) // 2
    d_out = np.asarray(d_feats, dtype=dtype).transpose(1, 0, 2).copy()
    d_out[~mask.T] = 0
    d_z = np.zeros((2, bs, state["n_chunks"], D), dtype)
    for s, part in enumerate(PARTS):
        pre = part + "_decoder."
        layers, x_last = state["stacks"][s]
        cols = slice(0, BODY) if s == 0 else slice(BODY, BODY + HANDS)
        g = _ln_bwd(x_last, P(pre + "norm.weight"), np.matmul(d_out[..., cols], P(part + "_final_layer.weight")))
        gskip = {}
        prefixes = layer_prefixes(pre, nl)
        for l in reversed(range(nl)):
            p, sv = prefixes[l], layers[l]
            if l < nb:
                g = g + gskip[l]
            if taps is not None:
                taps[f"g.{s}.{l}"] = g
            dpre = np.matmul(g, P(p + "linear2.weight")) * _gelu_grad(sv["pre"])
            g = g + _ln_bwd(sv["x2"], P(p + "norm3.weight"), np.matmul(dpre, P(p + "linear1.weight")))
            dn2, dmem = _attn_bwd(P, p + "multihead_attn.", sv["cross"], g, bs)
            dzl = dmem.transpose(1, 0, 2)
            d_z[s] += dzl
            if taps is not None:
                taps[f"dz.{s}.{l}"] = dzl
            g = g + _ln_bwd(sv["x1"], P(p + "norm2.weight"), dn2)
            if l == 0:
                break                                   # the queries are constants: nothing below layer 0's cross-attention reaches z
            dq, dkv = _attn_bwd(P, p + "self_attn.", sv["self"], g, bs)
            g = g + _ln_bwd(sv["x0"], P(p + "norm1.weight"), dq + dkv)
            if l > nb:
                j = l - nb - 1
                dcat = np.matmul(g, P(f"{pre}linear_blocks.{j}.weight"))
                g, gskip[nb - 1 - j] = dcat[..., :D], dcat[..., D:]
    return d_z


def decode_vjp(sd, z, lengths, d_feats, num_layers=5, dtype=np.float64):
    """(feats, d_z, taps) of one forward and one sweep."""
    feats, state, taps = decode_forward(sd, z, lengths, num_layers, dtype)
    d_z = decode_sweep(state, d_feats, taps)
    return feats, d_z, taps


# ----------------------------------------------------------------------------- the cases of tests/golden/vae_decode_vjp.npz
# name -> (z shape, lengths, z scale).  ragged / single / long are the latents of tests/golden/vae_decode.npz (make_golden_vae.py draws them
# from PCG64(77) in this order), so the forward is pinned by that file too; tiny has its own seed.  The cotangent of every case is seeded.
CASES = {
    "tiny": ((2, 2, 2, 128), [17, 1], 1.0),
    "single": ((2, 1, 8, 128), [64], 1.0),
    "ragged": ((2, 3, 8, 128), [128, 100, 37], 1.0),
    "long": ((2, 2, 16, 128), [200, 256], 1.5),
}


def case_inputs(name):
    """(z float32, lengths, d_feats float32 [bs, nframes, 189]) of a case, regenerated from seeds."""
    rng = np.random.Generator(np.random.PCG64(77))
    zs = {}
    for n in ("ragged", "single", "long"):
        shape, _, scale = CASES[n]
        z = rng.standard_normal(shape, dtype=np.float32)
        zs[n] = z if scale == 1.0 else np.float32(scale) * z
    shape, lengths, _ = CASES[name]
    z = zs[name] if name in zs else np.random.Generator(np.random.PCG64(7701)).standard_normal(shape, dtype=np.float32)
    d = np.random.Generator(np.random.PCG64(4200 + len(name))).standard_normal((shape[1], max(lengths), BODY + HANDS), dtype=np.float32)
    return z, list(lengths), d


DEPTH_CASE = ((2, 2, 3, 128), [40, 17])   # three row tiles; the case of tests/golden/vae_depths.npz and tests/test_gpu_vae_depths.py


def depth_case_inputs():
    """(z float32, lengths, d_feats float32) of DEPTH_CASE, seeded like ``case_inputs``; the same at every depth."""
    shape, lengths = DEPTH_CASE
    z = np.random.Generator(np.random.PCG64(7702)).standard_normal(shape, dtype=np.float32)
    d = np.random.Generator(np.random.PCG64(4200 + len("depths"))).standard_normal((shape[1], max(lengths), BODY + HANDS), dtype=np.float32)
    return z, list(lengths), d


def errors(got, want):
    """(relative L2, worst 128-wide row: the row's error norm over the RMS row norm) of gradients with a last axis of 128."""
    got, want = np.asarray(got, np.float64).reshape(-1, D), np.asarray(want, np.float64).reshape(-1, D)
    err = np.linalg.norm(got - want, axis=-1)
    rms = math.sqrt(float((want * want).sum()) / want.shape[0]) + 1e-300
    return float(np.linalg.norm(err) / (np.linalg.norm(want) + 1e-300)), float(err.max() / rms)
