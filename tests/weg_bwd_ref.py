"""High-precision restatement of one word-excitation-guidance evaluation with gradient taps -- TEST INFRASTRUCTURE.

The saved forward, the attend-and-excite objective and the reverse sweep of ``oracle/weg_ref.py`` (``forward_saved`` /
``focus_loss`` / ``backward_to_sample``) written again in the reference's UNFOLDED formulation, in one numpy dtype chosen by the
caller: float64 is the reference the HIP reverse sweep is measured against launch by launch (tests/test_gpu_weg_backward.py), the
same code at float32 is the yardstick (how far plain float32 arithmetic lands from float64 at the same tap).  Nothing here looks
at the kernels: no folded keys, no per-key scales, no cells.

What counts as INPUT and is therefore taken in float32 and cast: the weights, the latents and memories, the sinusoid row of the
timestep (a load-time float32 table in the reference and in the product) and the 3x3 smoothing kernel.

Layout: activations and gradients are [L, B, C] (sequence first, as the reference's decoder); ``rows()`` turns a tap into the
product's token-row order [B * L, C] (row b * L + t).

Taps (``l`` = layer):
  gx.l.k    gradient at the residual stream where the product saves it: k = 0 the layer's input, 1 after self-attention, 2 after
            time block 1, 3 after the cross-attention, 4 after time block 2.  gx.0.0 is the gradient at the embedding's output
            ("g_emb"), gx.(l+1).0 the gradient at layer l's output; "g_out" is the gradient at the last layer's output (zero: the
            objective reads the attention maps only, so gx.(last).3 and .4 are zero too)
  dpre.l    at the FFN pre-activation              dn1.l / dn2.l / dn3.l   at the norm1 / norm2 / norm3 output
  dz1.l / dz2.l  at the SiLU output of time block 1 / 2 (the input of its last linear layer)
  dO.l      at the self-attention core's output, before out_proj
  dqkv.l    at the packed in-projection's output [L, B, 1536]: dq (at the UNSCALED query) | dk | dv
  dP.l.j    at the cross-attention probabilities of memory j [B, L, S_j]          p.l.j  those probabilities
  x.l.k     the forward's residual stream at the five points
"""
import math

import numpy as np
from scipy.special import erf

from oracle import weg_ref
from oracle.denoiser_ref import D, MEM_NAMES, timestep_embedding

TLSN = 2


def rows(tap):
    """[L, B, C] -> [B * L, C], the product's token-row order."""
    return np.ascontiguousarray(np.transpose(tap, (1, 0, 2))).reshape(-1, tap.shape[-1])


class _Net:
    def __init__(self, sd, dtype):
        self.sd, self.dt, self.c = sd, dtype, {}

    def __call__(self, key):
        if key not in self.c:
            self.c[key] = np.asarray(self.sd[key], dtype=self.dt)
        return self.c[key]


def _lin(x, w, b=None):
    y = np.matmul(x, w.T)
    return y if b is None else y + b


def _ln_stats(x, eps=1e-5):
    mu = x.mean(axis=-1, keepdims=True)
    xc = x - mu
    rstd = 1.0 / np.sqrt((xc * xc).mean(axis=-1, keepdims=True) + x.dtype.type(eps))
    return xc * rstd, rstd


def _ln(x, g, b):
    return _ln_stats(x)[0] * g + b


def _ln_bwd(x, g, dy):
    xh, rstd = _ln_stats(x)
    dh = dy * g
    return rstd * (dh - dh.mean(axis=-1, keepdims=True) - xh * (dh * xh).mean(axis=-1, keepdims=True))


def _sigmoid(x):
    return 1.0 / (1.0 + np.exp(-x))


def _silu(x):
    return x * _sigmoid(x)


def _silu_grad(x):
    s = _sigmoid(x)
    return s * (1.0 + x * (1.0 - s))


def _gelu(x):
    return x * 0.5 * (1.0 + erf(x * x.dtype.type(1.0 / math.sqrt(2.0))))


def _gelu_grad(x):
    t = x.dtype.type
    return 0.5 * (1.0 + erf(x * t(1.0 / math.sqrt(2.0)))) + x * np.exp(-0.5 * x * x) * t(1.0 / math.sqrt(2.0 * math.pi))


def _softmax(sc):
    e = np.exp(sc - sc.max(axis=-1, keepdims=True))
    return e / e.sum(axis=-1, keepdims=True)


def _softmax_bwd(p, dp):
    return p * (dp - (dp * p).sum(axis=-1, keepdims=True))


# ----------------------------------------------------------------------------- the objective
def focus_loss(att, focus_indices, normalize_eot, eot_indices):
    """word_excitation_guidance.py:11-81 on the maps [B, layers, L, S] in their own dtype: mean over the layers, the text slice
    [1, last), softmax over it, 3x3 reflect-padded smoothing, per focus token the largest entry over the frames, loss = mean over
    the batch of mean_i max(0, 1 - value).  Returns (loss, losses [B], max_att list of lists, d loss / d att)."""
    dt = att.dtype.type
    B, NL, L, S = att.shape
    A = att.mean(axis=1)
    last = int(eot_indices[0]) if normalize_eot else -1
    X = A[:, :, 1:last]
    W = X.shape[2]
    sm = _softmax(X)
    K = weg_ref.gaussian_kernel().astype(att.dtype)
    pad = np.pad(sm, ((0, 0), (1, 1), (1, 1)), mode="reflect")
    sg = np.zeros_like(sm)
    for a in range(3):
        for b in range(3):
            sg = sg + K[a, b] * pad[:, a:a + L, b:b + W]
    dsg = np.zeros_like(sg)
    max_att, losses = [], []
    for b in range(B):
        vals = []
        nt = len(focus_indices[b])
        for i in focus_indices[b]:
            col = sg[b, :, i - 1]
            ls = int(np.argmax(col))
            vals.append(col[ls])
            if 1.0 - col[ls] > 0:
                dsg[b, ls, i - 1] -= dt(1.0 / (nt * B))
        max_att.append(vals)
        losses.append(np.mean([max(dt(0), dt(1) - v) for v in vals]) if vals else dt(0))
    losses = np.asarray(losses, dtype=att.dtype)
    loss = losses.mean()
    # the smoothing backwards: every padded cell hands its share to the cell it mirrors
    dpad = np.zeros((B, L + 2, W + 2), dtype=att.dtype)
    for a in range(3):
        for b in range(3):
            dpad[:, a:a + L, b:b + W] += K[a, b] * dsg
    src_l = np.pad(np.arange(L), 1, mode="reflect")
    src_w = np.pad(np.arange(W), 1, mode="reflect")
    dsm = np.zeros_like(sm)
    for i, li in enumerate(src_l):
        for k, wk in enumerate(src_w):
            dsm[:, li, wk] += dpad[:, i, k]
    dX = _softmax_bwd(sm, dsm)
    dA = np.zeros_like(A)
    dA[:, :, 1:last] = dX
    d_att = np.repeat((dA / dt(NL))[:, None], NL, axis=1)
    return loss, losses, max_att, d_att


# ----------------------------------------------------------------------------- forward, objective, reverse sweep
def loss_and_grad_taps(sd, latents, t, encoder_hidden_states, cond_masks, focus_indices, normalize_eot=True, eot_indices=None,
                       dtype=np.float64, num_layers=9, nhead=4):
    """One evaluation.  Returns (loss, losses [B], max_att, grad [B, L, 128], taps dict, att_tlsn [B, layers, L, S], d_att)."""
    dt = np.dtype(dtype).type
    P = _Net(sd, dtype)
    masks = dict(cond_masks or {})
    if eot_indices is None:
        eot_indices = np.argmax(np.asarray(masks["tlsn"]).astype(np.int64), axis=1) - 1
    taps = {}
    # ---- forward (denoiser.py:173-386, cross_attention.py:556-664), keeping what the sweep needs
    x = _lin(np.asarray(latents, dtype=dtype).transpose(1, 0, 2), P("latent_embd.weight"), P("latent_embd.bias"))
    L, B, _ = x.shape
    temb = timestep_embedding(np.full((B,), float(t))).astype(dtype)                     # (a float32 table row: input)
    temb = _lin(_silu(_lin(temb, P("time_embedding.linear_1.weight"), P("time_embedding.linear_1.bias"))),
                P("time_embedding.linear_2.weight"), P("time_embedding.linear_2.bias"))[None]
    mems = [np.asarray(m, dtype=dtype).transpose(1, 0, 2) + temb for m in encoder_hidden_states]
    x = x.copy()
    x[0::2] += P("bh_embedding.weight")[0] + P("query_pos.pe")[: L // 2]
    x[1::2] += P("bh_embedding.weight")[1] + P("query_pos.pe")[: L // 2]
    for j in range(5):
        mems[j] = (mems[j] + P("condition_embedding.weight")[j]) + P("mem_pos.pe")[: mems[j].shape[0]]
    hd = D // nhead
    qs, xs = dt(math.sqrt(1.0 / hd)), dt(math.sqrt(1.0 / D))
    heads = lambda a: a.reshape(a.shape[0], B * nhead, hd).transpose(1, 0, 2)            # [n, B, D] -> [B H, n, hd]
    unheads = lambda a: a.transpose(1, 0, 2).reshape(a.shape[1], B, D)
    saved = []
    for i in range(num_layers):
        p = f"decoder.layers.{i}."
        sv = {"x0": x}
        n1 = _ln(x, P(p + "norm1.weight"), P(p + "norm1.bias"))
        qkv = _lin(n1, P(p + "self_attn.in_proj_weight"), P(p + "self_attn.in_proj_bias"))
        q, k, v = heads(qkv[..., :D]) * qs, heads(qkv[..., D:2 * D]), heads(qkv[..., 2 * D:])
        pr = _softmax(np.matmul(q, k.transpose(0, 2, 1)))
        sv["self"] = (q, k, v, pr)
        x = x + _lin(unheads(np.matmul(pr, v)), P(p + "self_attn.out_proj.weight"), P(p + "self_attn.out_proj.bias"))
        sv["x1"] = x
        for tb, key in (("time_block1.", "tb1"),):
            e = _lin(_silu(temb), P(p + tb + "emb_layers.1.weight"), P(p + tb + "emb_layers.1.bias"))
            h = _ln(x, P(p + tb + "norm.weight"), P(p + tb + "norm.bias")) * (1.0 + e[..., :D]) + e[..., D:]
            sv[key] = (h, e[..., :D])
            x = x + _lin(_silu(h), P(p + tb + "out_layers.2.weight"), P(p + tb + "out_layers.2.bias"))
        sv["x2"] = x
        n2 = _ln(x, P(p + "norm2.weight"), P(p + "norm2.bias"))
        outs, sv["cross"] = [], []
        for j, name in enumerate(MEM_NAMES):
            a = p + "multihead_attn_" + name
            Wi, bi = P(a + ".in_proj_weight"), P(a + ".in_proj_bias")
            m = _ln(mems[j], P(p + name + "_norm.weight"), P(p + name + "_norm.bias"))
            qj = (_lin(n2, Wi[:D], bi[:D]) * xs).transpose(1, 0, 2)                      # [B, L, D] (one head)
            kj = _lin(m, Wi[D:2 * D], bi[D:2 * D]).transpose(1, 0, 2)                    # [B, S, D]
            vj = _lin(m, Wi[2 * D:], bi[2 * D:]).transpose(1, 0, 2)
            sc = np.matmul(qj, kj.transpose(0, 2, 1))
            mk = masks.get(name)
            if mk is not None:
                sc = np.where(np.asarray(mk, dtype=bool)[:, None, :], dt(-np.inf), sc)
            pj = _softmax(sc)
            outs.append(_lin(np.matmul(pj, vj).transpose(1, 0, 2), P(a + ".out_proj.weight"), P(a + ".out_proj.bias")))
            sv["cross"].append((kj, vj, pj))
            taps[f"p.{i}.{j}"] = pj
        x = x + _lin(np.concatenate(outs, axis=-1), P(p + "att_fuser.weight"), P(p + "att_fuser.bias"))
        sv["x3"] = x
        e = _lin(_silu(temb), P(p + "time_block2.emb_layers.1.weight"), P(p + "time_block2.emb_layers.1.bias"))
        h = _ln(x, P(p + "time_block2.norm.weight"), P(p + "time_block2.norm.bias")) * (1.0 + e[..., :D]) + e[..., D:]
        sv["tb2"] = (h, e[..., :D])
        x = x + _lin(_silu(h), P(p + "time_block2.out_layers.2.weight"), P(p + "time_block2.out_layers.2.bias"))
        sv["x4"] = x
        n3 = _ln(x, P(p + "norm3.weight"), P(p + "norm3.bias"))
        sv["pre"] = _lin(n3, P(p + "linear1.weight"), P(p + "linear1.bias"))
        x = x + _lin(_gelu(sv["pre"]), P(p + "linear2.weight"), P(p + "linear2.bias"))
        for kk in range(5):
            taps[f"x.{i}.{kk}"] = sv[f"x{kk}"]
        saved.append(sv)
    taps[f"x.{num_layers}.0"] = x
    att = np.stack([taps[f"p.{i}.{TLSN}"] for i in range(num_layers)], axis=1)            # [B, layers, L, S]
    loss, losses, max_att, d_att = focus_loss(att, focus_indices, normalize_eot, eot_indices)

    # ---- reverse sweep; g = gradient at the residual stream, top down
    g = np.zeros_like(x)
    taps["g_out"] = g
    live = False                                                                        # anything above this point reaches the objective
    for i in reversed(range(num_layers)):
        p = f"decoder.layers.{i}."
        sv = saved[i]
        taps[f"gx.{i + 1}.0"] = g
        if live:
            taps[f"dpre.{i}"] = d1 = np.matmul(g, P(p + "linear2.weight")) * _gelu_grad(sv["pre"])
            taps[f"dn3.{i}"] = dn3 = np.matmul(d1, P(p + "linear1.weight"))
            g = g + _ln_bwd(sv["x4"], P(p + "norm3.weight"), dn3)
            taps[f"gx.{i}.4"] = g
            h, scale = sv["tb2"]
            taps[f"dz2.{i}"] = dz = np.matmul(g, P(p + "time_block2.out_layers.2.weight"))
            g = g + _ln_bwd(sv["x3"], P(p + "time_block2.norm.weight"), dz * _silu_grad(h) * (1.0 + scale))
            taps[f"gx.{i}.3"] = g
        else:
            taps[f"gx.{i}.4"] = taps[f"gx.{i}.3"] = g
        dcat = np.matmul(g, P(p + "att_fuser.weight")) if live else None
        dn2 = np.zeros_like(g)
        for j, name in enumerate(MEM_NAMES):
            if not live and j != TLSN:
                continue
            a = p + "multihead_attn_" + name
            kj, vj, pj = sv["cross"][j]
            dp = np.zeros_like(pj)
            if live:
                do = np.matmul(dcat[..., j * D:(j + 1) * D], P(a + ".out_proj.weight")).transpose(1, 0, 2)
                dp = np.matmul(do, vj.transpose(0, 2, 1))
            if j == TLSN:
                dp = dp + d_att[:, i]
            taps[f"dP.{i}.{j}"] = dp
            dq = (np.matmul(_softmax_bwd(pj, dp), kj) * xs).transpose(1, 0, 2)
            dn2 = dn2 + np.matmul(dq, P(a + ".in_proj_weight")[:D])
        taps[f"dn2.{i}"] = dn2
        g = g + _ln_bwd(sv["x2"], P(p + "norm2.weight"), dn2)
        live = True
        taps[f"gx.{i}.2"] = g
        h, scale = sv["tb1"]
        taps[f"dz1.{i}"] = dz = np.matmul(g, P(p + "time_block1.out_layers.2.weight"))
        g = g + _ln_bwd(sv["x1"], P(p + "time_block1.norm.weight"), dz * _silu_grad(h) * (1.0 + scale))
        taps[f"gx.{i}.1"] = g
        taps[f"dO.{i}"] = dO = np.matmul(g, P(p + "self_attn.out_proj.weight"))
        q, k, v, pr = sv["self"]
        do = heads(dO)
        ds = _softmax_bwd(pr, np.matmul(do, v.transpose(0, 2, 1)))
        dq = unheads(np.matmul(ds, k)) * qs                                             # at the projection's output, in front of the scale
        dk = unheads(np.matmul(ds.transpose(0, 2, 1), q))
        dv = unheads(np.matmul(pr.transpose(0, 2, 1), do))
        taps[f"dqkv.{i}"] = dqkv = np.concatenate([dq, dk, dv], axis=-1)
        taps[f"dn1.{i}"] = dn1 = np.matmul(dqkv, P(p + "self_attn.in_proj_weight"))
        g = g + _ln_bwd(sv["x0"], P(p + "norm1.weight"), dn1)
    taps["gx.0.0"] = taps["g_emb"] = g
    grad = np.ascontiguousarray(np.matmul(g, P("latent_embd.weight")).transpose(1, 0, 2))
    return loss, losses, max_att, grad, taps, att, d_att


# ----------------------------------------------------------------------------- the two error measures of the tap tests
def tap_errors(got, want):
    """(relative L2 over the tap, worst row: the row's error norm over the tap's RMS row norm) of [rows, C] arrays."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    err = np.linalg.norm(got - want, axis=-1)
    rms = math.sqrt(float((want * want).sum()) / want.shape[0]) + 1e-300
    return float(np.linalg.norm(err) / (np.linalg.norm(want) + 1e-300)), float(err.max() / rms)


# ----------------------------------------------------------------------------- the cases of the launch-by-launch test
# name -> (B, L, S, pad_tail, timestep, focus tokens); seeded weights 1234 / 1.0, no end-of-text normalisation (last = S_tlsn - 1)
BWD_CASES = {
    "ragged_b2": (2, 20, (6, 40, 12, 8, 1), (2, 5, 3, 0, 0), 613, [[2, 5], [1, 7]]),     # ragged second query tile, two batch rows, several 16-key blocks
    "big_keys": (1, 16, (24, 530, 24, 8, 1), (0, 0, 0, 0, 0), 250, [[3, 9, 22]]),        # 32 + 544 + 3 * 32 = 672 padded keys > 512
    "tiny": (1, 4, (3, 5, 6, 2, 1), (0, 0, 0, 0, 0), 37, [[1, 4]]),                       # one partial tile, every memory inside one key block
}
_cache = {}


def bwd_case(name, dtype=np.float64):
    """(inputs, timestep, focus, result of loss_and_grad_taps) of a case, computed once per dtype."""
    from oracle import inputs
    from tests.helpers import state_dict
    B, L, S, pad, t, focus = BWD_CASES[name]
    key = (name, np.dtype(dtype).name)
    if key not in _cache:
        inp = inputs.make_plain_batch(seed=900 + len(name), Be=B, L=L, S=S, pad_tail=pad)
        _cache[key] = (inp, loss_and_grad_taps(state_dict(1234, 1.0), inp["sample"], t, inp["memories"], inp["masks"], focus, False, (), dtype))
    inp, res = _cache[key]
    return inp, t, focus, res


def tap_class(key):
    """The gate class of a tap: its name without layer and memory."""
    return key.split(".")[0]


def tap_rows(key, tap):
    return tap.reshape(-1, tap.shape[-1]) if key.startswith(("dP.", "p.")) else rows(tap)
