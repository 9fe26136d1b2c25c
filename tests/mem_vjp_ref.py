"""High-precision restatement of the vector-Jacobian product of one denoiser forward with respect to its sample AND its five
memories -- TEST INFRASTRUCTURE.

``tests/vjp_ref.out_and_vjp`` (the reference's UNFOLDED formulation, from the blocks of ``tests/weg_bwd_ref.py``) with the key side of
every cross-attention added: for layer i, memory j and batch row r, with ``m = mem_j[r] + temb + condition_embedding[j] + mem_pos.pe``,
``mh = LN_ij(m)``, ``k = Wk mh + bk``, ``v = Wv mh + bv``, ``q`` the scaled query and ``dS`` the softmax backward of ``dP = do . v^T``:

    dk = dS^T q      dv = p^T do      dmh = dk Wk + dv Wv      d_mem_j[r] = sum_i LN_ij'(dmh)

Masked keys have p = 0 and dS = 0, so their gradient is exactly 0.  One memory per batch row: a caller with row maps expands them and
sums the rows of an instance (``sum_instances``).  float64 is what ``cfd_denoise_vjp_mem`` is measured against
(tests/test_gpu_mem_vjp.py), the same code at float32 the yardstick; pinned on the CPU against float32 torch autograd through
``oracle.denoiser_torch`` by tests/test_mem_vjp_host.py.
"""
import math

import numpy as np

from oracle.denoiser_ref import D, MEM_NAMES, timestep_embedding
from tests.weg_bwd_ref import (_gelu, _gelu_grad, _lin, _ln, _ln_bwd, _Net, _silu, _silu_grad, _softmax, _softmax_bwd)


def out_and_vjp_mem(sd, sample, t, encoder_hidden_states, masks, d_out, dtype=np.float64, num_layers=9, nhead=4):
    """(out [B, L, 128], d_out^T . d(out)/d(sample) [B, L, 128], [d_out^T . d(out)/d(memory j) [B, S_j, 512] for the five memories])."""
    dt = np.dtype(dtype).type
    P = _Net(sd, dtype)
    masks = dict(masks or {})
    # ---- forward (denoiser.py:173-386, cross_attention.py:556-664), keeping what the sweep needs
    x = _lin(np.asarray(sample, dtype=dtype).transpose(1, 0, 2), P("latent_embd.weight"), P("latent_embd.bias"))
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

    def time_block(p, x):
        e = _lin(_silu(temb), P(p + "emb_layers.1.weight"), P(p + "emb_layers.1.bias"))
        h = _ln(x, P(p + "norm.weight"), P(p + "norm.bias")) * (1.0 + e[..., :D]) + e[..., D:]
        return x + _lin(_silu(h), P(p + "out_layers.2.weight"), P(p + "out_layers.2.bias")), (h, e[..., :D])

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
        x, sv["tb1"] = time_block(p + "time_block1.", x)
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
            sv["cross"].append((kj, vj, pj, qj))
        x = x + _lin(np.concatenate(outs, axis=-1), P(p + "att_fuser.weight"), P(p + "att_fuser.bias"))
        sv["x3"] = x
        x, sv["tb2"] = time_block(p + "time_block2.", x)
        sv["x4"] = x
        n3 = _ln(x, P(p + "norm3.weight"), P(p + "norm3.bias"))
        sv["pre"] = _lin(n3, P(p + "linear1.weight"), P(p + "linear1.bias"))
        x = x + _lin(_gelu(sv["pre"]), P(p + "linear2.weight"), P(p + "linear2.bias"))
        saved.append(sv)
    out = _lin(_ln(x, P("decoder.norm.weight"), P("decoder.norm.bias")), P("latent_proj.weight"), P("latent_proj.bias"))

    # ---- reverse sweep from the output; g = gradient at the residual stream, top down
    dnf = np.matmul(np.asarray(d_out, dtype=dtype).transpose(1, 0, 2), P("latent_proj.weight"))
    g = _ln_bwd(x, P("decoder.norm.weight"), dnf)
    d_mem = [np.zeros_like(m) for m in mems]                                              # [S_j, B, 512]
    for i in reversed(range(num_layers)):
        p = f"decoder.layers.{i}."
        sv = saved[i]
        d1 = np.matmul(g, P(p + "linear2.weight")) * _gelu_grad(sv["pre"])
        g = g + _ln_bwd(sv["x4"], P(p + "norm3.weight"), np.matmul(d1, P(p + "linear1.weight")))
        h, scale = sv["tb2"]
        dz = np.matmul(g, P(p + "time_block2.out_layers.2.weight"))
        g = g + _ln_bwd(sv["x3"], P(p + "time_block2.norm.weight"), dz * _silu_grad(h) * (1.0 + scale))
        dcat = np.matmul(g, P(p + "att_fuser.weight"))
        dn2 = np.zeros_like(g)
        for j, name in enumerate(MEM_NAMES):
            a = p + "multihead_attn_" + name
            kj, vj, pj, qj = sv["cross"][j]
            do = np.matmul(dcat[..., j * D:(j + 1) * D], P(a + ".out_proj.weight")).transpose(1, 0, 2)
            ds = _softmax_bwd(pj, np.matmul(do, vj.transpose(0, 2, 1)))
            dq = (np.matmul(ds, kj) * xs).transpose(1, 0, 2)
            dn2 = dn2 + np.matmul(dq, P(a + ".in_proj_weight")[:D])
            # the key side: dk = dS^T q (q the scaled query), dv = p^T do, through Wk | Wv and this layer's memory LayerNorm
            Wi = P(a + ".in_proj_weight")
            dk = np.matmul(ds.transpose(0, 2, 1), qj).transpose(1, 0, 2)                 # [S, B, D]
            dv = np.matmul(pj.transpose(0, 2, 1), do).transpose(1, 0, 2)
            dmh = np.matmul(dk, Wi[D:2 * D]) + np.matmul(dv, Wi[2 * D:])
            d_mem[j] = d_mem[j] + _ln_bwd(mems[j], P(p + name + "_norm.weight"), dmh)
        g = g + _ln_bwd(sv["x2"], P(p + "norm2.weight"), dn2)
        h, scale = sv["tb1"]
        dz = np.matmul(g, P(p + "time_block1.out_layers.2.weight"))
        g = g + _ln_bwd(sv["x1"], P(p + "time_block1.norm.weight"), dz * _silu_grad(h) * (1.0 + scale))
        q, k, v, pr = sv["self"]
        do = heads(np.matmul(g, P(p + "self_attn.out_proj.weight")))
        ds = _softmax_bwd(pr, np.matmul(do, v.transpose(0, 2, 1)))
        dqkv = np.concatenate([unheads(np.matmul(ds, k)) * qs, unheads(np.matmul(ds.transpose(0, 2, 1), q)),
                               unheads(np.matmul(pr.transpose(0, 2, 1), do))], axis=-1)
        g = g + _ln_bwd(sv["x0"], P(p + "norm1.weight"), np.matmul(dqkv, P(p + "self_attn.in_proj_weight")))
    grad = np.ascontiguousarray(np.matmul(g, P("latent_embd.weight")).transpose(1, 0, 2))
    return np.ascontiguousarray(out.transpose(1, 0, 2)), grad, [np.ascontiguousarray(m.transpose(1, 0, 2)) for m in d_mem]


def sum_instances(d_mem_rows, row_map, U):
    """Per-row gradients [Be, S, 512] -> per-instance sums [U, S, 512] (ascending row order; an instance no row maps to stays zero)."""
    out = np.zeros((U,) + d_mem_rows.shape[1:], dtype=d_mem_rows.dtype)
    for b, u in enumerate(np.asarray(row_map).reshape(-1)):
        out[int(u)] += d_mem_rows[b]
    return out
