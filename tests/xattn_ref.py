"""The cross-attention block of one decoder layer (cross_attention.py:578-652) in plain numpy, two ways -- the yardsticks of
tests/test_gpu_xattn_block.py, checked against each other on the CPU by tests/test_xattn_ref_host.py.

  block_unfolded   the reference formulation: LayerNorm2 of the rows, per memory its LayerNorm, one-head attention with in- and out-projection,
                   the five outputs side by side through att_fuser.
  block_folded     the form the fused kernel computes: with a_s the centred static part of a memory row, b the centred
                   timestep embedding and rs_s the row's 1 / sigma,
                       score(q, s) = rs_s (q . KA_s + c_q) + cbk_s,   c_q = q . (A b),   cbk_s = rs_s (c . a_s + c . b)
                       O = VA^T P',  P' = p rs,      update = sum_j [O_j + (sum_s P'_s) VV_j b] + folded bias
                   everything built from the state dict in `dtype`.  `round_ops`, a subset of {"q", "k", "v", "p"}, rounds operands of the LONG
                   memories (>= 128 padded keys) through np.float16 where the kernel's F16 instance does (csrc/xattn_fused.hpp): the LayerNorm2
                   rows that meet KA (not c_q: it is made from the full rows), KA, VA, and P' -- per 32-key tile, relative to the running
                   maximum of the tiles so far, which is how the online softmax forms it; the sums (sum p, sum P') stay unrounded.

Shapes: x_in [Be][L][512]; mem_taps: the oracle's taps "mem.<name>" [S_j][U_j][512] (memory + temb + condition id + PE, float32) and "temb"
[1][*][512] (one timestep: every row the same); masks: name -> bool [U_j][S_j] or None; row_map: None (U_j = Be, row b uses instance b) or five
int arrays [Be].  Both functions return (update [Be][L][512], [five probabilities [Be][L][S_j]]).  A row whose keys of one memory are all
masked is NaN, as in the reference.  dtype=np.float32 is the float32 restatement of either form.
"""
import numpy as np

from oracle import denoiser_ref

MEM_NAMES = denoiser_ref.MEM_NAMES
D = 512
TILE = 32
LONG_KEYS = 128      # XA_F16_MIN_KEYS


def memory_taps(sd, t, memories):
    """The taps "temb" and "mem.<name>" of oracle.denoiser_ref.denoiser_forward (denoiser.py:195-261, 332-353) for one timestep t, without the
    forward: memories five [U_j][S_j][512] -> "mem.<name>" [S_j][U_j][512]."""
    R = denoiser_ref
    temb = R.timestep_embedding(np.asarray([t], dtype=np.float64))
    temb = R.linear(R.silu(R.linear(temb, sd["time_embedding.linear_1.weight"], sd["time_embedding.linear_1.bias"])),
                    sd["time_embedding.linear_2.weight"], sd["time_embedding.linear_2.bias"])[None]
    taps = {"temb": temb.copy()}
    for j, n in enumerate(MEM_NAMES):
        m = np.asarray(memories[j], dtype=np.float32).transpose(1, 0, 2) + temb
        taps["mem." + n] = (m + sd["condition_embedding.weight"][j]) + sd["mem_pos.pe"][: m.shape[0]]
    return taps


def _ln(x, w, b):
    xc = x - x.mean(-1, keepdims=True)
    return xc / np.sqrt((xc * xc).mean(-1, keepdims=True) + x.dtype.type(1e-5)) * w + b


def _f16(x):
    return x.astype(np.float16).astype(x.dtype)


def _softmax(sc):
    with np.errstate(invalid="ignore"):
        pr = np.exp(sc - sc.max(-1, keepdims=True))      # every key masked: (-inf) - (-inf) = NaN, as in the reference
        return pr / pr.sum(-1, keepdims=True)


def _groups(row_map, Be):
    rm = np.arange(Be) if row_map is None else np.asarray(row_map)
    return [(int(u), np.nonzero(rm == u)[0]) for u in np.unique(rm)]


class _Layer:
    def __init__(self, sd, layer, dtype):
        self.p = f"decoder.layers.{layer}."
        self.sd, self.dt = sd, dtype

    def __call__(self, key):
        return self.sd[self.p + key].astype(self.dt)


def block_unfolded(sd, layer, x_in, mem_taps, masks, row_map=None, dtype=np.float64):
    w = _Layer(sd, layer, dtype)
    x = np.asarray(x_in).astype(dtype)
    Be = x.shape[0]
    q_in = _ln(x, w("norm2.weight"), w("norm2.bias"))
    outs, probs = [], []
    for j, name in enumerate(MEM_NAMES):
        mem = mem_taps["mem." + name].astype(dtype).transpose(1, 0, 2)                     # [U][S][512]
        mn = _ln(mem, w(name + "_norm.weight"), w(name + "_norm.bias"))
        a = "multihead_attn_" + name
        wi, bi = w(a + ".in_proj_weight"), w(a + ".in_proj_bias")
        q = (q_in @ wi[:D].T + bi[:D]) / dtype(np.sqrt(512.0))
        k, v = mn @ wi[D:2 * D].T + bi[D:2 * D], mn @ wi[2 * D:].T + bi[2 * D:]
        o = np.empty_like(q)
        pr = np.empty(q.shape[:2] + (mem.shape[1],), dtype)
        for u, rows in _groups(None if row_map is None else row_map[j], Be):
            sc = q[rows] @ k[u].T
            if masks.get(name) is not None:
                sc = np.where(np.asarray(masks[name][u], dtype=bool)[None, None, :], dtype(-np.inf), sc)
            pr[rows] = _softmax(sc)
            o[rows] = pr[rows] @ v[u]
        outs.append(o @ w(a + ".out_proj.weight").T + w(a + ".out_proj.bias"))
        probs.append(pr)
    return np.concatenate(outs, -1) @ w("att_fuser.weight").T + w("att_fuser.bias"), probs


def _online_f16(sc, rs, va, dtype):
    """softmax(sc) (rs o VA) for one instance's rows, tile by tile as the kernel's online softmax walks it, P' through fp16: sc [R][L][S]
    (-inf on dead keys), rs [S], va [S][512] -> (O [R][L][512], sum_s P'_s [R][L], probabilities [R][L][S])."""
    S = sc.shape[-1]
    m = np.full(sc.shape[:-1], -np.inf, dtype)
    lsum, wl, O = np.zeros_like(m), np.zeros_like(m), np.zeros(sc.shape[:-1] + (D,), dtype)
    with np.errstate(invalid="ignore"):
        for s0 in range(0, S, TILE):
            t = sc[..., s0:s0 + TILE]
            m_new = np.maximum(m, t.max(-1))
            dead = np.isneginf(m_new)                      # nothing but dead keys so far: the tile contributes 0
            ref = np.where(dead, dtype(0), m_new)
            scale = np.where(dead, dtype(1), np.exp(m - ref))     # (first live tile: m = -inf -> 0, times sums that are still 0)
            e = np.exp(t - ref[..., None])
            pp = e * rs[s0:s0 + TILE]
            O = O * scale[..., None] + _f16(pp) @ va[s0:s0 + TILE]
            lsum = lsum * scale + e.sum(-1)
            wl = wl * scale + pp.sum(-1)
            m = m_new
        inv = dtype(1) / lsum                              # every key dead: 0 * inf = NaN
        pr = np.exp(sc - np.where(np.isneginf(m), dtype(0), m)[..., None]) * inv[..., None]
        return O * inv[..., None], wl * inv, pr


def block_folded(sd, layer, x_in, mem_taps, masks, row_map=None, round_ops=(), dtype=np.float64):
    assert set(round_ops) <= {"q", "k", "v", "p"}, round_ops
    w = _Layer(sd, layer, dtype)
    x = np.asarray(x_in).astype(dtype)
    Be = x.shape[0]
    q_in = _ln(x, w("norm2.weight"), w("norm2.bias"))
    q16 = _f16(q_in) if "q" in round_ops else q_in
    temb = mem_taps["temb"].reshape(-1, D)
    assert (temb == temb[0]).all(), "one timestep for all rows"
    temb = temb[0].astype(dtype)
    b = temb - temb.mean()
    scale = dtype(1.0 / np.sqrt(512.0))
    fuser = w("att_fuser.weight")
    update = np.zeros_like(x) + w("att_fuser.bias")
    probs = []
    for j, name in enumerate(MEM_NAMES):
        mem = mem_taps["mem." + name].astype(dtype).transpose(1, 0, 2)                     # [U][S][512]
        S = mem.shape[1]
        long_mem = (S + TILE - 1) // TILE * TILE >= LONG_KEYS
        stat = mem - temb
        a_s = stat - stat.mean(-1, keepdims=True)
        n = a_s + b
        rs = 1.0 / np.sqrt((n * n).mean(-1) + dtype(1e-5))                                # [U][S]
        g, beta = w(name + "_norm.weight"), w(name + "_norm.bias")
        a = "multihead_attn_" + name
        wi, bi = w(a + ".in_proj_weight"), w(a + ".in_proj_bias")
        wq, wk, wv, bq, bv = wi[:D], wi[D:2 * D], wi[2 * D:], bi[:D], bi[2 * D:]
        wo, bo, fj = w(a + ".out_proj.weight"), w(a + ".out_proj.bias"), fuser[:, D * j:D * (j + 1)]
        ka_of = lambda z: scale * (((z * g) @ wk.T) @ wq)                                  # A z,  A = scale Wq^T Wk diag(g)
        c_of = lambda z: scale * (((z * g) @ wk.T) @ bq)                                   # c . z
        va_of = lambda z: (((z * g) @ wv.T) @ wo.T) @ fj.T                                 # VV z, VV = Wf_j Wo Wv diag(g)
        KA, VA, Ab, VVb = ka_of(a_s), va_of(a_s), ka_of(b), va_of(b)
        cbk = rs * (c_of(a_s) + c_of(b))
        if masks.get(name) is not None:
            cbk = np.where(np.asarray(masks[name], dtype=bool), dtype(-np.inf), cbk)
        if long_mem and "k" in round_ops:
            KA = _f16(KA)
        if long_mem and "v" in round_ops:
            VA = _f16(VA)
        cq = q_in @ Ab                                                                     # [Be][L]
        qs = q16 if long_mem else q_in
        pr = np.empty(x.shape[:2] + (S,), dtype)
        for u, rows in _groups(None if row_map is None else row_map[j], Be):
            sc = rs[u] * (qs[rows] @ KA[u].T + cq[rows][..., None]) + cbk[u]
            if long_mem and "p" in round_ops:
                O, wsum, pr[rows] = _online_f16(sc, rs[u], VA[u], dtype)
            else:
                pr[rows] = _softmax(sc)
                pp = pr[rows] * rs[u]
                O, wsum = pp @ VA[u], pp.sum(-1)
            update[rows] += O + wsum[..., None] * VVb
        update += fj @ (wo @ (wv @ beta + bv) + bo)
        probs.append(pr)
    return update, probs


def row_errors(d, ex):
    """(e [rows], E, rms): e_r = |d_r - ex_r|_2 / rms_r |ex_r|_2 and E = |d - ex|_F / |ex|_F over the rows where ex is finite (rms over
    those rows; the others get e_r = NaN)."""
    d = np.asarray(d, dtype=np.float64).reshape(-1, D)
    ex = np.asarray(ex, dtype=np.float64).reshape(-1, D)
    ok = np.isfinite(ex).all(-1)
    rms = float(np.sqrt((ex[ok] ** 2).sum(-1).mean()))
    e = np.full(ex.shape[0], np.nan)
    e[ok] = np.sqrt(((d[ok] - ex[ok]) ** 2).sum(-1)) / rms
    return e, float(np.linalg.norm(d[ok] - ex[ok]) / np.linalg.norm(ex[ok])), rms


# ---- the cases of tests/test_gpu_xattn_block.py (their premises are checked on the CPU by tests/test_xattn_ref_host.py) -------------------
# S = (spkemb, alsn, tlsn, apb, lsnemb) as in oracle.inputs.make_cfg_batch; the effective batch is the 7 guidance chunks of B utterances.
T_STEP = 417
LAYERS = (1, 8)
CASES = {
    "one_long":       dict(B=2, L=18, S=(6, 130, 6, 8, 1), pad=(2, 5, 1, 0, 0), seed=1101),
    "threshold":      dict(B=2, L=36, S=(24, 97, 24, 8, 1), pad=(3, 0, 2, 0, 0), seed=1102),
    "threshold_96":   dict(B=2, L=36, S=(24, 96, 24, 8, 1), pad=(3, 0, 2, 0, 0), seed=1102),
    "two_long_mixed": dict(B=2, L=36, S=(70, 257, 130, 33, 1), pad=(5, 9, 0, 2, 0), seed=1103),
    "two_tiles":      dict(B=40, L=16, S=(6, 130, 6, 8, 1), pad=(2, 5, 1, 0, 0), seed=1104),
    "four_tiles":     dict(B=40, L=24, S=(6, 130, 6, 8, 1), pad=(2, 5, 1, 0, 0), seed=1105),
    "concentrated":   dict(B=2, L=36, S=(70, 257, 130, 33, 1), pad=(5, 9, 0, 2, 0), seed=1112),
    "dead_memory":    dict(B=2, L=18, S=(6, 130, 6, 8, 1), pad=(2, 5, 1, 0, 0), seed=1107),
}
CONCENTRATED_QK, CONCENTRATED_V = 5.0, 16.0      # factors on the q | k and the v rows of the cross-attention in-projections of LAYERS


def make_case(name, B=None):
    """dict(sample [7B][L][128], unique five [B + 1][S_j][512], umasks name -> bool [B + 1][S_j] | None, row_map five int32 [7B],
    memories / masks: the same per row, as the oracle takes them)."""
    from oracle import inputs
    c = CASES[name]
    B = c["B"] if B is None else B
    cb = inputs.make_cfg_batch(seed=c["seed"], B=B, L=c["L"], S=c["S"], pad_tail=c["pad"])
    umasks = {}
    for j, n in enumerate(MEM_NAMES):
        mk, rm = cb["masks"][n], cb["row_map"][j]
        umasks[n] = None if mk is None else np.stack([mk[np.nonzero(rm == u)[0][0]] for u in range(B + 1)])
    if name == "dead_memory":      # the conditional audio memory of utterance 0: every key masked
        umasks["alsn"][1, :] = True
    return dict(sample=np.concatenate([cb["init"]] * 7), unique=cb["unique"], umasks=umasks, row_map=cb["row_map"],
                memories=[u[rm] for u, rm in zip(cb["unique"], cb["row_map"])],
                masks={n: (None if umasks[n] is None else umasks[n][cb["row_map"][j]]) for j, n in enumerate(MEM_NAMES)})


def case_state_dict(name):
    from tests.helpers import state_dict
    sd = state_dict()
    if name != "concentrated":
        return sd
    sd = {k: v.copy() for k, v in sd.items()}
    for l in LAYERS:
        for n in MEM_NAMES:
            for part in ("weight", "bias"):
                a = sd[f"decoder.layers.{l}.multihead_attn_{n}.in_proj_{part}"]
                a[:2 * D] *= np.float32(CONCENTRATED_QK)
                a[2 * D:] *= np.float32(CONCENTRATED_V)
    return sd
