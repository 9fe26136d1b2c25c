"""The self-attention block of one decoder layer (cross_attention.py:568-572) in plain numpy -- the yardstick of
tests/test_gpu_selfattn_block.py, checked on the CPU by tests/test_selfattn_ref_host.py.  No torch.

  block(sd, layer, x_in, dtype)   (update [Be][L][512], probabilities [Be][4][L][L]): LayerNorm1 of the rows, q | k | v through
                                  self_attn.in_proj_*, 4 heads of 128, q scaled by 1 / sqrt(128), the softmax over the row's L keys (the block
                                  has no key mask), P.V, out_proj with its bias.  dtype=np.float64 is the reference, dtype=np.float32 the
                                  float32 restatement (weights, input and every operation in float32).
  yardstick32(sd, layer, x_in)    the float32 restatement formed the way the device forms its result: fl32(x_in + block_f32(x_in)) - x_in.
  row_errors(d, ex), worst(e, L)  the measures of tests/test_gpu_xattn_block.py: per query row r = (batch row, token)
                                  e_r = |d_r - ex_r|_2 / rms_r |ex_r|_2, its worst row with the row's index, and E = |d - ex|_F / |ex|_F.
  gate(measure_f32)               5 x the float32 yardstick's measure + 1e-6 (22-bit split-pair operands against float32's 24, and a floor
                                  for rows whose float32 error is small by chance): the cross-attention block's rule.

The emulated faults, each a keyword of `block` (what a subtly wrong kernel would compute; tests/test_selfattn_ref_host.py proves that the
gate separates each from rounding):
  p16, v16, k16   that operand through np.float16 -- a product that lost the low half of one split-pair operand.  P is rounded before
                  normalisation, relative to the row's maximum as the kernels hold it; the sum stays unrounded.
  pad_weight      one extra key, a copy of token L - 1, takes part in the softmax: a padding slot with weight.  (The probabilities
                  returned then have L + 1 columns.)
  key_order       inside the first 32-key block V's keys 4g .. 4g+3 and 16+4g .. 16+4g+3 (g = 0 .. 3) change places while the probabilities
                  stay: the two transposed reads of a V^T fragment exchanged.  L >= 32 only.
  adjacent        V's keys 0 and 1 exchanged.

Two weight sets (weights(name)): "plain" = tests.helpers.state_dict(); "peaked" = the q and k rows of every layer's
self_attn.in_proj_weight and in_proj_bias (the first 1024) times PEAKED_QK, so that one key holds most of a typical row's weight and a
wrong key order cannot hide under near-uniform probabilities.
"""
import functools

import numpy as np

D, NHEAD, HD = 512, 4, 128
T_STEP = 417
LAYERS = (0, 4, 8)
S, PAD = (6, 40, 6, 8, 1), (2, 5, 1, 0, 0)      # the memories of tests/test_gpu_selfattn_token_major.py
WEIGHT_SETS = ("plain", "peaked")
PEAKED_QK = 4.0
FAULTS = ("p16", "v16", "k16", "pad_weight", "key_order", "adjacent")


def _ln(x, w, b):
    xc = x - x.mean(-1, keepdims=True)
    return xc / np.sqrt((xc * xc).mean(-1, keepdims=True) + x.dtype.type(1e-5)) * w + b


def _f16(x):
    return x.astype(np.float16).astype(x.dtype)


def block(sd, layer, x_in, dtype=np.float64, *, p16=False, v16=False, k16=False, pad_weight=False, key_order=False, adjacent=False):
    dtype = np.dtype(dtype).type
    p = f"decoder.layers.{layer}."
    w = lambda key: sd[p + key].astype(dtype)
    x = np.asarray(x_in).astype(dtype)
    Be, L, _ = x.shape
    h = _ln(x, w("norm1.weight"), w("norm1.bias"))
    wi, bi = w("self_attn.in_proj_weight"), w("self_attn.in_proj_bias")
    heads = lambda z: z.reshape(Be, L, NHEAD, HD).transpose(0, 2, 1, 3)                  # [Be][4][token][128]
    q = heads((h @ wi[:D].T + bi[:D]) * dtype(1.0 / np.sqrt(float(HD))))
    k = heads(h @ wi[D:2 * D].T + bi[D:2 * D])
    v = heads(h @ wi[2 * D:].T + bi[2 * D:])
    if k16:
        k = _f16(k)
    if v16:
        v = _f16(v)
    if pad_weight:
        k, v = np.concatenate([k, k[:, :, -1:]], 2), np.concatenate([v, v[:, :, -1:]], 2)
    sc = q @ k.transpose(0, 1, 3, 2)
    e = np.exp(sc - sc.max(-1, keepdims=True))
    pr = (_f16(e) if p16 else e) / e.sum(-1, keepdims=True)
    if key_order:
        assert L >= 32, "key_order needs a whole 32-key block"
        v = v.copy()
        v[:, :, 0:16], v[:, :, 16:32] = v[:, :, 16:32].copy(), v[:, :, 0:16].copy()      # (groups g = 0 .. 3 side by side: the two halves change places)
    if adjacent:
        v = v.copy()
        v[:, :, 0], v[:, :, 1] = v[:, :, 1].copy(), v[:, :, 0].copy()
    o = (pr @ v).transpose(0, 2, 1, 3).reshape(Be, L, D)
    return o @ w("self_attn.out_proj.weight").T + w("self_attn.out_proj.bias"), pr


def yardstick32(sd, layer, x_in):
    x = np.asarray(x_in, dtype=np.float32)
    u32 = block(sd, layer, x, np.float32)[0]
    assert u32.dtype == np.float32
    return (x + u32).astype(np.float64) - x.astype(np.float64)


def row_errors(d, ex):
    """(e [rows], E): e_r = |d_r - ex_r|_2 / rms_r |ex_r|_2 and E = |d - ex|_F / |ex|_F."""
    d = np.asarray(d, dtype=np.float64).reshape(-1, D)
    ex = np.asarray(ex, dtype=np.float64).reshape(-1, D)
    rms = float(np.sqrt((ex ** 2).sum(-1).mean()))
    return np.sqrt(((d - ex) ** 2).sum(-1)) / rms, float(np.linalg.norm(d - ex) / np.linalg.norm(ex))


def worst(e, L):
    """(the worst row's error, its (batch row, token))."""
    r = int(np.argmax(e))
    return float(e[r]), (r // L, r % L)


def measures(d, ex, L):
    """(worst row, (batch row, token), E)."""
    e, E = row_errors(d, ex)
    w, at = worst(e, L)
    return w, at, E


def gate(measure_f32):
    return 5.0 * measure_f32 + 1e-6


@functools.lru_cache(maxsize=None)
def weights(name):
    from tests.helpers import state_dict
    sd = state_dict()
    if name == "plain":
        return sd
    assert name == "peaked", name
    sd = {k: v.copy() for k, v in sd.items()}
    for l in range(9):
        for part in ("weight", "bias"):
            sd[f"decoder.layers.{l}.self_attn.in_proj_{part}"][:2 * D] *= np.float32(PEAKED_QK)
    return sd


def peak_median(pr):
    """The median over (batch row, head, query) of a row's largest probability."""
    return float(np.median(pr.max(-1)))


# ---- the cases of tests/test_gpu_selfattn_block.py ------------------------------------------------------------------------------------------
# path: "tile" = the tile kernels (a handle with the row-tile path off), self_attn_fused_kernel; "tile16" = the tile kernels at L = 16 (the grouped
# q | k + V^T launch and rt_selfattn_kernel at tpr = 1); "rowtile" = the row-tile path (RT_EPI_QKV, rt_selfattn_kernel); "saved" = the row-tile
# gradient engine's saved forward (Denoiser.vjp, the taps "weg.x.<l>.<k>").  Be: batch rows -- on the tile kernels 7 guidance chunks of Be / 7
# utterances, on the row-tile path independent rows.  alone: the case that also runs batch row 0 by itself (rows are independent).
CASES = (
    dict(path="tile", Be=14, L=18, why="one partial key tile, one partial query tile"),
    dict(path="tile", Be=14, L=32, why="whole tiles only: no clamped slot, the mask never bites"),
    dict(path="tile", Be=7, L=64, why="whole tiles only: no clamped slot, the mask never bites"),
    dict(path="tile", Be=14, L=34, why="2 real keys + 30 clamped copies in the last tile", alone=True),
    dict(path="tile", Be=7, L=66, why="three key tiles, both LDS stages reused"),
    dict(path="tile", Be=7, L=128, why="exactly one full query workgroup"),
    dict(path="tile", Be=7, L=130, why="second workgroup with one active wave of 2 queries"),
    dict(path="tile", Be=7, L=196, why="7 key tiles, the last holds 4 keys; second workgroup: 4 whole waves, one of 4 queries, 3 idle"),
    dict(path="tile16", Be=14, L=16, why="the only L with this launch pair", alone=True),
    dict(path="rowtile", Be=1, L=2, why="one key pair; V^T columns >= 16 never written by the epilogue"),
    dict(path="rowtile", Be=3, L=18, why="second token tile with 2 rows, keys 18 .. 31 masked", alone=True),
    dict(path="rowtile", Be=13, L=16, why="13 token tiles: one 16-feature block per workgroup in the out-projection"),
    dict(path="rowtile", Be=14, L=16, why="14 token tiles: two 16-feature blocks per workgroup in the out-projection"),
    dict(path="rowtile", Be=1, L=32, why="the path's limit"),
    dict(path="rowtile", Be=7, L=32, why="the path's limit; 14 tiles at tpr = 2"),
    dict(path="saved", Be=1, L=2, why="as the row-tile case"),
    dict(path="saved", Be=2, L=18, why="as the row-tile case", alone=True),
    dict(path="saved", Be=1, L=32, why="as the row-tile case"),
)


# The host test's input seed per length (default 3000 + L).  L = 2: with the peaked weights most seeds give layer 0 rows whose two
# probabilities are 1 and < 1e-8 in every head -- P's low half then carries nothing and p16 / k16 move nothing, which says nothing about
# the gate; seed 3003 has rows with two live keys in every layer.
HOST_SEEDS = {2: 3003}


def case_id(c):
    return f"{c['path']}-{c['Be']}x{c['L']}"


def cases(*paths):
    return [c for c in CASES if c["path"] in paths]


def host_inputs(L, seed=None):
    """The host test's problem at length L: B = 1 utterance, 7 guidance rows -> dict(sample [7][L][128], memories, masks)."""
    from oracle import inputs
    cb = inputs.make_cfg_batch(seed=HOST_SEEDS.get(L, 3000 + L) if seed is None else seed, B=1, L=L, S=S, pad_tail=PAD)
    return dict(sample=np.concatenate([cb["init"]] * 7), memories=cb["memories"], masks=cb["masks"])


def case_inputs(path, Be, L):
    """dict(sample [Be][L][128], memories five [Be][S_j][512], masks name -> bool [Be][S_j] | None) of a case.  Tile kernels: the 7 guidance
    chunks of Be / 7 utterances.  Row-tile path: independent rows; the 13 rows at L = 16 are the first 13 of the 14."""
    from oracle import inputs
    if path in ("tile", "tile16"):
        assert Be % 7 == 0
        cb = inputs.make_cfg_batch(seed=2000 + L, B=Be // 7, L=L, S=S, pad_tail=PAD)
        return dict(sample=np.concatenate([cb["init"]] * 7), memories=cb["memories"], masks=cb["masks"])
    n = 14 if (L == 16 and Be == 13) else Be
    inp = inputs.make_plain_batch(seed=2500 + 40 * L + n, Be=n, L=L, S=S, pad_tail=PAD)
    return first_rows(inp, Be)


def first_rows(inp, n):
    return dict(sample=inp["sample"][:n].copy(), memories=[m[:n].copy() for m in inp["memories"]],
                masks={k: (None if v is None else v[:n].copy()) for k, v in inp["masks"].items()})


def oracle_taps(sd, inp):
    """name -> [Be][L][512] of oracle.denoiser_ref.denoiser_forward's residual-stream taps: "x0", "l<i>.after_self", "l<i>.out"."""
    from oracle import denoiser_ref
    taps = {}
    denoiser_ref.denoiser_forward(sd, inp["sample"], T_STEP, inp["memories"], inp["masks"], taps=taps)
    return {k: v.transpose(1, 0, 2).copy() for k, v in taps.items() if k == "x0" or k.endswith(".after_self") or k.endswith(".out")}


def block_input(taps, layer):
    return taps["x0"] if layer == 0 else taps[f"l{layer - 1}.out"]
