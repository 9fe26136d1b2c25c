"""float64 numpy restatement of the T5 v1.0 encoder (transformers T5EncoderModel, feed_forward_proj "relu") and of the reference's
projection (t5.py:48-49, 57), on a state dict keyed like ``T5EncoderModel.state_dict()`` plus ``projection.1.*``:

    x   = embed[ids]                                   (no scaling, no absolute positions)
    h   = x + O_l(Attn(Q_l n, K_l n, V_l n)),          n = rms(x) * g1_l,  rms(x) = x * rsqrt(mean(x^2) + eps)
          scores = q k^T + bias[head][bucket(j - i)] + mask        (no 1 / sqrt(d_kv); masked keys get probability exactly 0)
    x'  = h + Wo_l relu(Wi_l (rms(h) * g2_l))
    out = rms(x_last) * g_final;   text_emb = Linear(relu(out)) + b

``bias`` is block 0's relative_attention_bias, shared by all blocks; padded queries are computed like any other.  Checked against
``T5EncoderModel(...).double()`` in tests/test_t5_host.py; the GPU tests (tests/test_gpu_t5.py) use it as their reference, so they need
no transformers.  ``encode`` / ``project`` are the composition of one function per launch of the HIP call (``stage_*``), which
tests/test_gpu_t5_stages.py applies to the device's own intermediates."""
import numpy as np

D, DKV, H, FF, EPS = 768, 64, 12, 3072, 1e-6
NUM_BUCKETS, MAX_DISTANCE = 32, 128


def bucket(rel):
    """T5Attention._relative_position_bucket, bidirectional, for integer relative positions ``rel = j - i`` (key minus query).  The large
    buckets go through float32 log / division like torch's (the edges are where a float64 path could differ)."""
    rel = np.asarray(rel, dtype=np.int64)
    nb = NUM_BUCKETS // 2
    out = (rel > 0).astype(np.int64) * nb
    a = np.abs(rel)
    max_exact = nb // 2
    small = a < max_exact
    af = np.maximum(a, 1).astype(np.float32)
    big = np.log(af / np.float32(max_exact)) / np.float32(np.log(MAX_DISTANCE / max_exact)) * np.float32(nb - max_exact)
    big = max_exact + big.astype(np.int64)
    big = np.minimum(big, nb - 1)
    return out + np.where(small, a, big)


def rms(x, g, eps=EPS):
    return x / np.sqrt((x * x).mean(-1, keepdims=True) + eps) * g


def num_layers_of(sd):
    n = 0
    while f"encoder.block.{n}.layer.0.layer_norm.weight" in sd:
        n += 1
    return n


def _w(sd, key, dtype):
    return np.asarray(sd[key], dtype=dtype)


def _block(l):
    return f"encoder.block.{l}.layer."


REL_BIAS = "encoder.block.0.layer.0.SelfAttention.relative_attention_bias.weight"


# One stage each, what one launch of cfd_t5_encode computes (csrc/t5_enc.hpp), in ``dtype`` throughout (float64, or float32 for what the
# formula itself loses in single precision): inputs and weights are cast to it, rows are [..., width] with any leading shape.

def stage_qkv(sd, l, x, dtype=np.float64):
    """x [..., 768] -> q | k | v [..., 2304] = (rms(x) g1) Wq^T | Wk^T | Wv^T of block l"""
    p = _block(l)
    nx = rms(np.asarray(x, dtype=dtype), _w(sd, p + "0.layer_norm.weight", dtype))
    return np.concatenate([nx @ _w(sd, p + f"0.SelfAttention.{m}.weight", dtype).T for m in "qkv"], axis=-1)


def stage_attn(sd, qkv, mask, T, dtype=np.float64):
    """q | k | v [n * T rows, 2304] and mask [n, T] (nonzero = key kept; any pattern) -> ctx [n, T, 768]: per head
    softmax_j(q_i k_j + bias[head][bucket(j - i)]) v_j over the kept keys j, for every query i (padded ones included).  A sequence without
    any key gives NaN rows."""
    keep = np.asarray(mask).astype(bool).reshape(-1, T)
    n = keep.shape[0]
    qkv = np.asarray(qkv, dtype=dtype).reshape(n, T, 3, H, DKV)
    q, k, v = (qkv[:, :, m].transpose(0, 2, 1, 3) for m in range(3))                                   # [n, H, T, DKV]
    pos = np.arange(T)
    bias = _w(sd, REL_BIAS, dtype)[bucket(pos[None, :] - pos[:, None])]                                # [i, j, H]
    bias = bias.transpose(2, 0, 1)[None]                                                               # [1, H, i, j]
    s = q @ k.transpose(0, 1, 3, 2) + bias
    with np.errstate(invalid="ignore"):                                                               # (-inf) - (-inf): a sequence without keys
        s = np.where(keep[:, None, None, :], s, -np.inf)
        s = s - s.max(-1, keepdims=True)
        e = np.exp(s)
        pr = e / e.sum(-1, keepdims=True)
        return (pr @ v).transpose(0, 2, 1, 3).reshape(n, T, H * DKV)


def stage_attn_out(sd, l, x, ctx, dtype=np.float64):
    """h = x + ctx Wo^T of block l"""
    return np.asarray(x, dtype=dtype) + np.asarray(ctx, dtype=dtype) @ _w(sd, _block(l) + "0.SelfAttention.o.weight", dtype).T


def stage_ff_in(sd, l, h, dtype=np.float64):
    """f = relu((rms(h) g2) Wi^T) of block l"""
    p = _block(l)
    nh = rms(np.asarray(h, dtype=dtype), _w(sd, p + "1.layer_norm.weight", dtype))
    return np.maximum(nh @ _w(sd, p + "1.DenseReluDense.wi.weight", dtype).T, dtype(0.0))


def stage_ff_out(sd, l, h, f, dtype=np.float64):
    """x' = h + f Wo_ff^T of block l"""
    return np.asarray(h, dtype=dtype) + np.asarray(f, dtype=dtype) @ _w(sd, _block(l) + "1.DenseReluDense.wo.weight", dtype).T


def _project(sd, hidden, dtype):
    return np.maximum(np.asarray(hidden, dtype=dtype), dtype(0.0)) @ _w(sd, "projection.1.weight", dtype).T + _w(sd, "projection.1.bias", dtype)


def stage_final(sd, x, project, dtype=np.float64):
    """the last hidden state rms(x) g_final, or with ``project`` the reference's Linear(relu(.)) of it"""
    hidden = rms(np.asarray(x, dtype=dtype), _w(sd, "encoder.final_layer_norm.weight", dtype))
    return _project(sd, hidden, dtype) if project else hidden


def encode(sd, ids, mask, taps=None):
    """ids int [n, T], mask [n, T] (1 = token) -> last hidden state float64 [n, T, 768].  ``taps``: a list that receives the residual
    stream behind every block.  The composition of the stages above in float64."""
    ids = np.asarray(ids)
    n, T = ids.shape
    x = _w(sd, "shared.weight", np.float64)[ids]
    for l in range(num_layers_of(sd)):
        ctx = stage_attn(sd, stage_qkv(sd, l, x), mask, T)
        h = stage_attn_out(sd, l, x, ctx)
        x = stage_ff_out(sd, l, h, stage_ff_in(sd, l, h))
        if taps is not None:
            taps.append(x)
    return stage_final(sd, x, project=False)


def project(sd, hidden):
    """the reference's projection: Linear(relu(last_hidden_state))"""
    return _project(sd, hidden, np.float64)


def make_state(num_layers, seed, vocab=64, proj_dim=512):
    """A seeded state dict (float32 arrays) from numpy.random.RandomState -- the same values on every machine --: transformers' init
    scales, every block different, norm gains 1 + 0.1 randn, relative_attention_bias with std 1 (a wrong bucket then shows far above any
    tolerance)."""
    r = np.random.RandomState(seed)
    f = lambda *shape, std=1.0: (r.randn(*shape) * std).astype(np.float32)
    sd = {"shared.weight": f(vocab, D)}
    sd["encoder.embed_tokens.weight"] = sd["shared.weight"]
    for l in range(num_layers):
        p = f"encoder.block.{l}.layer."
        sd[p + "0.SelfAttention.q.weight"] = f(H * DKV, D, std=(D * DKV) ** -0.5)
        sd[p + "0.SelfAttention.k.weight"] = f(H * DKV, D, std=D ** -0.5)
        sd[p + "0.SelfAttention.v.weight"] = f(H * DKV, D, std=D ** -0.5)
        sd[p + "0.SelfAttention.o.weight"] = f(D, H * DKV, std=(H * DKV) ** -0.5)
        if l == 0:
            sd[p + "0.SelfAttention.relative_attention_bias.weight"] = f(NUM_BUCKETS, H)
        sd[p + "0.layer_norm.weight"] = (1.0 + 0.1 * r.randn(D)).astype(np.float32)
        sd[p + "1.DenseReluDense.wi.weight"] = f(FF, D, std=D ** -0.5)
        sd[p + "1.DenseReluDense.wo.weight"] = f(D, FF, std=FF ** -0.5)
        sd[p + "1.layer_norm.weight"] = (1.0 + 0.1 * r.randn(D)).astype(np.float32)
    sd["encoder.final_layer_norm.weight"] = (1.0 + 0.1 * r.randn(D)).astype(np.float32)
    sd["projection.1.weight"] = f(proj_dim, D, std=D ** -0.5)
    sd["projection.1.bias"] = f(proj_dim, std=0.1)
    return sd


# The cases of tests/golden/t5_enc.npz and tests/test_gpu_t5.py: name -> (num_layers, state seed, sequence lengths, padded length T)
# D: 65 sequences of up to 32 tokens = 2080 token rows in one block: the shape at which the q | k | v and Wi products run as 128 x 128 blocks
# on a 256-CU device (the others run every product as 64 x 64 blocks)
_D_LENS = (32,) + tuple(int(v) for v in np.random.RandomState(7).randint(1, 33, size=64))
CASES = {"A": (2, 11, (1, 2, 17, 33, 40), 40), "B": (1, 12, (200,), 200), "C": (1, 13, (1,), 1), "D": (1, 14, _D_LENS, 32)}
VOCAB = 64
# what the fixture stores of a case's float32 output: every (sequence stride, position stride)-th row (all of A and C)
STORED = {"A": (1, 1), "B": (1, 8), "C": (1, 1), "D": (8, 4)}


def case_inputs(name):
    """ids int32 [n, T] (seeded; padding positions hold id 0 like <pad>) and mask uint8 [n, T]"""
    _, seed, lens, T = CASES[name]
    r = np.random.RandomState(1000 + seed)
    ids = np.zeros((len(lens), T), np.int32)
    mask = np.zeros((len(lens), T), np.uint8)
    for s, n in enumerate(lens):
        ids[s, :n] = r.randint(1, VOCAB, size=n)
        mask[s, :n] = 1
    return ids, mask


def hole_masks(T=129):
    """uint8 [3, T], masks that are no prefix: keys 0 .. 63 masked (the first kept key lies in the second 64-key tile), keys 64 .. 127
    masked (a whole inner tile), every second key masked (keys 1, 3, 5, ... out)."""
    mask = np.ones((3, T), np.uint8)
    mask[0, :64] = 0
    mask[1, 64:128] = 0
    mask[2, 1::2] = 0
    return mask


# The end-to-end cases of tests/golden/t5_edges.npz and tests/test_gpu_t5_edges.py: name -> (num_layers, state seed, lengths or None for
# hole_masks, T).  L12: t5-base's depth; T256: the longest sequence the call takes, next to one whose last 64-key tile holds one key;
# H: the hole masks at T = 129
EDGE_CASES = {"L12": (12, 21, (9, 4), 9), "T256": (1, 22, (256, 193), 256), "H": (1, 23, None, 129)}
# what the fixture stores of an edge case's float32 projected output: every (position stride)-th row
EDGE_STORED = {"L12": 1, "T256": 16, "H": 8}


def prefix_inputs(seed, lens, T):
    """ids int32 [n, T] drawn from RandomState(seed) (padding holds id 0) and the prefix mask uint8 [n, T] of ``lens``"""
    r = np.random.RandomState(seed)
    ids = np.zeros((len(lens), T), np.int32)
    mask = np.zeros((len(lens), T), np.uint8)
    for s, n in enumerate(lens):
        ids[s, :n] = r.randint(1, VOCAB, size=n)
        mask[s, :n] = 1
    return ids, mask


def hole_inputs(seed, T=129):
    """ids int32 [3, T] with a token at EVERY position (a masked key carries values that must leave no trace) and hole_masks(T)"""
    return np.random.RandomState(seed).randint(1, VOCAB, size=(3, T)).astype(np.int32), hole_masks(T)


def edge_inputs(name):
    _, seed, lens, T = EDGE_CASES[name]
    return hole_inputs(2000 + seed, T) if lens is None else prefix_inputs(2000 + seed, lens, T)


def rel_err(got, want):
    """the GPU tests' measure: max-abs distance over the reference's RMS, every position counted"""
    want = np.asarray(want, np.float64)
    return float(np.abs(np.asarray(got, np.float64) - want).max() / np.sqrt((want * want).mean()))


def keep_norm_dtype(model):
    """transformers' T5LayerNorm squares ``hidden_states.to(torch.float32)`` whatever the module's dtype, so ``model.double()`` alone is not
    a float64 forward (it agrees with one to 5e-7 only).  This rebinds the norms' forward ON THE GIVEN INSTANCE to the same formula in
    the input's own dtype; with it ``.double()`` is float64 throughout.  A float32 module computes the same with or without it."""
    import types
    import torch

    def forward(self, hidden_states):
        variance = hidden_states.pow(2).mean(-1, keepdim=True)
        return self.weight * (hidden_states * torch.rsqrt(variance + self.variance_epsilon))
    for mod in model.modules():
        if type(mod).__name__ == "T5LayerNorm":
            mod.forward = types.MethodType(forward, mod)
    return model


def stub_text_model(sd):
    """A torch module with T5EncoderModel's parameter names (the encoder keys of ``sd``, ``shared`` and ``embed_tokens`` tied) and a
    ``config`` -- what ``convofusion_amd.text.T5TextEncoder.from_parts`` needs of ``text_model``, without transformers."""
    from types import SimpleNamespace
    import torch
    from torch import nn
    root = nn.Module()
    params = {}
    for key, value in sd.items():
        if key.startswith("projection."):
            continue
        if id(value) not in params:
            params[id(value)] = nn.Parameter(torch.from_numpy(np.array(value)), requires_grad=False)
        *path, leaf = key.split(".")
        mod = root
        for part in path:
            if part not in mod._modules:
                mod.add_module(part, nn.Module())
            mod = mod._modules[part]
        mod.register_parameter(leaf, params[id(value)])
    root.config = SimpleNamespace(d_model=D, d_kv=DKV, num_heads=H, d_ff=FF, num_layers=num_layers_of(sd), vocab_size=sd["shared.weight"].shape[0],
                                  layer_norm_epsilon=EPS, feed_forward_proj="relu", is_gated_act=False,
                                  relative_attention_num_buckets=NUM_BUCKETS, relative_attention_max_distance=MAX_DISTANCE)
    return root


def projection_module(sd):
    """the reference's ``Sequential(ReLU, Linear)`` holding ``sd``'s projection"""
    import torch
    from torch import nn
    w = sd["projection.1.weight"]
    proj = nn.Sequential(nn.ReLU(), nn.Linear(w.shape[1], w.shape[0]))
    proj.load_state_dict({"1.weight": torch.from_numpy(np.array(w)), "1.bias": torch.from_numpy(np.array(sd["projection.1.bias"]))}, strict=True)
    return proj
