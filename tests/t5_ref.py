"""float64 numpy restatement of the T5 v1.0 encoder (transformers T5EncoderModel, feed_forward_proj "relu") and of the reference's
projection (t5.py:48-49, 57), on a state dict keyed like ``T5EncoderModel.state_dict()`` plus ``projection.1.*``:

    x   = embed[ids]                                   (no scaling, no absolute positions)
    h   = x + O_l(Attn(Q_l n, K_l n, V_l n)),          n = rms(x) * g1_l,  rms(x) = x * rsqrt(mean(x^2) + eps)
          scores = q k^T + bias[head][bucket(j - i)] + mask        (no 1 / sqrt(d_kv); masked keys get probability exactly 0)
    x'  = h + Wo_l relu(Wi_l (rms(h) * g2_l))
    out = rms(x_last) * g_final;   text_emb = Linear(relu(out)) + b

``bias`` is block 0's relative_attention_bias, shared by all blocks; padded queries are computed like any other.  Checked against
``T5EncoderModel(...).double()`` in tests/test_t5_host.py; the GPU tests (tests/test_gpu_t5.py) use it as their reference, so they need
no transformers."""
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


def encode(sd, ids, mask, taps=None):
    """ids int [n, T], mask [n, T] (1 = token) -> last hidden state float64 [n, T, 768].  ``taps``: a list that receives the residual
    stream behind every block."""
    w = {k: np.asarray(v, dtype=np.float64) for k, v in sd.items() if k.startswith("encoder.") or k == "shared.weight"}
    ids = np.asarray(ids)
    n, T = ids.shape
    x = w["shared.weight"][ids]
    pos = np.arange(T)
    rel_bucket = bucket(pos[None, :] - pos[:, None])                                                   # [i, j]
    bias = w["encoder.block.0.layer.0.SelfAttention.relative_attention_bias.weight"][rel_bucket]        # [i, j, H]
    bias = bias.transpose(2, 0, 1)[None]                                                               # [1, H, i, j]
    keep = np.asarray(mask).astype(bool)[:, None, None, :]
    for l in range(num_layers_of(sd)):
        p = f"encoder.block.{l}.layer."
        nx = rms(x, w[p + "0.layer_norm.weight"])
        heads = lambda y: y.reshape(n, T, H, DKV).transpose(0, 2, 1, 3)
        q, k, v = (heads(nx @ w[p + f"0.SelfAttention.{m}.weight"].T) for m in "qkv")
        s = q @ k.transpose(0, 1, 3, 2) + bias
        s = np.where(keep, s, -np.inf)
        s = s - s.max(-1, keepdims=True)
        e = np.exp(s)
        pr = e / e.sum(-1, keepdims=True)
        ctx = (pr @ v).transpose(0, 2, 1, 3).reshape(n, T, H * DKV)
        h = x + ctx @ w[p + "0.SelfAttention.o.weight"].T
        nh = rms(h, w[p + "1.layer_norm.weight"])
        x = h + np.maximum(nh @ w[p + "1.DenseReluDense.wi.weight"].T, 0.0) @ w[p + "1.DenseReluDense.wo.weight"].T
        if taps is not None:
            taps.append(x)
    return rms(x, w["encoder.final_layer_norm.weight"])


def project(sd, hidden):
    """the reference's projection: Linear(relu(last_hidden_state))"""
    return np.maximum(hidden, 0.0) @ np.asarray(sd["projection.1.weight"], np.float64).T + np.asarray(sd["projection.1.bias"], np.float64)


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
