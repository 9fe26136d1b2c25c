"""The reference's ``T5TextEncoder`` (convofusion/models/architectures/t5.py:9-109) on the MI355X: token ids to the text memories
``spkemb`` / ``tlsn`` in ONE library call (cfd_t5_encode, csrc/t5_enc.hpp: 5 launches per block + 1, exact float32).

What stays on the host, as in the reference: the tokenizer (``<bos> ... <eos>`` wrapping except for ``'-' * 10``, ``padding=True``,
t5.py:93-96) and ``token2word_map`` (:104-105).  What moves: the T5 v1.0 encoder stack and ``projection`` (ReLU, Linear).  The mirror
holds the same three children -- ``text_model`` (transformers' ``T5EncoderModel``: its parameters, ``from_pretrained`` and the
checkpoint hooks of base.py:83-123 are used, its forward is not), ``tokenizer``, ``projection`` -- so its state-dict keys are the
reference's.

``forward`` encodes only the DISTINCT strings of its argument and gathers rows: the reference calls the encoder on the 7-way replicated
guidance batch (convofusion.py:909-934: 14 B strings, at most 2 B + 1 distinct).  A sequence's rows are the same bits whatever else is in
the batch (t5_enc.hpp), so the gather changes nothing.

Opt-in: ``install(model, fused_text=True)`` swaps ``model.text_audio_encoder.text_encoder`` for a mirror that shares its parameters;
``python -m convofusion_amd.run`` binds the yaml target with ``CFD_RUN_FUSED_TEXT=1``.  Inference only; there is no CPU fallback.
"""
import ctypes as C
import math
import os

import torch
from torch import nn

from . import _lib

D_MODEL, D_KV, NUM_HEADS, D_FF, MAX_LAYERS, MAX_T = 768, 64, 12, 3072, 12, 256
NUM_BUCKETS, MAX_DISTANCE = 32, 128
PLACEHOLDER = "-" * 10      # the reference's "no text" string, tokenised without <bos> / <eos> (t5.py:93)


def block_floats():
    """floats of one block in the packed weights (t5_block_floats, csrc/t5_enc.hpp)"""
    return 2 * D_MODEL + 4 * D_MODEL * D_MODEL + 2 * D_FF * D_MODEL


def pack_floats(vocab, num_layers):
    return vocab * D_MODEL + num_layers * block_floats() + D_MODEL


def _block_keys(l):
    p = f"encoder.block.{l}.layer."
    return [(p + "0.layer_norm.weight", (D_MODEL,)), (p + "0.SelfAttention.q.weight", (D_MODEL, D_MODEL)),
            (p + "0.SelfAttention.k.weight", (D_MODEL, D_MODEL)), (p + "0.SelfAttention.v.weight", (D_MODEL, D_MODEL)),
            (p + "0.SelfAttention.o.weight", (D_MODEL, D_MODEL)), (p + "1.layer_norm.weight", (D_MODEL,)),
            (p + "1.DenseReluDense.wi.weight", (D_FF, D_MODEL)), (p + "1.DenseReluDense.wo.weight", (D_MODEL, D_FF))]


def pack_layout(vocab, num_layers):
    """(state-dict key, shape) in the order of the packed weights: embed | per block g1, Wq, Wk, Wv, Wo, g2, Wi, Wo_ff | g_final
    (csrc/t5_enc.hpp: Wq | Wk | Wv lie behind one another, which makes them the [2304][768] matrix of the q | k | v product)."""
    out = [("shared.weight", (vocab, D_MODEL))]
    for l in range(num_layers):
        out += _block_keys(l)
    return out + [("encoder.final_layer_norm.weight", (D_MODEL,))]


def pack_weights(state, num_layers, device=None):
    """The packed float32 weights of ``state`` (a mapping key -> tensor keyed like ``T5EncoderModel.state_dict()``) on ``device``."""
    vocab = state["shared.weight"].shape[0]
    parts = []
    for key, shape in pack_layout(vocab, num_layers):
        t = state[key]
        if tuple(t.shape) != shape:
            raise ValueError(f"{key} is {tuple(t.shape)}, the HIP encoder needs {shape}")
        parts.append(t.detach().to(device=device, dtype=torch.float32).reshape(-1))
    pack = torch.cat(parts)
    assert pack.numel() == pack_floats(vocab, num_layers)
    return pack


def unpack_weights(pack, vocab, num_layers):
    """The inverse of ``pack_weights``: key -> view of ``pack``."""
    if pack.numel() != pack_floats(vocab, num_layers):
        raise ValueError(f"pack holds {pack.numel()} floats, the layout of vocab {vocab} and {num_layers} blocks {pack_floats(vocab, num_layers)}")
    out, off = {}, 0
    for key, shape in pack_layout(vocab, num_layers):
        n = math.prod(shape)
        out[key] = pack[off:off + n].view(shape)
        off += n
    return out


def relative_bucket(rel):
    """The bidirectional T5 bucket of integer relative positions ``rel = key - query`` (int64 tensor), 32 buckets, max distance 128:
    the operations of ``T5Attention._relative_position_bucket`` in torch's float32, so that bucket edges agree with transformers."""
    nb = NUM_BUCKETS // 2
    out = (rel > 0).to(torch.long) * nb
    a = torch.abs(rel)
    max_exact = nb // 2
    large = max_exact + (torch.log(a.float() / max_exact) / math.log(MAX_DISTANCE / max_exact) * (nb - max_exact)).to(torch.long)
    large = torch.min(large, torch.full_like(large, nb - 1))
    return out + torch.where(a < max_exact, a, large)


def rel_bias_table(weight, T):
    """cfd_t5_args.rel_bias: float32 [heads][2 T - 1], entry [h][d + T - 1] = relative_attention_bias[bucket(d)][h]."""
    d = torch.arange(-(T - 1), T, dtype=torch.long)
    return weight.detach().to(torch.float32)[relative_bucket(d).to(weight.device)].t().contiguous()


def unique_index(texts):
    """(distinct strings in order of first appearance, for every string its position among them)"""
    pos, uniq, index = {}, [], []
    for t in texts:
        if t not in pos:
            pos[t] = len(uniq)
            uniq.append(t)
        index.append(pos[t])
    return uniq, index


def check_config(cfg):
    """The five integers and eps of a configuration the HIP encoder runs; ValueError for anything else."""
    gated = bool(getattr(cfg, "is_gated_act", False)) or getattr(cfg, "feed_forward_proj", "relu") != "relu"
    if gated:
        raise ValueError("the HIP T5 encoder implements T5 v1.0 (feed_forward_proj='relu'), not %r" % getattr(cfg, "feed_forward_proj", "gated"))
    got = (cfg.d_model, cfg.d_kv, cfg.num_heads, cfg.d_ff)
    if got != (D_MODEL, D_KV, NUM_HEADS, D_FF) or not 1 <= cfg.num_layers <= MAX_LAYERS:
        raise ValueError(f"the HIP T5 encoder implements t5-base dimensions (768, 64, 12, 3072) with 1 - {MAX_LAYERS} layers; got {got}, "
                         f"{cfg.num_layers} layers")
    if (getattr(cfg, "relative_attention_num_buckets", NUM_BUCKETS), getattr(cfg, "relative_attention_max_distance", MAX_DISTANCE)) != \
            (NUM_BUCKETS, MAX_DISTANCE):
        raise ValueError("the HIP T5 encoder implements 32 relative-position buckets with max distance 128")
    return int(cfg.num_layers), float(getattr(cfg, "layer_norm_epsilon", 1e-6))


def check_ids(ids, mask, vocab):
    """Host checks of an (ids, mask) pair: shapes, T <= 256, every id in [0, vocab), at least one token per sequence."""
    if ids.dim() != 2 or tuple(mask.shape) != tuple(ids.shape) or ids.shape[0] < 1 or ids.shape[1] < 1:
        raise ValueError(f"ids / mask must be [n_seq >= 1, T >= 1] and alike, got {tuple(ids.shape)} / {tuple(mask.shape)}")
    if ids.shape[1] > MAX_T:
        raise ValueError(f"the HIP T5 encoder takes up to {MAX_T} tokens per sequence, got {ids.shape[1]}")
    lo, hi = int(ids.min()), int(ids.max())
    if lo < 0 or hi >= vocab:
        raise ValueError(f"token ids must lie in [0, {vocab}), got {lo} .. {hi}")
    if not bool((mask != 0).any(dim=1).all()):
        raise ValueError("every sequence needs at least one token (a row of the mask is all 0)")


REL_BIAS_KEY = "encoder.block.0.layer.0.SelfAttention.relative_attention_bias.weight"


def _drop_pack(module, incompatible_keys):
    """load_state_dict post hook of the mirror: the parameters changed, the packed copy is stale"""
    module.repack()


class T5TextEncoder(nn.Module):
    """Mirror of the reference's ``T5TextEncoder``: same constructor signature, same state-dict keys, same return values."""

    def __init__(self, modelpath: str, finetune: bool = False, last_hidden_state: bool = False, latent_dim: list = [1, 256], **kwargs) -> None:
        super().__init__()
        from transformers import AutoTokenizer, T5EncoderModel, logging
        logging.set_verbosity_error()
        os.environ["TOKENIZERS_PARALLELISM"] = "false"
        self.latent_dim = latent_dim
        self.text_max_length = 200
        self.tokenizer = AutoTokenizer.from_pretrained(modelpath, model_max_length=self.text_max_length, use_fast=True)
        self.tokenizer.add_special_tokens({"eos_token": "<eos>", "bos_token": "<bos>", "pad_token": "<pad>", "unk_token": "<unk>"})
        self.text_model = T5EncoderModel.from_pretrained(modelpath)
        if not finetune:
            self.text_model.training = False
            for p in self.text_model.parameters():
                p.requires_grad = False
        self.text_encoded_dim = self.latent_dim
        self.projection = nn.Sequential(nn.ReLU(), nn.Linear(self.text_model.config.hidden_size, self.latent_dim))
        self._init_engine()

    @classmethod
    def from_parts(cls, text_model, tokenizer, projection):
        """Wrap existing objects (no ``from_pretrained``): ``text_model`` a module with ``T5EncoderModel``'s parameter names and a
        ``config``, ``tokenizer`` a callable like transformers', ``projection`` the ``Sequential(ReLU, Linear)``.  Parameters are shared."""
        self = cls.__new__(cls)
        nn.Module.__init__(self)
        self.text_max_length = 200
        self.tokenizer = tokenizer
        self.text_model = text_model
        self.projection = projection
        self.latent_dim = self.text_encoded_dim = projection[1].out_features
        self._init_engine()
        return self

    def _init_engine(self):
        self._pack = None            # (key, packed weights, {T: rel_bias})
        self.last_call = None        # what the last forward / encode_ids did: n_texts, n_encoded, T, launches
        self.register_load_state_dict_post_hook(_drop_pack)      # (a module-level function: the module stays picklable)

    def __getstate__(self):
        state = dict(self.__dict__)
        state["_pack"] = None        # the device copy is rebuilt on the first call after loading
        return state

    def repack(self):
        """Forget the packed device weights: the next call packs the parameters as they are then."""
        self._pack = None

    def _device(self):
        return next(self.text_model.parameters()).device

    def _packed(self):
        """The packed weights, made once per (device, parameter storage, parameter version)."""
        state = dict(self.text_model.state_dict(keep_vars=True))
        num_layers, _ = check_config(self.text_model.config)
        names = [k for k, _ in pack_layout(1, num_layers)] + [REL_BIAS_KEY]      # (the per-T bias tables live and die with the pack)
        key = (str(self._device()),) + tuple((state[k].data_ptr(), state[k]._version) for k in names)
        if self._pack is None or self._pack[0] != key:
            self._pack = (key, pack_weights(state, num_layers, self._device()), {})
        return self._pack

    def _rel_bias(self, T):
        _, _, tables = self._packed()
        if T not in tables:
            w = self.text_model.state_dict(keep_vars=True)[REL_BIAS_KEY]
            tables[T] = rel_bias_table(w.cpu(), T).to(self._device())       # (bucket edges on the host's float32 log, as transformers on CPU)
        return tables[T]

    def encode_ids(self, ids, mask, project=True):
        """ids [n_seq, T] integer, mask [n_seq, T] (nonzero = token) -> float32 [n_seq, T, latent_dim], or the last hidden state
        [n_seq, T, 768] with ``project=False``."""
        if self.training:
            raise NotImplementedError("the HIP T5TextEncoder is inference-only (call .eval())")
        dev = self._device()
        if dev.type != "cuda":
            raise RuntimeError("convofusion_amd.text runs on an MI355X only (move the module to 'cuda'); no CPU fallback")
        num_layers, eps = check_config(self.text_model.config)
        _, pack, _ = self._packed()
        vocab = (pack.numel() - num_layers * block_floats() - D_MODEL) // D_MODEL
        check_ids(ids, mask, vocab)
        n_seq, T = ids.shape
        ids_d = ids.to(device=dev, dtype=torch.int32).contiguous()
        mask_d = (mask != 0).to(device=dev, dtype=torch.uint8).contiguous()
        bias = self._rel_bias(T)
        a = _lib.T5Args()
        a.wpack, a.vocab = pack.data_ptr(), vocab
        a.d_model, a.d_kv, a.num_heads, a.d_ff, a.num_layers, a.gated_act, a.eps = D_MODEL, D_KV, NUM_HEADS, D_FF, num_layers, 0, eps
        a.n_seq, a.T, a.ids, a.mask, a.rel_bias = n_seq, T, ids_d.data_ptr(), mask_d.data_ptr(), bias.data_ptr()
        width = D_MODEL
        if project:
            lin = self.projection[1]
            w = lin.weight.detach().to(device=dev, dtype=torch.float32).contiguous()
            b = lin.bias.detach().to(device=dev, dtype=torch.float32).contiguous()
            a.proj_w, a.proj_b, a.proj_dim = w.data_ptr(), b.data_ptr(), w.shape[0]
            width = w.shape[0]
        out = torch.empty(n_seq, T, width, device=dev, dtype=torch.float32)
        from .conditioning import _engine_handle
        with torch.cuda.device(dev):
            stream = torch.cuda.current_stream(dev).cuda_stream
            _lib.check(_lib.load().cfd_t5_encode(_engine_handle(dev), C.byref(a), C.c_void_p(out.data_ptr()), C.c_void_p(stream)))
        self.last_call = {"n_texts": n_seq, "n_encoded": n_seq, "T": T, "launches": 5 * num_layers + 1}
        return out

    def token_to_word_list(self, texts, token2word_map):
        """t5.py:77-86"""
        out = []
        for idx, txt in enumerate(texts):
            words = txt.split()
            out.append([words[j] if j is not None else "" for j in token2word_map[idx]])
        return out

    def get_last_hidden_state(self, texts, return_map: bool = False, project=False):
        """t5.py:88-109 on the distinct strings: (hidden [len(texts), T, 768 or latent_dim], bool mask [len(texts), T], word map or None)"""
        texts = [f"<bos> {text} <eos>" if text != PLACEHOLDER else text for text in texts]
        uniq, index = unique_index(texts)
        enc = self.tokenizer(uniq, return_tensors="pt", padding=True)
        hidden = self.encode_ids(enc.input_ids, enc.attention_mask, project=project)
        gather = torch.tensor(index, device=hidden.device, dtype=torch.long)
        self.last_call.update(n_texts=len(texts))
        mask = enc.attention_mask.to(device=hidden.device, dtype=bool).index_select(0, gather)
        word_map = None
        if return_map:
            word_map = self.token_to_word_list(texts, [enc.word_ids(i) for i in index])
        return hidden.index_select(0, gather), mask, word_map

    def forward(self, texts, return_map: bool = False):
        """(text_emb [len(texts), T, latent_dim], bool mask [len(texts), T], token2word_map or None), as t5.py:51-59."""
        return self.get_last_hidden_state(texts, return_map=return_map, project=True)


def install(model, fused_text=False):
    """``fused_text=True``: swap ``model.text_audio_encoder.text_encoder`` (the reference's ``T5TextEncoder``) for a mirror that SHARES its
    ``text_model``, ``tokenizer`` and ``projection``; the original is kept as ``model._cfd_text_encoder`` (outside the module tree) and ``uninstall`` puts it back.
    ``False`` (the default) changes nothing.  Returns the model."""
    if not fused_text:
        return model
    holder = model.text_audio_encoder
    old = holder.text_encoder
    if isinstance(old, T5TextEncoder):
        return model
    new = T5TextEncoder.from_parts(old.text_model, old.tokenizer, old.projection)
    new.train(getattr(old, "training", False))
    # kept in the instance dict directly: ``model._cfd_text_encoder = old`` on an nn.Module would REGISTER the old encoder as a child --
    # duplicate state-dict keys, a strict load_state_dict that misses them, and nothing in vars(model) for uninstall to find
    model.__dict__["_cfd_text_encoder"] = old
    holder.text_encoder = new
    return model


def uninstall(model):
    """Put the encoder ``install(model, fused_text=True)`` replaced back.  Returns the model."""
    old = model.__dict__.pop("_cfd_text_encoder", None)
    if old is not None:
        model.text_audio_encoder.text_encoder = old
    return model
