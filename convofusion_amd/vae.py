"""``ConvoFusionVae`` with the encoder and the decoder on the HIP path.

Drop-in for ``convofusion.models.architectures.vae.ConvoFusionVae`` (reference vae.py:33-372) for generation and evaluation: same
constructor, same 337-entry state-dict layout (so ``motion_vae.*`` of a reference checkpoint loads strictly), ``decode(z, lengths)`` --
the step right after the denoising loop (test.py / unbounded_synthesis.py: latents -> 189 motion features per frame) -- and
``encode(features, lengths)`` -- test.py's evaluation path (convofusion.py:1053-1057 encodes the ground truth and the generated motion).
``forward`` belongs to training and is not provided: it raises (the reference's own forward cannot run either: it unpacks two values
from the three ``encode`` returns).

``decode`` restates vae.py:268-372 for arch 'encoder_decoder' / PE_TYPE 'convofusion' with every arithmetic step in
libcfdenoise float32 kernels (cfd_linear_act, cfd_layer_norm, cfd_mha, cfd_add, cfd_zero_rows); torch only slices,
concatenates and allocates.  Two SkipTransformerDecoders (cross_attention.py:66-125) of pre-norm
TransformerDecoderLayers (:361-382): d_model 128, 2 heads, ff 1024, 5 layers -- tiny next to the loop (a few ms per
batch), so the kernels are plain and exact rather than tuned.

``encode`` restates vae.py:162-266 in ONE launch for both SkipTransformerEncoders (cfd_vae_encode, csrc/vae_enc.hpp): chunking, root
subtraction, skeleton embedding, global tokens, PE, mask, the encoder stacks and the final norm, exact float32.  torch then forms
std = exp(logvar) ** 0.5 and draws ``Normal(mu, std).rsample()`` from the default generator exactly as the reference does.  The
kernel reads a packed copy of the encoder weights that is rebuilt whenever a parameter changes (``load_state_dict``, ``.to``).

``decode`` is differentiable with respect to ``z``: with grad enabled and ``z.requires_grad`` it returns the same launch sequence's output
(bit-identical to the ``no_grad`` result) behind a ``torch.autograd.Function`` whose backward is ``decode_vjp``.  ``decode_vjp(z, lengths,
d_feats)`` is one call of cfd_vae_decode_vjp (csrc/vae_dec.hpp): a forward of both decoder stacks on 16-frame row tiles that saves what the
reverse sweep needs, and the sweep from the cotangent at the 189 features back to the latents -- what the reference gets from torch autograd
over its ``decode``.  Exact float32, no atomics (two calls return the same bits), nframes <= 256, n_chunks <= 16.  It reads a packed copy of
the decoder weights (every matrix in both orders, ``_decoder_pack``) kept by the same cache rule as the encoder's (``_cached_pack``).  No gradients to weights or lengths.

``decode(z, lengths, fused=True)`` (opt-in; the default is the launch sequence above, bit for bit) runs the forward on those same kernels as a
call of its own: without grad one forward-only cfd_vae_decode (12 launches at 5 layers, a workspace of 4 KB per frame row), the bits of
``decode_vjp``'s forward (about 1e-5 from the default path's); with grad the forward is kept in the handle's workspace under a ticket and
the backward is the reverse sweep alone (cfd_vae_decode_sweep) -- or ``decode_vjp`` on the saved z when another decode has used the
workspace since: the same bits either way.
"""
import ctypes as C

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import _lib
from .conditioning import ACT_GELU, ACT_NONE, _engine_handle, linear_act

# The body part of stack s of the latent's first axis: encode's kernel runs the body stack as stack 0 and the hands stack as stack 1
# (csrc/vae_enc.hpp: blockIdx.y, the packed weights' body block first, ``_encoder_sources``), decode reads z[0] with the body decoder.
LATENT_PARTS = ("body", "hands")


def _ptr(t):
    return C.c_void_p(t.data_ptr())


def _stream(t):
    return C.c_void_p(torch.cuda.current_stream(t.device).cuda_stream)


def _lengths_list(lengths, default=None):
    """Frames per sequence as a list of ints, from a list / tuple / tensor; None means ``default``."""
    if lengths is None:
        return default
    return [int(v) for v in (lengths.reshape(-1).tolist() if torch.is_tensor(lengths) else lengths)]


def layer_norm(x, norm):
    """nn.LayerNorm over the last dimension on the device."""
    x = x.contiguous()
    out = torch.empty_like(x)
    D = x.shape[-1]
    w = norm.weight.detach().to(x.device, torch.float32).contiguous()
    b = norm.bias.detach().to(x.device, torch.float32).contiguous()
    with torch.cuda.device(x.device):
        _lib.check(_lib.load().cfd_layer_norm(_engine_handle(x.device), _ptr(x), x.numel() // D, D, _ptr(w), _ptr(b),
                                              C.c_float(norm.eps), _ptr(out), _stream(x)))
    return out


def add_(x, y):
    """x += y on the device (x, y contiguous float32 of equal size)."""
    with torch.cuda.device(x.device):
        _lib.check(_lib.load().cfd_add(_engine_handle(x.device), _ptr(x), _ptr(y), x.numel(), _stream(x)))
        _lib.wrote(x)
    return x


def mha(attn, query, key, value, key_padding_mask=None):
    """``nn.MultiheadAttention.forward(query, key, value, key_padding_mask=...)[0]`` for [L, N, E] tensors."""
    E, H = attn.embed_dim, attn.num_heads
    W, B = attn.in_proj_weight, attn.in_proj_bias
    q = linear_act(query, W[:E], B[:E])
    k = linear_act(key, W[E:2 * E], B[E:2 * E])
    v = linear_act(value, W[2 * E:], B[2 * E:])
    Lq, N, _ = q.shape
    Lk = k.shape[0]
    out = torch.empty_like(q)
    kpm = None
    if key_padding_mask is not None:
        kpm = key_padding_mask.to(device=q.device, dtype=torch.uint8).contiguous()
    with torch.cuda.device(q.device):
        _lib.check(_lib.load().cfd_mha(_engine_handle(q.device), _ptr(q), _ptr(k), _ptr(v), Lq, Lk, N, E, H,
                                       _ptr(kpm) if kpm is not None else None, _ptr(out), _stream(q)))
    return linear_act(out, attn.out_proj.weight, attn.out_proj.bias)


class _EncoderLayer(nn.Module):
    """Parameter layout of TransformerEncoderLayer (cross_attention.py:250-308); only held for checkpoint loading."""

    def __init__(self, d, nhead, ff):
        super().__init__()
        self.self_attn = nn.MultiheadAttention(d, nhead)
        self.linear1 = nn.Linear(d, ff)
        self.linear2 = nn.Linear(ff, d)
        self.norm1 = nn.LayerNorm(d)
        self.norm2 = nn.LayerNorm(d)


class _DecoderLayer(nn.Module):
    """TransformerDecoderLayer, pre-norm, eval mode (cross_attention.py:311-382)."""

    def __init__(self, d, nhead, ff):
        super().__init__()
        self.self_attn = nn.MultiheadAttention(d, nhead)
        self.multihead_attn = nn.MultiheadAttention(d, nhead)
        self.linear1 = nn.Linear(d, ff)
        self.linear2 = nn.Linear(ff, d)
        self.norm1 = nn.LayerNorm(d)
        self.norm2 = nn.LayerNorm(d)
        self.norm3 = nn.LayerNorm(d)

    def run(self, tgt, memory, tgt_key_padding_mask):
        t2 = layer_norm(tgt, self.norm1)                                                      # :368
        add_(tgt, mha(self.self_attn, t2, t2, t2, tgt_key_padding_mask))                      # :369-372
        t2 = layer_norm(tgt, self.norm2)                                                      # :373
        add_(tgt, mha(self.multihead_attn, t2, memory, memory, None))                         # :374-378
        t2 = layer_norm(tgt, self.norm3)                                                      # :379
        h = linear_act(t2, self.linear1.weight, self.linear1.bias, ACT_GELU)                  # :380
        add_(tgt, linear_act(h, self.linear2.weight, self.linear2.bias, ACT_NONE))            # :380-381
        return tgt


class _Skip(nn.Module):
    """SkipTransformerEncoder / SkipTransformerDecoder parameter layout and the decoder's forward (:66-125)."""

    def __init__(self, layer_cls, d, nhead, ff, num_layers):
        super().__init__()
        assert num_layers % 2 == 1
        nb = (num_layers - 1) // 2
        self.norm = nn.LayerNorm(d)
        self.input_blocks = nn.ModuleList([layer_cls(d, nhead, ff) for _ in range(nb)])
        self.middle_block = layer_cls(d, nhead, ff)
        self.output_blocks = nn.ModuleList([layer_cls(d, nhead, ff) for _ in range(nb)])
        self.linear_blocks = nn.ModuleList([nn.Linear(2 * d, d) for _ in range(nb)])

    def run(self, tgt, memory, tgt_key_padding_mask):
        x, xs = tgt, []
        for blk in self.input_blocks:
            x = blk.run(x, memory, tgt_key_padding_mask)
            xs.append(x.clone())
        x = self.middle_block.run(x, memory, tgt_key_padding_mask)
        for blk, lin in zip(self.output_blocks, self.linear_blocks):
            x = linear_act(torch.cat([x, xs.pop()], dim=-1), lin.weight, lin.bias)
            x = blk.run(x, memory, tgt_key_padding_mask)
        return layer_norm(x, self.norm)


class _SinePE(nn.Module):
    def __init__(self, d, max_len=1024):
        super().__init__()
        from .denoiser import sine_pe
        self.register_buffer("pe", sine_pe(max_len, d))


class ConvoFusionVae(nn.Module):
    def __init__(self, ablation, nfeats, latent_dim=[1, 256], ff_size=1024, num_layers=9, num_heads=4, dropout=0.1,
                 arch="all_encoder", normalize_before=False, activation="gelu", position_embedding="learned", **kwargs):
        super().__init__()
        if arch != "encoder_decoder" or not normalize_before or activation != "gelu" or position_embedding not in ("sine", "v2"):
            raise ValueError("the HIP VAE decoder implements the shipped configuration only (configs/modules/motion_vae.yaml: "
                             "arch 'encoder_decoder', pre-norm, gelu, sine position embedding)")
        if getattr(ablation, "PE_TYPE", "convofusion") != "convofusion":
            raise ValueError("Not support position encoding type!")          # vae.py:350
        if getattr(ablation, "MLP_DIST", False):
            raise ValueError("MLP_DIST=True is not supported by the HIP VAE mirror")
        self.latent_size, self.latent_dim = latent_dim[0], latent_dim[-1]
        self.body_nfeats, self.hands_nfeats = 23 * 3, 40 * 3                  # vae.py:53-54
        self.arch, self.num_heads, self.num_layers, self.ff_size = arch, num_heads, num_layers, ff_size
        self._packs = {}                                                      # name -> (key, pack): _cached_pack
        d = self.latent_dim
        self.body_global_motion_token = nn.Parameter(torch.randn(self.latent_size * 2, d))
        self.hands_global_motion_token = nn.Parameter(torch.randn(self.latent_size * 2, d))
        self.query_pos_encoder = _SinePE(d)
        self.query_pos_decoder = _SinePE(d)
        self.mem_pos_decoder = _SinePE(d)
        self.body_encoder = _Skip(_EncoderLayer, d, num_heads, ff_size, num_layers)
        self.hands_encoder = _Skip(_EncoderLayer, d, num_heads, ff_size, num_layers)
        self.body_decoder = _Skip(_DecoderLayer, d, num_heads, ff_size, num_layers)
        self.hands_decoder = _Skip(_DecoderLayer, d, num_heads, ff_size, num_layers)
        self.body_skel_embedding = nn.Linear(self.body_nfeats, d)
        self.hands_skel_embedding = nn.Linear(self.hands_nfeats, d)
        self.body_final_layer = nn.Linear(d, self.body_nfeats)
        self.hands_final_layer = nn.Linear(d, self.hands_nfeats)

    def forward(self, features, lengths=None):
        raise NotImplementedError("convofusion_amd.vae.ConvoFusionVae provides encode() and decode() only; training uses the "
                                  "reference module")

    def _encoder_sources(self):
        """(tensor, pad K to) in the order of the packed layout (csrc/vae_enc.hpp); pad None = a vector, 0 = a matrix as it is."""
        src = []
        for enc, emb, tok in ((self.body_encoder, self.body_skel_embedding, self.body_global_motion_token),
                              (self.hands_encoder, self.hands_skel_embedding, self.hands_global_motion_token)):
            src += [(emb.weight, ENC_D), (emb.bias, None), (tok, None), (self.query_pos_encoder.pe[:ENC_TOKENS], None)]
            for blk in list(enc.input_blocks) + [enc.middle_block] + list(enc.output_blocks):
                a = blk.self_attn
                src += [(blk.norm1.weight, None), (blk.norm1.bias, None), (a.in_proj_weight, 0), (a.in_proj_bias, None),
                        (a.out_proj.weight, 0), (a.out_proj.bias, None), (blk.norm2.weight, None), (blk.norm2.bias, None),
                        (blk.linear1.weight, 0), (blk.linear1.bias, None), (blk.linear2.weight, 0), (blk.linear2.bias, None)]
            for lin in enc.linear_blocks:
                src += [(lin.weight, 0), (lin.bias, None)]
            src += [(enc.norm.weight, None), (enc.norm.bias, None)]
        return src

    def _cached_pack(self, name, dev, src, parts_of, n_floats):
        """The packed copy ``name`` of the sources ``src`` [(tensor, kind)] on ``dev``: ``parts_of(tensor on dev as float32, kind)`` lists a
        source's parts; rebuilt when any source tensor was replaced or written (its address or version counter moved)."""
        key = (str(dev),) + tuple((t.data_ptr(), t._version) for t, _ in src)
        if name not in self._packs or self._packs[name][0] != key:
            pack = torch.cat([part for t, kind in src for part in parts_of(t.detach().to(dev, torch.float32), kind)]).contiguous()
            assert pack.numel() == n_floats, pack.numel()
            self._packs[name] = (key, pack)
        return self._packs[name][1]

    def _encoder_pack(self, dev):
        """The packed encoder weights of both stacks on ``dev`` (``_cached_pack``)."""
        return self._cached_pack("encoder", dev, self._encoder_sources(), lambda t, k: [_pack_w(t, k) if k is not None else t.reshape(-1)],
                                 2 * encoder_pack_floats(self.num_layers))

    def _encode_spec_error(self):
        if (self.latent_dim, self.num_heads, self.ff_size, self.latent_size) != (ENC_D, 2, 1024, 1) or self.num_layers > 9:
            return (f"the HIP VAE encoder is specialised for latent_dim [1, 128], 2 heads, ff_size 1024 and odd num_layers <= 9 "
                    f"(configs/modules/motion_vae.yaml); this module has latent_dim [{self.latent_size}, {self.latent_dim}], "
                    f"{self.num_heads} heads, ff_size {self.ff_size}, {self.num_layers} layers")
        return None

    @torch.no_grad()
    def encode(self, features, lengths=None):
        """features [bs, nframes, 189] (any strides), lengths: frames per sequence (list / tuple / 1-D tensor; None = all nframes)
        -> (latent [2, bs, nframes / 16, 128], torch.distributions.Normal(mu, std) over [2, bs * nframes / 16, 128],
        root-subtracted features [bs, nframes, 189])  (vae.py:162-266)."""
        nf = self.body_nfeats + self.hands_nfeats
        if features.dim() != 3 or features.shape[-1] != nf:
            raise ValueError(f"features must be [bs, nframes, {nf}], got {tuple(features.shape)}")
        bs, nframes, _ = features.shape
        lens = _lengths_list(lengths, [nframes] * bs)                                        # vae.py:168
        if bs < 1 or len(lens) != bs:
            raise ValueError(f"{len(lens)} lengths for a batch of {bs}")
        if nframes < 16 or nframes % 16:
            raise ValueError(f"nframes must be a positive multiple of 16 (16-frame chunks, vae.py:178), got {nframes}")
        if max(lens) != nframes or min(lens) < 0:
            raise ValueError(f"max(lengths) must equal nframes = {nframes} (the reference's mask reshape, vae.py:189), got {max(lens)}")
        err = self._encode_spec_error()
        if err:
            raise ValueError(err)
        if features.device.type != "cuda":
            raise NotImplementedError("the HIP VAE encoder runs on an MI355X only (move the module and the features to 'cuda'); "
                                      "no CPU path")
        dev = features.device
        n_chunks = nframes // 16
        x = features.detach().to(torch.float32)
        if x.stride(2) != 1 or x.stride(0) != nframes * x.stride(1) or x.stride(1) < nf:
            x = x.contiguous()                          # one row stride between all (sequence, frame) rows
        pack = self._encoder_pack(dev)
        lens_d = torch.tensor(lens, dtype=torch.int32, device=dev)
        mulv = torch.empty(2, 2, bs * n_chunks, ENC_D, device=dev)
        feats = torch.empty(bs, nframes, nf, device=dev)
        with torch.cuda.device(dev):
            _lib.check(_lib.load().cfd_vae_encode(_engine_handle(dev), _ptr(pack), self.latent_dim, self.num_heads, self.ff_size,
                                                  self.num_layers, self.latent_size, _ptr(x), bs, nframes, x.stride(1), _ptr(lens_d),
                                                  _ptr(mulv), _ptr(feats), 0, _stream(x)))
        mu, logvar = mulv[0], mulv[1]                                                      # vae.py:250-253
        std = logvar.exp().pow(0.5)                                                        # :256-258
        dist = torch.distributions.Normal(mu, std)
        latent = dist.rsample()
        return latent.reshape(-1, bs, n_chunks, self.latent_dim), dist, feats

    def decode(self, z, lengths, fused=False):
        """z [2, bs, n_chunks, latent_dim] (body | hands), lengths: frames per sequence -> feats [bs, nframes, 189].  Differentiable with
        respect to z when grad is enabled and ``z.requires_grad`` (backward: ``decode_vjp``); the values are the same bits either way.
        fused=True: the forward of ``decode_vjp`` as one cfd_vae_decode call instead of the launch sequence (its bits, about 1e-5 from the
        default's; padded frames exactly 0); under grad the forward is kept and the backward is the sweep alone (``_DecodeFused``).
        NotImplementedError beyond the kernels' limits (``decode_vjp_refusal``), before any device work."""
        if fused:
            lens = _lengths_list(lengths)
            why = self._decode_vjp_refusal(z, lens, None, forward=True)
            if why:
                raise NotImplementedError(f"decode(fused=True): {why}")
            if z.device.type != "cuda":
                raise RuntimeError("the HIP VAE decoder runs on an MI355X only (move the module and z to 'cuda'); no CPU fallback")
            if torch.is_grad_enabled() and z.requires_grad:
                return _DecodeFused.apply(z, self, lens)
            return self._decode_fused(z, lens, keep=False)[0]
        if z.device.type != "cuda":
            raise RuntimeError("the HIP VAE decoder runs on an MI355X only (move the module and z to 'cuda'); no CPU fallback")
        if torch.is_grad_enabled() and z.requires_grad:
            lens = _lengths_list(lengths)
            why = self._decode_vjp_refusal(z, lens, None)
            if why:
                raise NotImplementedError(f"decode cannot be differentiated here: {why}")
            return _DecodeVjp.apply(z, self, lens)
        return self._decode_launches(z, lengths)

    @torch.no_grad()
    def _decode_launches(self, z, lengths):
        _, bs, n_chunks, D = z.shape
        dev = z.device
        lens = torch.as_tensor(list(lengths), device=dev)
        nframes = int(max(lengths))
        mask = torch.arange(nframes, device=dev).expand(bs, nframes) < lens.unsqueeze(1)      # lengths_to_mask
        # queries = zeros + PE = the PE rows themselves (vae.py:277,328)
        queries = self.query_pos_decoder.pe[:nframes].to(torch.float32).expand(nframes, bs, D).contiguous()
        pe_mem = self.mem_pos_decoder.pe[:n_chunks].to(torch.float32).expand(n_chunks, bs, D).contiguous()
        kpm = ~mask
        outs = []
        for dec, fin, zi in ((self.body_decoder, self.body_final_layer, z[0]), (self.hands_decoder, self.hands_final_layer, z[1])):
            mem = zi.detach().to(torch.float32).permute(1, 0, 2).contiguous()                 # :281-286
            add_(mem, pe_mem)                                                                  # :329,339
            x = dec.run(queries.clone(), mem, kpm)                                            # :330-347
            outs.append(linear_act(x, fin.weight, fin.bias))                                  # :359-360
        out = torch.cat(outs, dim=-1).contiguous()                                            # :362
        keep = mask.t().contiguous().to(torch.uint8)                                          # rows are (frame, batch)
        with torch.cuda.device(dev):
            _lib.check(_lib.load().cfd_zero_rows(_engine_handle(dev), _ptr(out), _ptr(keep), nframes * bs, out.shape[-1], _stream(out)))
            _lib.wrote(out)
        return out.permute(1, 0, 2)                                                           # :370

    def _decoder_sources(self):
        """(tensor, kind) in the order of the packed layout (csrc/vae_dec.hpp).  kind: "v" a vector, "m" a matrix stored in both orders,
        "f" / "fb" final_layer's weight / bias, zero-padded to 128 output features."""
        src = []
        for dec, fin in ((self.body_decoder, self.body_final_layer), (self.hands_decoder, self.hands_final_layer)):
            for blk in list(dec.input_blocks) + [dec.middle_block] + list(dec.output_blocks):
                sa, ca = blk.self_attn, blk.multihead_attn
                src += [(blk.norm1.weight, "v"), (blk.norm1.bias, "v"), (sa.in_proj_weight, "m"), (sa.in_proj_bias, "v"),
                        (sa.out_proj.weight, "m"), (sa.out_proj.bias, "v"), (blk.norm2.weight, "v"), (blk.norm2.bias, "v"),
                        (ca.in_proj_weight, "m"), (ca.in_proj_bias, "v"), (ca.out_proj.weight, "m"), (ca.out_proj.bias, "v"),
                        (blk.norm3.weight, "v"), (blk.norm3.bias, "v"), (blk.linear1.weight, "m"), (blk.linear1.bias, "v"),
                        (blk.linear2.weight, "m"), (blk.linear2.bias, "v")]
            for lin in dec.linear_blocks:
                src += [(lin.weight, "m"), (lin.bias, "v")]
            src += [(dec.norm.weight, "v"), (dec.norm.bias, "v"), (fin.weight, "f"), (fin.bias, "fb")]
        src += [(self.query_pos_decoder.pe[:DEC_MAX_FRAMES], "v"), (self.mem_pos_decoder.pe[:DEC_MAX_CHUNKS], "v")]
        return src

    def _decoder_pack(self, dev):
        """The packed decoder weights of both stacks and the two PE tables on ``dev`` (``_cached_pack``, like the encoder's)."""
        def parts_of(t, kind):
            if kind in ("v", "fb"):
                t = t.reshape(-1)
                return [F.pad(t, (0, ENC_D - t.numel())) if kind == "fb" else t]
            if kind == "f":
                t = F.pad(t, (0, 0, 0, ENC_D - t.shape[0]))
            return [_pack_w(t), _pack_w(t.t().contiguous())]
        return self._cached_pack("decoder", dev, self._decoder_sources(), parts_of, decoder_pack_floats(self.num_layers))

    def _decode_vjp_refusal(self, z, lens, d_feats, forward=False):
        """ValueError for arguments ``decode_vjp`` cannot mean anything for; returns the NotImplementedError text for shapes beyond the
        kernels' limits (``decode_vjp_refusal``; forward: worded for ``decode(fused=True)``) or None.  No library, no device."""
        nf = self.body_nfeats + self.hands_nfeats
        if z.dim() != 4 or z.shape[0] != 2 or z.shape[-1] != self.latent_dim:
            raise ValueError(f"z must be [2, bs, n_chunks, {self.latent_dim}], got {tuple(z.shape)}")
        bs, n_chunks = int(z.shape[1]), int(z.shape[2])
        if bs < 1 or n_chunks < 1 or len(lens) != bs:
            raise ValueError(f"{len(lens)} lengths for z of shape {tuple(z.shape)}")
        if min(lens) < 1:
            raise ValueError(f"every length must be at least 1, got {min(lens)}")
        if d_feats is not None:
            if d_feats.dim() != 3 or d_feats.shape[0] != bs or d_feats.shape[2] != nf:
                raise ValueError(f"d_feats must be [{bs}, nframes, {nf}], got {tuple(d_feats.shape)}")
            if max(lens) != d_feats.shape[1]:
                raise ValueError(f"max(lengths) = {max(lens)} must equal d_feats.shape[1] = {d_feats.shape[1]}")
        return decode_vjp_refusal(bs, max(lens), n_chunks, self.latent_dim, self.num_heads, self.ff_size, self.num_layers, self.latent_size,
                                  forward=forward)

    def _decode_fused(self, z, lens, keep):
        """(feats, ticket): one cfd_vae_decode on checked arguments.  keep False: forward-only, ticket 0.  keep True: the forward with saves;
        the ticket names it on the device's engine handle until another decode call uses the VAE workspace.  Waits as ``decode_vjp`` does."""
        dev = z.device
        bs, n_chunks, nframes = int(z.shape[1]), int(z.shape[2]), max(lens)
        zc = z.detach().to(torch.float32).contiguous()
        pack = self._decoder_pack(dev)
        lens_d = torch.tensor(lens, dtype=torch.int32, device=dev)
        feats = torch.empty(bs, nframes, self.body_nfeats + self.hands_nfeats, device=dev)
        args = _lib.VaeDecodeArgs(_ptr(pack), self.latent_dim, self.num_heads, self.ff_size, self.num_layers, bs, nframes, n_chunks,
                                  _ptr(zc), _ptr(lens_d))
        ticket = C.c_uint64(0)
        with torch.cuda.device(dev):
            # (decode_vjp's rule and reason: an open sampling run replays and reads on a stream of its own.  The forward-only call writes a
            # fresh torch block -- feats -- and runs beside such a replay just the same, so it needs no less.)
            torch.cuda.synchronize(dev)
            _lib.check(_lib.load().cfd_vae_decode(_engine_handle(dev), C.byref(args), _ptr(feats), C.byref(ticket) if keep else None,
                                                  _stream(zc)))
            torch.cuda.current_stream(dev).synchronize()
        return feats, ticket.value

    def _decode_sweep(self, ticket, d_feats, like):
        """d_z (shaped like ``like``, float32) of the reverse sweep over the forward ``ticket`` names (cfd_vae_decode_sweep), or None when
        the handle no longer keeps that forward -- asked before anything is launched (cfd_vae_decode_ticket)."""
        dev = like.device
        lib, h = _lib.load(), _engine_handle(dev)
        if not ticket or lib.cfd_vae_decode_ticket(h) != ticket:
            return None
        dc = d_feats.detach().to(device=dev, dtype=torch.float32).contiguous()
        d_z = torch.empty(like.shape, dtype=torch.float32, device=dev)
        with torch.cuda.device(dev):
            torch.cuda.synchronize(dev)
            _lib.check(lib.cfd_vae_decode_sweep(h, ticket, _ptr(dc), _ptr(d_z), _stream(dc)))
            torch.cuda.current_stream(dev).synchronize()
        return d_z

    def decode_vjp(self, z, lengths, d_feats, want_out=True):
        """(feats [bs, nframes, 189] or None, d_z [2, bs, n_chunks, 128]): ``decode(z, lengths)`` as one cfd_vae_decode_vjp call computes
        it (padded frames exactly 0) and d_feats^T . d(feats)/d(z) -- torch.autograd.grad(decode(z, lengths), z, d_feats) of the
        reference.  d_feats [bs, nframes, 189] is the cotangent at decode's output; its rows at or beyond a sequence's length are not
        read.  Deterministic: the same inputs give the same bits.  Returns with its results complete.  ValueError: a length below 1, a wrong shape, max(lengths) !=
        d_feats.shape[1]; NotImplementedError beyond the kernels' limits (``decode_vjp_refusal``), before any device work."""
        lens = _lengths_list(lengths)
        why = self._decode_vjp_refusal(z, lens, d_feats)
        if why:
            raise NotImplementedError(f"decode_vjp: {why}")
        if z.device.type != "cuda":
            raise RuntimeError("the HIP VAE decoder runs on an MI355X only (move the module and z to 'cuda'); no CPU fallback")
        dev = z.device
        bs, n_chunks, nframes = int(z.shape[1]), int(z.shape[2]), max(lens)
        zc = z.detach().to(torch.float32).contiguous()
        dc = d_feats.detach().to(device=dev, dtype=torch.float32).contiguous()
        pack = self._decoder_pack(dev)
        lens_d = torch.tensor(lens, dtype=torch.int32, device=dev)
        feats = torch.empty(bs, nframes, self.body_nfeats + self.hands_nfeats, device=dev) if want_out else None
        d_z = torch.empty_like(zc)
        args = _lib.VaeDecodeVjpArgs(_ptr(pack), self.latent_dim, self.num_heads, self.ff_size, self.num_layers, bs, nframes, n_chunks,
                                     _ptr(zc), _ptr(lens_d), _ptr(dc))
        with torch.cuda.device(dev):
            # The C call only enqueues.  This wrapper waits on both sides, as ``Denoiser.vjp`` returns with its results complete: an open
            # sampling run replays on a stream of its own and ``SamplingRun.read`` fills a fresh tensor through that stream, so launches of
            # this call that were still pending could run beside a replay (two queues at once: DESIGN.md section 6) or write into a block
            # torch has already handed to such a tensor.
            torch.cuda.synchronize(dev)
            _lib.check(_lib.load().cfd_vae_decode_vjp(_engine_handle(dev), C.byref(args), _ptr(feats) if want_out else None, _ptr(d_z),
                                                      _stream(zc)))
            torch.cuda.current_stream(dev).synchronize()
        return feats, d_z


class _DecodeVjp(torch.autograd.Function):
    """``ConvoFusionVae.decode``'s launch sequence as a function of ``z``; backward: ``decode_vjp`` on the saved INPUT (it recomputes the
    forward with saves, so nothing but z outlives the call)."""

    @staticmethod
    def forward(ctx, z, vae, lens):
        ctx.vae, ctx.lens = vae, lens
        ctx.save_for_backward(z)
        return vae._decode_launches(z, lens)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, d_feats):
        (z,) = ctx.saved_tensors
        return ctx.vae.decode_vjp(z, ctx.lens, d_feats, want_out=False)[1].to(z.dtype), None, None


class _DecodeFused(torch.autograd.Function):
    """``decode(z, lengths, fused=True)`` as a function of ``z``: the forward is kept in the engine handle's VAE workspace and the backward
    is the reverse sweep over it.  The handle keeps one forward: when another decode call has used the workspace since, the backward is
    ``decode_vjp`` on the saved input instead (the forward again, then the same sweep) -- the same bits, never an exception."""

    @staticmethod
    def forward(ctx, z, vae, lens):
        feats, ctx.ticket = vae._decode_fused(z, lens, keep=True)
        ctx.vae, ctx.lens = vae, lens
        ctx.save_for_backward(z)
        return feats

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, d_feats):
        (z,) = ctx.saved_tensors
        d_z = ctx.vae._decode_sweep(ctx.ticket, d_feats, z)
        if d_z is None:
            d_z = ctx.vae.decode_vjp(z, ctx.lens, d_feats, want_out=False)[1]
        return d_z.to(z.dtype), None, None


DEC_MAX_FRAMES, DEC_MAX_CHUNKS = 256, 16     # VD_MAX_FRAMES, VD_MAX_CHUNKS (csrc/vae_dec.hpp)


def decode_vjp_refusal(bs, nframes, n_chunks, latent_dim=128, num_heads=2, ff_size=1024, num_layers=5, latent_size=1, forward=False):
    """Why ``ConvoFusionVae.decode`` cannot be differentiated at these shapes, or None when it can: the message names the limit that is
    exceeded.  forward=True: the same limits worded for ``decode(fused=True)``, which runs on the same kernels ("fused forward" where the
    text says "backward").  Pure: no library, no device."""
    what, whose = ("fused forward", "decoder fused forward's") if forward else ("backward", "decoder backward's")
    if (latent_dim, num_heads, ff_size, latent_size) != (128, 2, 1024, 1) or num_layers > 9 or num_layers % 2 == 0:
        return (f"the HIP VAE decoder's {what} is specialised for latent_dim [1, 128], 2 heads, ff_size 1024 and odd num_layers <= 9; this "
                f"module has latent_dim [{latent_size}, {latent_dim}], {num_heads} heads, ff_size {ff_size}, {num_layers} layers")
    if nframes > DEC_MAX_FRAMES:
        return f"nframes = {nframes} exceeds the {whose} {DEC_MAX_FRAMES} frames"
    if n_chunks > DEC_MAX_CHUNKS:
        return f"n_chunks = {n_chunks} exceeds the {whose} {DEC_MAX_CHUNKS} latent chunks per sequence"
    if bs > 65535:
        return f"bs = {bs} exceeds the {whose} 65535 sequences per call"
    return None


def decoder_pack_floats(num_layers):
    """Floats of the packed decoder weights (vd_pack_floats, csrc/vae_dec.hpp)."""
    d, ff = 128, 1024
    layer = 6 * d + 2 * (2 * 3 * d * d + 3 * d) + 2 * (2 * d * d + d) + 2 * (2 * d * ff) + ff + d
    stack = num_layers * layer + (num_layers - 1) // 2 * (4 * d * d + d) + 2 * d + 2 * d * d + d
    return 2 * stack + (DEC_MAX_FRAMES + DEC_MAX_CHUNKS) * d


def _mirror_of(vae, skip):
    """A mirror built from a reference module's own hyper-parameters (read off its SkipTransformer ``skip``) and weights."""
    nl = 2 * len(skip.input_blocks) + 1
    attn = skip.middle_block.self_attn
    from types import SimpleNamespace
    m = ConvoFusionVae(ablation=SimpleNamespace(MLP_DIST=getattr(vae, "mlp_dist", False), PE_TYPE=getattr(vae, "pe_type", "convofusion")),
                       nfeats=vae.body_nfeats + vae.hands_nfeats, latent_dim=[vae.latent_size, vae.latent_dim],
                       ff_size=skip.middle_block.linear1.out_features, num_layers=nl, num_heads=attn.num_heads,
                       arch=vae.arch, normalize_before=skip.middle_block.normalize_before, activation="gelu",
                       position_embedding="sine")
    m.load_state_dict(vae.state_dict(), strict=True)
    return m.to(next(vae.parameters()).device).eval()


def _attach(vae, skip_attr, method):
    """Route ``vae.<method>`` of a REFERENCE ``ConvoFusionVae`` instance to the HIP path: builds the mirror from the module's own
    hyper-parameters (read off ``vae.<skip_attr>``) and weights and replaces the bound method.  The mirror takes a snapshot of the
    weights: call again after loading a different checkpoint.  Returns the mirror."""
    m = _mirror_of(vae, getattr(vae, skip_attr))
    setattr(vae, method, getattr(m, method))
    return m


def attach_hip_decode(vae, fused=False):
    """``vae.decode`` of a reference instance (kept for encode / training) on the HIP path (``_attach``).  fused=True: the attached
    ``decode(z, lengths)`` runs the mirror's ``decode(z, lengths, fused=True)`` unless its caller says otherwise.  Returns the mirror."""
    m = _attach(vae, "body_decoder", "decode")
    if fused:
        vae.decode = lambda z, lengths, fused=True: m.decode(z, lengths, fused=fused)
    return m


def attach_hip_encode(vae):
    """``vae.encode`` of a reference instance (kept for training) on the HIP path (``_attach``).  Returns the mirror."""
    return _attach(vae, "body_encoder", "encode")


ENC_D, ENC_TOKENS = 128, 18      # d_model, 2 global tokens + 16 frames per sequence


def encoder_pack_floats(num_layers):
    """Floats of one stack's block of the packed encoder weights (ve_stack_floats, csrc/vae_enc.hpp)."""
    d, ff = ENC_D, 1024
    layer = 4 * d + 3 * d * d + 3 * d + d * d + d + d * ff + ff + ff * d + d
    return d * d + d + 2 * d + ENC_TOKENS * d + num_layers * layer + (num_layers - 1) // 2 * (2 * d * d + d) + 2 * d


def _pack_w(w, k=0):
    """W [N][K] (nn.Linear) in the kernel's MFMA-B order, K zero-padded to ``k``: float4 ((n/16 * K/16 + k/16) * 64 + lane), lane =
    16 * ((k % 16) / 4) + n % 16, element k % 4."""
    n, k0 = w.shape
    if k and k != k0:
        w = F.pad(w, (0, k - k0))
    kk = w.shape[1]
    return w.reshape(n // 16, 16, kk // 16, 4, 4).permute(0, 2, 3, 1, 4).reshape(-1)
