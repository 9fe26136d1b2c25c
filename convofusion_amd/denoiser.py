"""Drop-in for ``convofusion.models.architectures.denoiser.Denoiser`` backed by libcfdenoise.

Same constructor signature (reference convofusion/models/architectures/denoiser.py:18-39), same
``forward(sample, timestep, encoder_hidden_states, lengths=None, mem_mask_dict={}, **kwargs)
-> (sample, att_mats)`` (:173-179,386) and the same 537-entry state-dict layout (SURVEY.md
section 8b), so ``instantiate_from_config`` (convofusion/config.py:24-31) can point at it by
changing ``target`` in configs/modules/denoiser.yaml, and ``model.load_state_dict`` of a reference
checkpoint loads strictly.  The torch modules below are parameter CONTAINERS only: the forward is
the HIP path.

Autograd: ``forward`` is differentiable with respect to ``sample`` -- and, with ``memory_grad=True``, with respect to
its five memories; never to parameters.  Under grad mode with ``sample.requires_grad`` the returned output carries a
``grad_fn`` (``_DenoiseVjp``, once differentiable): its forward is the inference path (bit-identical output), its
backward one ``cfd_denoise_vjp`` call, which recomputes the forward with saved activations and runs the reverse sweep
of the row-tile kernels, so no activation state outlives a call.  The attention maps come back detached; shapes beyond
the row-tile path (``vjp_refusal``) and per-row timesteps are refused before any device work.

Without the keyword no gradient reaches a memory (one that requires grad is refused).  ``forward(..., memory_grad=True)``
takes the differentiable path when the sample OR a memory requires grad: the same ``_DenoiseVjp`` (sample and the five
memories are its tensor arguments in both modes), whose backward then asks for exactly what requires grad -- one
``cfd_denoise_vjp_mem`` call with one memory per batch row, so every input row gets its own gradient, as torch autograd gives
the reference.  ``vjp_memories`` is the direct call: distinct memories with row maps receive the sum over the rows that share
them, which is what fitting one conditioning tensor to several examples needs (``convofusion_amd.fit``).  ``vjp``,
``vjp_memories`` and that backward are one marshalling body, ``Denoiser._vjp_call``.
"""
import copy
import ctypes as C
import math
import os

import torch
from torch import nn

from . import _lib

MEM_NAMES = _lib.MEM_NAMES
# declaration order of the reference layer (cross_attention.py:451-459) -- matters for state-dict order
_MHA_DECL_ORDER = ("spkemb", "tlsn", "alsn", "apb", "lsnemb")


def sinusoid_table(n_rows, dim=512, flip_sin_to_cos=True, downscale_freq_shift=0.0, max_period=10000):
    """Rows t = 0..n_rows-1 of get_timestep_embedding (reference tools/embeddings.py:245-285), computed
    with the same torch float32 ops so the table is bit-identical to what the reference feeds its MLP."""
    half = dim // 2
    exponent = -math.log(max_period) * torch.arange(start=0, end=half, dtype=torch.float32)
    exponent = exponent / (half - downscale_freq_shift)
    emb = torch.exp(exponent)
    emb = torch.arange(n_rows)[:, None].float() * emb[None, :]
    emb = torch.cat([torch.sin(emb), torch.cos(emb)], dim=-1)
    if flip_sin_to_cos:
        emb = torch.cat([emb[:, half:], emb[:, :half]], dim=-1)
    return emb.contiguous()


def sine_pe(max_len, d_model=512):
    """PositionEmbeddingSine1D / SineBH buffer (reference operator/position_encoding.py:118-125)."""
    pe = torch.zeros(max_len, d_model)
    position = torch.arange(0, max_len, dtype=torch.float).unsqueeze(1)
    div_term = torch.exp(torch.arange(0, d_model, 2).float() * (-math.log(10000.0) / d_model))
    pe[:, 0::2] = torch.sin(position * div_term)
    pe[:, 1::2] = torch.cos(position * div_term)
    return pe.unsqueeze(0).transpose(0, 1).contiguous()


def _contents_signature(tensors, force_checksum=False):
    """Per tensor (version counter or None, device checksum or None): what ``Denoiser.forward`` compares between two calls that pass the same
    tensor objects.  The version counter catches every in-place torch op for free.  Tensors created under ``torch.inference_mode()`` --
    everything the reference's test loop passes, pytorch_lightning's Trainer runs it in inference mode -- have no version counter
    (reading it raises); for those, and for every tensor with ``force_checksum``, a checksum of the bytes stands in: three strided integer
    sums per tensor, all tensors' sums fetched with ONE host read."""
    vers, todo = [], []
    for i, t in enumerate(tensors):
        v = None
        if t is not None:
            try:
                v = None if t.is_inference() else t._version
            except RuntimeError:      # "Inference tensors do not track version counter"
                v = None
            if v is None or force_checksum:
                todo.append(i)
        vers.append(v)
    sums = [None] * len(tensors)
    if todo:
        parts = []
        for i in todo:
            t = tensors[i].detach()
            flat = (t if t.is_contiguous() else t.contiguous()).reshape(-1)
            w = flat.view(torch.int32) if flat.element_size() == 4 else flat.view(torch.uint8)
            parts.append(torch.stack([w.sum(dtype=torch.int64), w[::7].sum(dtype=torch.int64), w[3::13].sum(dtype=torch.int64)]))
        got = torch.stack(parts).tolist()     # the one synchronising read
        for i, g in zip(todo, got):
            sums[i] = tuple(g)
    return list(zip(vers, sums))


# The limits of the differentiable forward: those of the row-tile path of the library (csrc/rowtile.hpp RT_MAX_L / RT_MAX_KEYS; the
# handle's rt_max_rows, which the developer knob CFD_ROWTILE_MAX_ROWS moves).
VJP_MAX_L = 32
VJP_MAX_KEYS = 1024
VJP_MAX_ROWS = 700


def vjp_max_rows():
    try:
        return int(os.environ.get("CFD_ROWTILE_MAX_ROWS", VJP_MAX_ROWS))
    except ValueError:
        return VJP_MAX_ROWS


def vjp_refusal(Be, L, S, max_rows=None):
    """Why ``Denoiser.forward`` cannot be differentiated at batch ``Be``, ``L`` tokens per row and memory lengths ``S`` (five ints), or
    None when it can: the message names the limit that is exceeded.  Pure: no library, no device."""
    max_rows = vjp_max_rows() if max_rows is None else int(max_rows)
    if L > VJP_MAX_L:
        return f"L = {L} tokens per batch row exceed the row-tile path's {VJP_MAX_L}"
    if Be * L > max_rows:
        return f"Be * L = {Be * L} token rows exceed the row-tile path's {max_rows}"
    keys = sum((int(s) + 31) // 32 * 32 for s in S)
    if keys > VJP_MAX_KEYS:
        return f"{keys} padded keys of the five memories together (each length rounded up to 32) exceed the row-tile path's {VJP_MAX_KEYS}"
    return None


# The guide call (``Denoiser.guide``, cfd_denoise_guide) has a row limit of its own in place of VJP_MAX_ROWS: the handle's guide_max_rows,
# which the developer knob CFD_GUIDE_MAX_ROWS moves.
GUIDE_MAX_ROWS = 4096


def guide_max_rows():
    try:
        return int(os.environ.get("CFD_GUIDE_MAX_ROWS", GUIDE_MAX_ROWS))
    except ValueError:
        return GUIDE_MAX_ROWS


def guide_refusal(Be, L, S, max_rows=None):
    """Why ``Denoiser.guide`` cannot run ``Be`` = chunks x latent rows forward rows of ``L`` tokens against memory lengths ``S`` (five
    ints), or None when it can: ``vjp_refusal`` with the guide call's own row limit.  Pure: no library, no device."""
    max_rows = guide_max_rows() if max_rows is None else int(max_rows)
    if L <= VJP_MAX_L and Be * L > max_rows:
        return f"Be * L = {Be * L} token rows exceed the guide call's {max_rows}"
    return vjp_refusal(Be, L, S, max_rows=max_rows)


def guide_pose_refusal(Be, L, S, bs, nframes, max_rows=None, **decoder):
    """Why ``Denoiser.guide_pose`` cannot run ``Be`` forward rows of ``L`` tokens against memory lengths ``S`` with ``bs`` latent rows
    decoded to ``nframes`` frames, or None when it can: ``guide_refusal``, then ``vae.decode_vjp_refusal`` for bs sequences of L / 2
    chunks (``decoder``: that function's keywords -- latent_dim, num_heads, ff_size, num_layers, latent_size), then the two limits
    that belong to the pair.  Pure: no library, no device."""
    from .vae import decode_vjp_refusal
    why = guide_refusal(Be, L, S, max_rows=max_rows)
    if why is not None:
        return why
    if L % 2:
        return f"L = {L} is odd: a latent chunk is a body and a hands token"
    why = decode_vjp_refusal(bs, nframes, L // 2, **decoder)
    if why is not None:
        return why
    if nframes < 1 or nframes > 16 * (L // 2):
        return f"nframes = {nframes} is not in [1, 16 * (L / 2)] = [1, {16 * (L // 2)}], the frames of {L // 2} latent chunks"
    return None


def tie_csr(tie):
    """The inverse of a tie table [B, L] (``run_kind.check_tie``) as ``Denoiser.guide`` takes it: int32 [2 B L + 1] on the table's
    device, built on the host by cfd_guide_tie_csr (offsets, then every source's tied tokens in ascending order)."""
    import numpy as np
    host = np.ascontiguousarray(tie.detach().to("cpu", torch.int32).numpy().reshape(-1))
    csr = np.empty(2 * host.size + 1, dtype=np.int32)
    _lib.check(_lib.load().cfd_guide_tie_csr(host.ctypes.data, host.size, csr.ctypes.data))
    return torch.from_numpy(csr).to(tie.device)


def _require_row_tile(sample, mems, what):
    """The refusal of a gradient with respect to ``what`` ("its sample" ...) at shapes beyond the row-tile path."""
    why = vjp_refusal(sample.shape[0], sample.shape[1], [int(m.shape[1]) for m in mems])
    if why is not None:
        raise NotImplementedError(f"the gradient of the HIP denoiser with respect to {what} runs on the row-tile path only: {why}")


class _DenoiseVjp(torch.autograd.Function):
    """``out`` of ``Denoiser._forward_hip`` as a function of ``sample`` and the five memories (tensor arguments, so that autograd can reach
    them; ``memory_grad`` says whether it may).  Backward: one ``Denoiser._vjp_call`` on the saved INPUTS for exactly what
    ``needs_input_grad`` names -- with memories, one per batch row (U = Be, no row map)."""

    @staticmethod
    def forward(ctx, denoiser, timestep, mem_mask_dict, kwargs, memory_grad, sample, *mems):
        out, att = denoiser._forward_hip(sample, timestep, list(mems), mem_mask_dict, kwargs)
        ctx.denoiser, ctx.t, ctx.side = denoiser, int(torch.as_tensor(timestep).reshape(-1)[0].item()), bool(kwargs.get("side_engine", False))
        ctx.masks, ctx.memory_grad = dict(mem_mask_dict or {}), memory_grad
        ctx.save_for_backward(sample, *mems)
        ctx.mark_non_differentiable(*att)
        return (out, *att)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, d_out, *d_att):
        sample, *mems = ctx.saved_tensors
        need = ctx.needs_input_grad[5:]
        wrt = tuple(name for name, n in zip(MEM_NAMES, need[1:]) if n) if ctx.memory_grad else ()
        _, grad, d_mem = ctx.denoiser._vjp_call(sample, ctx.t, mems, ctx.masks, d_out, wrt, None, ctx.side, False, bool(need[0]) or not wrt,
                                                "its sample and memories" if ctx.memory_grad else "its sample")
        return (None, None, None, None, None, grad) + tuple(d_mem.get(name) for name in MEM_NAMES)


class _PE(nn.Module):
    def __init__(self, d_model, max_len=1024):
        super().__init__()
        self.register_buffer("pe", sine_pe(max_len, d_model))


class _TimestepEmbedding(nn.Module):
    def __init__(self, channel, time_embed_dim):
        super().__init__()
        self.linear_1 = nn.Linear(channel, time_embed_dim)
        self.linear_2 = nn.Linear(time_embed_dim, time_embed_dim)


class _TimeBlock(nn.Module):
    def __init__(self, d, dropout):
        super().__init__()
        self.emb_layers = nn.Sequential(nn.SiLU(), nn.Linear(d, 2 * d))
        self.norm = nn.LayerNorm(d)
        self.out_layers = nn.Sequential(nn.SiLU(), nn.Dropout(p=dropout), nn.Linear(d, d))


class _Layer(nn.Module):
    """Parameter container mirroring TransformerDecoderLayer2Att.__init__ (cross_attention.py:444-489)."""

    def __init__(self, d, nhead, ff, dropout):
        super().__init__()
        self.self_attn = nn.MultiheadAttention(d, nhead, dropout=dropout)
        self.time_block1 = _TimeBlock(d, dropout)
        for m in _MHA_DECL_ORDER:
            setattr(self, "multihead_attn_" + m, nn.MultiheadAttention(d, 1, dropout=dropout))
        self.att_fuser = nn.Linear(d * 5, d)
        self.time_block2 = _TimeBlock(d, dropout)
        self.linear1 = nn.Linear(d, ff)
        self.linear2 = nn.Linear(ff, d)
        self.norm1 = nn.LayerNorm(d)
        self.norm2 = nn.LayerNorm(d)
        self.norm3 = nn.LayerNorm(d)
        for m in ("spkemb", "alsn", "tlsn", "apb", "lsnemb"):
            setattr(self, m + "_norm", nn.LayerNorm(d))


class _Decoder(nn.Module):
    def __init__(self, layer, num_layers, d):
        super().__init__()
        self.layers = nn.ModuleList([copy.deepcopy(layer) for _ in range(num_layers)])  # _get_clones, :687-688
        self.norm = nn.LayerNorm(d)


class Denoiser(nn.Module):

    def __init__(self,
                 ablation,
                 nfeats: int = 263,
                 condition: str = "text",
                 latent_dim: list = [1, 256],
                 ff_size: int = 1024,
                 num_layers: int = 6,
                 num_heads: int = 4,
                 dropout: float = 0.1,
                 normalize_before: bool = False,
                 activation: str = "gelu",
                 flip_sin_to_cos: bool = True,
                 return_intermediate_dec: bool = False,
                 position_embedding: str = "learned",
                 arch: str = "trans_enc",
                 freq_shift: int = 0,
                 guidance_scale: float = 7.5,
                 guidance_uncondp: float = 0.1,
                 text_encoded_dim: int = 768,
                 audio_encoded_dim: int = 512,
                 nclasses: int = 10,
                 **kwargs) -> None:
        super().__init__()
        self.latent_dim = latent_dim[-1]
        self.text_encoded_dim = text_encoded_dim
        self.audio_encoded_dim = audio_encoded_dim
        self.condition = condition
        self.arch = arch
        self.pe_type = ablation.DIFF_PE_TYPE
        self.causal_attn = ablation.CAUSAL_ATTN
        self.num_layers = num_layers
        # the configurations the HIP path implements (everything configs/modules/denoiser.yaml selects)
        if condition not in ("text+audio", "textaudio_uncond"):
            raise TypeError(f"condition type {condition} not supported")            # denoiser.py:113
        if self.pe_type != "convofusion":
            raise ValueError("Not Support PE type")                                   # :123
        if arch != "trans_dec":
            raise ValueError(f"Not supported architechure{arch}!")                    # :171 (trans_enc: VAE-only)
        if ablation.VAE_TYPE == "no":
            raise ValueError("diffusion-only (no VAE) mode is not implemented by the HIP path")
        if not normalize_before or activation != "gelu" or position_embedding not in ("sine", "v2") \
                or return_intermediate_dec or self.causal_attn or not flip_sin_to_cos or freq_shift != 0:
            raise ValueError("the HIP denoiser implements the shipped configuration only "
                             "(pre-norm, gelu, sine PE, flip_sin_to_cos, freq_shift 0, no causal mask)")
        d = text_encoded_dim
        self.latent_embd = nn.Linear(latent_dim[-1], d)
        self.latent_proj = nn.Linear(d, latent_dim[-1])
        self.time_embedding = _TimestepEmbedding(d, d)
        self.query_pos = _PE(d)
        self.mem_pos = _PE(d)
        self.bh_embedding = nn.Embedding(2, d)
        self.condition_embedding = nn.Embedding(5, d)
        self.cond_params = nn.Parameter(1 / 5 * torch.ones(5))
        self.decoder = _Decoder(_Layer(d, num_heads, ff_size, dropout), num_layers, d)
        self._cfg = dict(num_layers=num_layers, latent_dim=latent_dim[-1], d_model=d, ff_size=ff_size, num_heads=num_heads)
        self.return_attention = True   # set False to skip materialising att_mats (returns [])
        # Consecutive forwards that pass the SAME conditioning tensor objects at the same version counters reuse the memories'
        # timestep-independent projections (cfd_forward_same_memories).  A write that torch's version counter does not see (``t.data.copy_()``,
        # DLPack / raw-pointer writes by other libraries) is invisible to that test: set this to False if the caller does such writes between
        # forwards, or verify_constant_memories = True (env CFD_VERIFY_MEMORIES=1) to have every reuse checked against a device checksum
        # (one small reduction per tensor and one host read per forward) and refused with a RuntimeError when the contents moved.
        self.assume_constant_memories = True
        self.verify_constant_memories = os.environ.get("CFD_VERIFY_MEMORIES", "0") not in ("", "0")
        self._main = dict(handle=None, device=None, version=-1, mem_len=0)
        self._side = dict(handle=None, device=None, version=-1, mem_len=0)
        self._version = 0          # bumped whenever the parameters may have changed: engines re-upload lazily
        self.register_load_state_dict_post_hook(lambda module, incompatible: module._mark_dirty())

    # ---- engine management ---------------------------------------------------------------------
    def _mark_dirty(self):
        self._version += 1

    def _apply(self, fn, *a, **kw):
        self._version = getattr(self, "_version", 0) + 1
        return super()._apply(fn, *a, **kw)

    def __del__(self):
        try:
            for st in (self._main, self._side):
                if st["handle"] is not None:
                    _lib.load().cfd_destroy(st["handle"])
        except Exception:
            pass

    def engine(self, device=None, mem_len=0, side=False):
        """The libcfdenoise handle with the current weights uploaded (re-uploaded after
        load_state_dict / .to()).  ``mem_len``: longest memory the call will pass; the closed-form
        memory PE is extended past the checkpoint's 1024 rows when needed (SURVEY.md fact 4 -- the
        reference itself raises for S > 1024).  ``side=True``: a second handle with the same weights for forwards
        issued while a sampling run is open on the first (the run owns its handle's workspace and captured graph)."""
        device = torch.device(device) if device is not None else self.latent_embd.weight.device
        if device.type != "cuda":
            raise RuntimeError("convofusion_amd.Denoiser runs on an MI355X only (move the module to 'cuda'); "
                               "there is no CPU fallback")
        lib = _lib.load()
        idx = device.index if device.index is not None else torch.cuda.current_device()
        st = self._side if side else self._main
        if st["handle"] is None or st["device"] != idx:
            if st["handle"] is not None:
                lib.cfd_destroy(st["handle"])
            st["handle"] = _lib.create_handle(idx, **self._cfg)
            st["device"] = idx
            st["version"] = -1
        if st["version"] != self._version or mem_len > st["mem_len"]:
            sd = self.state_dict()
            need = max(mem_len, sd["mem_pos.pe"].shape[0])
            for name, t in sd.items():
                if name == "mem_pos.pe" and need > t.shape[0]:
                    # keep the checkpoint's rows bit for bit (they are what the reference adds; a re-computed
                    # table can differ from a loaded buffer in the last bit) and append the closed form
                    ext = sine_pe(need, self.text_encoded_dim).to(t.device, t.dtype)
                    t = torch.cat([t, ext[t.shape[0]:]], dim=0)
                t = t.detach().to(torch.float32).contiguous()
                _lib.check(lib.cfd_load_tensor(st["handle"], name.encode(), C.c_void_p(t.data_ptr()), t.numel(),
                                               1 if t.is_cuda else 0))
            _lib.check(lib.cfd_finalize_weights(st["handle"]))
            tab = sinusoid_table(1000, self.text_encoded_dim)
            _lib.check(lib.cfd_set_timestep_table(st["handle"], C.c_void_p(tab.data_ptr()), tab.shape[0]))
            st["version"] = self._version
            st["mem_len"] = need
        return st["handle"]

    @property
    def _handle(self):
        return self._main["handle"]

    # ---- conditioning helpers ------------------------------------------------------------------
    @staticmethod
    def pack_memories(encoder_hidden_states, mem_mask_dict, row_maps=None):
        """Build the cfd_memory array.  Returns (array, keepalive list)."""
        keep = []
        arr = (_lib.Memory * _lib.NUM_MEM)()
        if len(encoder_hidden_states) != _lib.NUM_MEM:
            raise ValueError("encoder_hidden_states must be the 5-tuple (spk_emb, alsn, tlsn, apb, lsnemb)")
        for j, name in enumerate(MEM_NAMES):
            m = encoder_hidden_states[j]
            if m.dim() != 3 or m.shape[-1] != 512:
                raise ValueError(f"memory {name}: expected [rows, S, 512], got {tuple(m.shape)}")
            m = m.detach().to(torch.float32).contiguous()
            keep.append(m)
            mask = (mem_mask_dict or {}).get(name)
            mp = None
            if mask is not None:
                # A bool mask is read in place (same bytes as uint8): no copy, and its address -- part of what the gradient engine compares
                # before it reuses a memory side (rt_grad.hpp, append_memories) -- is the caller's tensor's, not a temporary's that the
                # caching allocator may or may not hand out again on the next call.
                mask = mask.to(device=m.device).contiguous()
                mask = mask.view(torch.uint8) if mask.dtype == torch.bool else mask.to(torch.uint8)
                if tuple(mask.shape) != (m.shape[0], m.shape[1]):
                    raise ValueError(f"key padding mask of {name}: expected {(m.shape[0], m.shape[1])}, got {tuple(mask.shape)}")
                keep.append(mask)
                mp = mask.data_ptr()
            rm = None
            if row_maps is not None and row_maps[j] is not None:
                r = row_maps[j].to(device=m.device, dtype=torch.int32).contiguous()
                keep.append(r)
                rm = r.data_ptr()
            arr[j] = _lib.Memory(m.data_ptr(), rm, mp, m.shape[0], m.shape[1])
        return arr, keep

    # ---- the vector-Jacobian product ---------------------------------------------------------------
    def _vjp_call(self, sample, timestep, encoder_hidden_states, mem_mask_dict, d_out, wrt, row_maps, side_engine, want_out, want_grad, what):
        """(out or None, grad or None, {name: d_mem}) of one forward: one ``cfd_denoise_vjp`` call (``wrt`` empty) or one
        ``cfd_denoise_vjp_mem`` call, the body of ``vjp``, ``vjp_memories`` and the backward of the differentiable ``forward``.
        ``what``: the phrase of the refusal ("its sample" ...)."""
        Be, L, _ = sample.shape
        _require_row_tile(sample, encoder_hidden_states, what)
        lib = _lib.load()
        h = self.engine(sample.device, mem_len=max(int(m.shape[1]) for m in encoder_hidden_states), side=bool(side_engine))
        x = sample.detach().to(torch.float32).contiguous()
        d = d_out.detach().to(device=x.device, dtype=torch.float32).contiguous()
        if tuple(d.shape) != tuple(x.shape):
            raise ValueError(f"d_out must have the sample's shape {list(x.shape)}")
        mems, keep = self.pack_memories(encoder_hidden_states, mem_mask_dict, row_maps)
        a = _lib.VjpArgs()
        a.Be, a.L, a.timestep, a.sample, a.mem = Be, L, int(timestep), x.data_ptr(), mems
        out = torch.empty_like(x) if want_out else None
        grad = torch.empty_like(x) if want_grad else None
        d_mem = {name: torch.empty(tuple(encoder_hidden_states[j].shape), dtype=torch.float32, device=x.device)
                 for j, name in enumerate(MEM_NAMES) if name in wrt}
        ptr = lambda t: None if t is None else C.c_void_p(t.data_ptr())
        with torch.cuda.device(x.device):
            stream = C.c_void_p(torch.cuda.current_stream(x.device).cuda_stream)
            if wrt:
                ptrs = (C.c_void_p * _lib.NUM_MEM)(*(d_mem[name].data_ptr() if name in d_mem else None for name in MEM_NAMES))
                _lib.check(lib.cfd_denoise_vjp_mem(h, C.byref(a), ptr(d), ptr(out), ptr(grad), ptrs, stream))
            else:
                _lib.check(lib.cfd_denoise_vjp(h, C.byref(a), ptr(d), ptr(out), ptr(grad), stream))
        del keep
        return out, grad, d_mem

    def vjp(self, sample, timestep, encoder_hidden_states, mem_mask_dict, d_out, *, row_maps=None, side_engine=False, want_out=True):
        """(out or None, d_out^T . d(out)/d(sample)) of one forward: the direct ``cfd_denoise_vjp`` call (the backward of the
        differentiable ``forward``).  ``row_maps``: as in ``pack_memories`` -- distinct memories with one int32 map [Be] each."""
        return self._vjp_call(sample, timestep, encoder_hidden_states, mem_mask_dict, d_out, (), row_maps, side_engine, want_out, True, "its sample")[:2]

    def vjp_memories(self, sample, timestep, encoder_hidden_states, mem_mask_dict, d_out, *, wrt=MEM_NAMES, row_maps=None, side_engine=False,
                     want_out=True, want_grad=True):
        """(out or None, grad, {name: d_out^T . d(out)/d(memory) [U_j, S_j, 512]}) of one forward: the direct ``cfd_denoise_vjp_mem``
        call.  ``wrt``: the memories whose gradient is wanted (names of ``MEM_NAMES``; none: the ``cfd_denoise_vjp`` call).  ``row_maps``
        as in ``pack_memories``: a distinct memory receives the SUM over the batch rows that map to it, one that no row maps to exact
        zeros; masked keys receive exact zeros.  ``grad`` is the sample's gradient as ``vjp`` returns it (bit for bit), or None with
        ``want_grad=False`` (at least one memory must then be wanted)."""
        wrt = tuple(wrt)
        for name in wrt:
            if name not in MEM_NAMES:
                raise ValueError(f"wrt names a memory that does not exist: {name!r} (the memories are {', '.join(MEM_NAMES)})")
        if not wrt and not want_grad:
            raise ValueError("vjp_memories: nothing is wanted (wrt is empty and want_grad is False)")
        if len(encoder_hidden_states) != _lib.NUM_MEM:
            raise ValueError("encoder_hidden_states must be the 5-tuple (spk_emb, alsn, tlsn, apb, lsnemb)")
        return self._vjp_call(sample, timestep, encoder_hidden_states, mem_mask_dict, d_out, wrt, row_maps, side_engine, want_out, want_grad,
                              "its memories")

    # ---- the key-pose guided update -------------------------------------------------------------------
    def guide(self, x, timestep, encoder_hidden_states, mem_mask_dict, w, target, mask, *, sqrt_acp, sqrt_1m_acp, step, inv_n=None,
              tie=None, csr=None, row_maps=None, side_engine=False, reuse_memory_side=0, want=("loss", "grad", "x_new"), x_new=None):
        """One ``cfd_denoise_guide`` call: (loss, grad, x_new, d_out), None for what ``want`` does not name.  ``x`` [B, L, 128]; the
        memories are those of the n evaluated guidance chunks, chunk-major (n * B rows, or distinct memories with ``row_maps`` as in
        ``vjp``); ``w`` [B, n] the chunk weights (column 0 is not read); ``target`` [B, L, 128] and ``mask`` [B, L] the key poses;
        ``sqrt_acp`` / ``sqrt_1m_acp`` from the scheduler's float64 table; ``inv_n`` 1 / (kept tokens * 128) (None: from ``mask``, one
        host read); ``tie`` [B, L] int32 with ``csr`` = ``tie_csr(tie)`` (None: built here).  ``x_new``: a tensor to write the update
        into (it may be ``x``).  ``reuse_memory_side`` 2: the conditioning is the previous guide call's, the timestep may differ."""
        B, L, _ = x.shape
        n = int(w.shape[1])
        why = guide_refusal(n * B, L, [int(m.shape[1]) for m in encoder_hidden_states])
        if why is not None:
            raise NotImplementedError(f"Denoiser.guide runs on the row-tile path: {why}")
        dev = x.device
        tg, mk = self._guide_operand(target, (B, L, 128), "target", dev), self._guide_operand(mask, (B, L), "mask", dev)
        if inv_n is None:
            kept = int((mk != 0).sum().item())
            if kept == 0:
                raise ValueError("Denoiser.guide: mask keeps no token")
            inv_n = 1.0 / (kept * 128)

        def latent_loss(a):
            a.target, a.mask, a.inv_n = tg.data_ptr(), mk.data_ptr(), float(inv_n)
            return None, None
        return self._guide_call(x, timestep, encoder_hidden_states, mem_mask_dict, w, latent_loss, ("loss", "grad", "x_new", "d_out"), sqrt_acp,
                                sqrt_1m_acp, step, tie, csr, row_maps, side_engine, reuse_memory_side, want, x_new)[:4]

    def guide_pose(self, x, timestep, encoder_hidden_states, mem_mask_dict, w, vae, target, frame_mask, *, feature_mask=None, lengths=None,
                   sqrt_acp, sqrt_1m_acp, step, inv_n=None, tie=None, csr=None, row_maps=None, side_engine=False, reuse_memory_side=0,
                   want=("loss", "grad", "x_new"), x_new=None):
        """One ``cfd_denoise_guide_pose`` call: ``guide`` with the loss of ``edit.pose_keyframe_loss`` -- the mean-square error of
        ``vae.decode(loop_to_vae(x0), lengths)`` against ``target`` [B, F, 189] over the frames of ``frame_mask`` [B, F] and the features
        of ``feature_mask`` [189] (None: all) -- decoded and swept on the same handle, in the same call.  Returns (loss, grad, x_new,
        d_out, feats), None for what ``want`` does not name (``feats`` [B, F, 189]: the decode of the predicted clean latents).
        ``vae``: a ``convofusion_amd.vae.ConvoFusionVae`` (its packed decoder weights are read; its own ``decode`` handle is not used).
        ``lengths``: frames per row (default F; each in [1, F]).  ``inv_n`` 1 / (selected frames * selected features) (None: from the
        masks, one host read).  Everything else as in ``guide``; memory packing, row maps and the tie are that call's."""
        B, L, _ = x.shape
        n = int(w.shape[1])
        if not isinstance(target, torch.Tensor) or target.dim() != 3 or target.shape[0] != B:
            raise ValueError(f"Denoiser.guide_pose: target must be a tensor [{B}, F, nfeats]")
        F, nf = int(target.shape[1]), int(target.shape[2])
        why = guide_pose_refusal(n * B, L, [int(m.shape[1]) for m in encoder_hidden_states], B, F, latent_dim=vae.latent_dim,
                                 num_heads=vae.num_heads, ff_size=vae.ff_size, num_layers=vae.num_layers, latent_size=vae.latent_size)
        if why is not None:
            raise NotImplementedError(f"Denoiser.guide_pose: {why}")
        if nf != vae.body_nfeats + vae.hands_nfeats:
            raise ValueError(f"Denoiser.guide_pose: target has {nf} features, the decoder {vae.body_nfeats + vae.hands_nfeats}")
        dev = x.device
        tg, fm = self._guide_operand(target, (B, F, nf), "target", dev), self._guide_operand(frame_mask, (B, F), "frame_mask", dev)
        cm = torch.ones(nf, dtype=torch.float32, device=dev) if feature_mask is None else self._guide_operand(feature_mask, (nf,), "feature_mask", dev)
        lens = torch.full((B,), F, dtype=torch.int32) if lengths is None else torch.as_tensor(lengths).detach().reshape(-1).to("cpu", torch.int32)
        if lens.numel() != B or int(lens.min()) < 1 or int(lens.max()) > F:
            raise ValueError(f"Denoiser.guide_pose: lengths must be {B} values in [1, {F}], got {lens.tolist()}")
        if inv_n is None:
            sel = int((fm != 0).sum().item()) * int((cm != 0).sum().item())
            if sel == 0:
                raise ValueError("Denoiser.guide_pose: the masks select no frame or no feature")
            inv_n = 1.0 / sel
        pack, lens_d = vae._decoder_pack(dev), lens.to(dev).contiguous()

        def pose_loss(a):
            p = _lib.GuidePose(pack.data_ptr(), vae.latent_dim, vae.num_heads, vae.ff_size, vae.num_layers, F, lens_d.data_ptr(), tg.data_ptr(),
                               fm.data_ptr(), cm.data_ptr(), float(inv_n))
            return p, (B, F, nf)
        return self._guide_call(x, timestep, encoder_hidden_states, mem_mask_dict, w, pose_loss, ("loss", "grad", "x_new", "d_out", "feats"),
                                sqrt_acp, sqrt_1m_acp, step, tie, csr, row_maps, side_engine, reuse_memory_side, want, x_new)

    def _guide_call(self, x, timestep, encoder_hidden_states, mem_mask_dict, w, set_loss, wantable, sqrt_acp, sqrt_1m_acp, step, tie, csr,
                    row_maps, side_engine, reuse_memory_side, want, x_new):
        """The body of ``guide`` and ``guide_pose``: operands, memory packing, row maps, tie and results are one code path;
        ``set_loss(args)`` fills the latent loss into the cfd_guide_args or returns (cfd_guide_pose, feats' shape) for the pose call.
        Returns (loss, grad, x_new, d_out, feats)."""
        B, L, _ = x.shape
        n = int(w.shape[1])
        unknown = set(want) - set(wantable)
        if unknown or not want:
            raise ValueError(f"want names {sorted(unknown)}: it is a non-empty subset of {', '.join(wantable)}")
        lib = _lib.load()
        dev = x.device
        h = self.engine(dev, mem_len=max(int(m.shape[1]) for m in encoder_hidden_states), side=bool(side_engine))
        xs, ws = self._guide_operand(x, (B, L, 128), "x", dev), self._guide_operand(w, (B, n), "w", dev)
        a = _lib.GuideArgs()
        mems, keep = self.pack_memories(encoder_hidden_states, mem_mask_dict, row_maps)
        a.B, a.L, a.n, a.timestep, a.sqrt_acp, a.sqrt_1m_acp = B, L, n, int(timestep), float(sqrt_acp), float(sqrt_1m_acp)
        a.x, a.mem, a.w = xs.data_ptr(), mems, ws.data_ptr()
        a.step, a.reuse_memory_side = float(step), int(reuse_memory_side)
        pose, feats_shape = set_loss(a)
        if tie is not None:
            tt = tie.detach().to(device=dev, dtype=torch.int32).contiguous()
            if tuple(tt.shape) != (B, L):
                raise ValueError(f"tie must be [B, L] = [{B}, {L}], not {list(tt.shape)}")
            cs = (tie_csr(tt) if csr is None else csr).to(device=dev, dtype=torch.int32).contiguous()
            if cs.numel() != 2 * B * L + 1:
                raise ValueError(f"csr must have 2 B L + 1 = {2 * B * L + 1} entries (tie_csr), not {cs.numel()}")
            keep += [tt, cs]
            a.tie, a.tie_csr = tt.data_ptr(), cs.data_ptr()
        loss = torch.empty((), dtype=torch.float32, device=dev) if "loss" in want else None
        grad = torch.empty_like(xs) if "grad" in want else None
        d_out = torch.empty((n * B, L, 128), dtype=torch.float32, device=dev) if "d_out" in want else None
        feats = torch.empty(feats_shape, dtype=torch.float32, device=dev) if "feats" in want else None
        given = x_new is not None and "x_new" in want
        if "x_new" in want:
            if x_new is None:
                x_new = torch.empty_like(xs)
            elif x_new.dtype != torch.float32 or not x_new.is_contiguous() or tuple(x_new.shape) != (B, L, 128) or x_new.device != dev:
                raise ValueError(f"x_new must be a contiguous float32 tensor [{B}, {L}, 128] on {dev}")
        else:
            x_new = None
        ptr = lambda t: None if t is None else C.c_void_p(t.data_ptr())
        with torch.cuda.device(dev):
            stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
            if pose is None:
                _lib.check(lib.cfd_denoise_guide(h, C.byref(a), ptr(loss), ptr(grad), ptr(x_new), ptr(d_out), stream))
            else:
                _lib.check(lib.cfd_denoise_guide_pose(h, C.byref(a), C.byref(pose), ptr(loss), ptr(grad), ptr(x_new), ptr(d_out), ptr(feats), stream))
        if given and not x_new.is_inference():      # (a ctypes write into the caller's tensor: see ``_lib.wrote``)
            _lib.wrote(x_new)
        del keep
        return loss, grad, x_new, d_out, feats

    @staticmethod
    def _guide_operand(t, shape, name, dev):
        if not isinstance(t, torch.Tensor) or tuple(t.shape) != tuple(shape):
            raise ValueError(f"Denoiser.guide: {name} must be a tensor {list(shape)}")
        return t.detach().to(device=dev, dtype=torch.float32).contiguous()

    # ---- forward -------------------------------------------------------------------------------
    @staticmethod
    def _refuse_grad(sample, timestep, encoder_hidden_states, mem_mask_dict, what):
        """Every refusal the two differentiable forward modes share, before any device work.  ``what``: "its sample" ..."""
        for name, m in (mem_mask_dict or {}).items():
            if m is not None and m.requires_grad:
                raise NotImplementedError(f"the HIP denoiser has no gradient with respect to a key-padding mask ({name} requires grad)")
        if torch.as_tensor(timestep).numel() != 1:
            raise NotImplementedError(f"the gradient of the HIP denoiser with respect to {what} needs one timestep for all rows "
                                      "(a per-row timestep vector is not on the row-tile path)")
        _require_row_tile(sample, encoder_hidden_states, what)

    def forward(self, sample, timestep, encoder_hidden_states, lengths=None, mem_mask_dict=dict(), **kwargs):
        """``kwargs['side_engine']=True`` (extension): run on the second handle, for calls made while a sampling run is
        open on the first; ``kwargs['memory_grad']=True`` (extension): memories that require grad receive gradients too (differentiable
        when grad is enabled and the sample or any memory requires grad); every other keyword (``return_dict`` ...) is ignored like the
        reference does.
        Under grad mode with ``sample.requires_grad`` the output is differentiable with respect to ``sample`` (module docstring)."""
        if sample.dim() != 3 or sample.shape[-1] != self.latent_dim:
            raise ValueError(f"sample must be [batch, tokens, {self.latent_dim}]")
        memory_grad = bool(kwargs.get("memory_grad", False))
        if memory_grad and len(encoder_hidden_states) != _lib.NUM_MEM:
            raise ValueError("encoder_hidden_states must be the 5-tuple (spk_emb, alsn, tlsn, apb, lsnemb)")
        if not (torch.is_grad_enabled() and (sample.requires_grad or (memory_grad and any(m.requires_grad for m in encoder_hidden_states)))):
            return self._forward_hip(sample, timestep, encoder_hidden_states, mem_mask_dict, kwargs)
        for name, m in zip(MEM_NAMES, encoder_hidden_states):
            if not memory_grad and m.requires_grad:
                raise NotImplementedError(f"the HIP denoiser has no gradient with respect to its memories ({name} requires grad): detach it")
            if memory_grad and (m.dim() != 3 or m.shape[0] != sample.shape[0]):
                raise ValueError(f"memory_grad=True takes one memory per batch row: {name} has shape {list(m.shape)} for {sample.shape[0]} rows")
        self._refuse_grad(sample, timestep, encoder_hidden_states, mem_mask_dict, "its sample and memories" if memory_grad else "its sample")
        out, *att = _DenoiseVjp.apply(self, timestep, mem_mask_dict, kwargs, memory_grad, sample, *encoder_hidden_states)
        return (out, list(att))

    def _forward_hip(self, sample, timestep, encoder_hidden_states, mem_mask_dict, kwargs):
        """The inference path: one cfd_forward."""
        lib = _lib.load()
        Be, L, _ = sample.shape
        h = self.engine(sample.device, mem_len=max(int(m.shape[1]) for m in encoder_hidden_states), side=bool(kwargs.get("side_engine", False)))
        x = sample.detach().to(torch.float32).contiguous()
        t = torch.as_tensor(timestep)
        if t.numel() == 1:
            ts = [int(t.reshape(-1)[0].item())]
        elif t.numel() == Be:
            ts = [int(v) for v in t.reshape(-1).tolist()]
        else:
            raise ValueError("timestep must be a scalar or have one entry per batch row")
        ts_arr = (C.c_int32 * len(ts))(*ts)
        mems, keep = self.pack_memories(encoder_hidden_states, mem_mask_dict)
        out = torch.empty_like(x)
        att_ptrs = (C.c_void_p * _lib.NUM_MEM)()
        att = []
        if self.return_attention:
            for j in range(_lib.NUM_MEM):
                a = torch.empty((Be, self.num_layers, L, int(encoder_hidden_states[j].shape[1])), dtype=torch.float32, device=x.device)
                att.append(a)
                att_ptrs[j] = a.data_ptr()
        stream = torch.cuda.current_stream(x.device).cuda_stream
        # The reference's own loop (no convofusion_amd.install) calls this once per iteration with the SAME conditioning tensors
        # (convofusion.py:499-513): the same tensor objects with the same contents as in the previous call on this handle (the previous
        # call's tensors are kept alive here, so an address cannot come back with other data), and the library then reuses their
        # timestep-independent projections (cfd_forward_same_memories; it checks shapes, weights and what ran in between).
        srcs = list(encoder_hidden_states) + [(mem_mask_dict or {}).get(name) for name in MEM_NAMES]
        same, sig = False, None
        if self.assume_constant_memories:
            last = getattr(self, "_last_forward_memories", None)
            sig = _contents_signature(srcs, force_checksum=self.verify_constant_memories)
            same = last is not None and last[0] == h and len(last[1]) == len(srcs) and all(a is b for a, b in zip(last[1], srcs))
            # (a refusal needs checksums on BOTH sides: the call before verify_constant_memories was switched on recorded none -- then the
            #  signatures merely differ and the projections are made again)
            both = same and all((a[1] is None) == (b[1] is None) for a, b in zip(last[2], sig))
            if same and both and self.verify_constant_memories and [v for v, _ in last[2]] == [v for v, _ in sig] and last[2] != sig:
                self._last_forward_memories = None
                raise RuntimeError("convofusion_amd.Denoiser: a conditioning tensor was rewritten between two forwards without moving its version "
                                   "counter (t.data.copy_(), a DLPack / raw-pointer write): the reuse of its projections would be stale; bump it with "
                                   "torch.autograd.graph.increment_version(t) or set denoiser.assume_constant_memories = False")
            same = same and last[2] == sig
        self._last_forward_memories = None
        self.last_forward_reused = bool(same)     # (diagnostic: whether this call promised the library the previous call's memories)
        with torch.cuda.device(x.device):
            if same:
                _lib.check(lib.cfd_forward_same_memories(h))
            _lib.check(lib.cfd_forward(h, C.c_void_p(x.data_ptr()), Be, L, ts_arr, len(ts), mems, C.c_void_p(out.data_ptr()),
                                       att_ptrs if self.return_attention else None, C.c_void_p(stream)))
        if sig is not None:
            self._last_forward_memories = (h, srcs, sig)
        return (out, att)
