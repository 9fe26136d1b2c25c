"""Host side of motion editing (no GPU): the token mask's layout, the VAE <-> loop latent permutes against the reference's, the strength ->
first-iteration mapping against diffusers' img2img formula, the argument refusals, the restated edit loop against the oracle loop, and the
ctypes mirror of cfd_edit_args / cfd_sample_begin_edit against the header."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest
import torch

from tests import edit_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_token_mask_layout_and_frame_to_chunk_mapping():
    from convofusion_amd.edit import part_index, token_mask
    assert (part_index("body"), part_index("hands")) == (0, 1)
    m = token_mask(3, keep_parts=("body",))
    assert m.dtype == torch.bool and tuple(m.shape) == (3, 16)
    assert m[:, 0::2].all() and not m[:, 1::2].any()                 # token 2c + p: body at even tokens
    m = token_mask(1, keep_parts="hands")
    assert m[0].tolist() == [False, True] * 8
    assert token_mask(2).all()
    m = token_mask(1, keep_frames=[(0, 32), (96, 128)])[0].reshape(8, 2)
    assert m.all(dim=1).tolist() == [True, True, False, False, False, False, True, True] and (m[:, 0] == m[:, 1]).all()
    for f in range(128):                                              # frame f lies in chunk f // 16
        m = token_mask(1, keep_frames=[(f, f + 1)], keep_parts=("hands",))[0]
        assert m.nonzero().flatten().tolist() == [2 * (f // 16) + 1]
    m = token_mask(1, keep_frames=[(10, 40)])[0].reshape(8, 2)        # a span touching a chunk keeps the whole chunk
    assert m.all(dim=1).tolist() == [True, True, True, False, False, False, False, False]
    assert token_mask(1, keep_frames=[(0, 64)], L=8).all()
    assert not token_mask(1, keep_parts=())[0].any()


@pytest.mark.parametrize("bad", [dict(keep_frames=[(0, 129)]), dict(keep_frames=[(5, 5)]), dict(keep_frames=[(-1, 4)]),
                                 dict(keep_frames=[3]), dict(keep_parts=("arms",)), dict(L=15)])
def test_token_mask_refusals(bad):
    from convofusion_amd.edit import token_mask
    with pytest.raises(ValueError):
        token_mask(2, **bad)


def test_latent_permutes_match_the_reference():
    """vae_to_loop: convofusion.py:725 (permute(1, 2, 0, 3)) + :558 (reshape(bs, t * bh, dim)); loop_to_vae: :548 (permute(1, 0, 2)) +
    :1028-1030 (reshape(ntokens // 2, 2, bs, dim), permute(1, 2, 0, 3)); the two are inverse and token 2c + p is chunk c of stack p."""
    from convofusion_amd.edit import loop_to_vae, vae_to_loop
    z = torch.randn(2, 3, 8, 128)
    bs, t, bh, dim = z.permute(1, 2, 0, 3).shape
    want_loop = z.permute(1, 2, 0, 3).reshape(bs, t * bh, dim)
    lat = vae_to_loop(z)
    assert torch.equal(lat, want_loop)
    zz = lat.permute(1, 0, 2)
    ntokens, b2, d2 = zz.shape
    want_vae = zz.reshape(ntokens // 2, 2, b2, d2).permute(1, 2, 0, 3)
    assert torch.equal(loop_to_vae(lat), want_vae) and torch.equal(loop_to_vae(lat), z)
    for c in range(8):
        for p in range(2):
            assert torch.equal(lat[:, 2 * c + p], z[p, :, c])


def test_latent_parts_follow_the_encoder_pack():
    """LATENT_PARTS[s] is stack s of the packed encoder weights (the kernel's stack index): the body block first."""
    from types import SimpleNamespace
    from convofusion_amd.vae import LATENT_PARTS, ConvoFusionVae
    from tests.test_vae_encode_host import KW
    v = ConvoFusionVae(ablation=SimpleNamespace(PE_TYPE="convofusion", MLP_DIST=False), **KW)
    src = [t for t, _ in v._encoder_sources()]
    half = len(src) // 2
    for s, part in enumerate(LATENT_PARTS):
        assert src[s * half] is getattr(v, f"{part}_skel_embedding").weight


@pytest.mark.parametrize("N", [1, 5, 10, 20, 50, 1000])
def test_strength_to_first_iteration_follows_diffusers_img2img(N):
    from convofusion_amd.sampler import edit_first_iteration
    for strength in (1.0, 0.999, 0.75, 0.7, 0.6, 0.5, 0.3, 0.1, 0.05, 0.01, 1e-3):
        k = min(int(N * strength), N)
        if k == 0:
            with pytest.raises(ValueError):
                edit_first_iteration(strength, N)
            continue
        k0 = edit_first_iteration(strength, N)
        assert k0 == edit_ref.strength_first_iteration(N, strength) == N - k
        assert 0 <= k0 < N
    assert edit_first_iteration(1.0, N) == 0


@pytest.mark.parametrize("strength", [0.0, -0.5, 1.5, math.nan, math.inf, "x", None])
def test_strength_refusals(strength):
    from convofusion_amd.sampler import edit_first_iteration
    with pytest.raises(ValueError):
        edit_first_iteration(strength, 20)


def test_check_edit_refusals():
    from convofusion_amd.sampler import check_edit
    B, L, N = 2, 16, 20
    src = torch.zeros(B, L, 128)
    keep = torch.zeros(B, L, dtype=torch.bool)
    assert check_edit(None, None, 1.0, B, L, N) is None
    s, k, k0 = check_edit(src, keep.to(torch.int64), 0.6, B, L, N)
    assert s.dtype == torch.float32 and k.dtype == torch.uint8 and k0 == 8
    assert check_edit(src.double(), None, 1.0, B, L, N)[1:] == (None, 0)
    bad = [
        dict(source_latents=None, keep_mask=keep),                              # keep_mask without a source
        dict(source_latents=None, strength=0.5),                                # strength < 1 without a source
        dict(preseq=torch.zeros(B, 4, 128)),                                    # preseq with an edit
        dict(source_latents=src[:1]), dict(source_latents=src[..., :64]),       # shapes
        dict(source_latents=src.to(torch.int32)), dict(source_latents=src.numpy()),
        dict(keep_mask=keep[:, :8]), dict(keep_mask=keep.float()), dict(keep_mask=torch.full((B, L), 2, dtype=torch.uint8)), dict(keep_mask=keep.numpy()),
        dict(strength=0.04),                                                    # int(20 * 0.04) == 0 iterations
    ]
    for b in bad:
        kw = dict(source_latents=src, keep_mask=keep, strength=1.0, preseq=None)
        kw.update(b)
        with pytest.raises(ValueError):
            check_edit(kw["source_latents"], kw["keep_mask"], kw["strength"], B, L, N, kw["preseq"])


def _fake_denoiser(seed):
    rng = np.random.default_rng(seed)
    w = rng.standard_normal((128, 128)).astype(np.float32) / 16

    def fn(x, t, enc, masks):
        chunks = np.split(x, 7, axis=0)
        out = np.concatenate([np.tanh(c @ w) * np.float32(1 + 0.1 * k) + np.float32(t / 1000.0) for k, c in enumerate(chunks)])
        return out.astype(np.float32), []
    return fn


@pytest.mark.parametrize("kind", ["ddpm", "dpmpp"])
def test_restated_edit_loop_without_edit_is_the_oracle_loop(kind):
    """edit_ref.edit_reverse with no kept token and k0 = 0 equals oracle.sampler_ref.diffusion_reverse bit for bit (DDPM with step noise;
    DPM-Solver++ through tests/dpmsolver_ref.py's step) on a cheap stand-in denoiser."""
    from oracle import philox_ref, sampler_ref, scheduler_ref
    from tests.dpmsolver_ref import DPMSolverMultistepRef
    B, L, n, seed = 2, 16, 10, 4
    mk = (lambda: DPMSolverMultistepRef(num_train_timesteps=1000, beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear")) \
        if kind == "dpmpp" else scheduler_ref.DDPMSchedulerRef
    init = philox_ref.normal_tensor(seed, 0, range(B), 1, L)
    noise = lambda i, t: philox_ref.normal_tensor(seed, i, range(B), 0, L)   # noqa: E731
    fn = _fake_denoiser(seed)
    want, _, _ = sampler_ref.diffusion_reverse(fn, mk(), None, None, init, noise, num_inference_steps=n)
    got, _ = edit_ref.edit_reverse(fn, mk(), None, None, init, noise, np.ones((B, L, 128), np.float32), np.zeros((B, L), bool), 0,
                                   num_inference_steps=n)
    assert np.array_equal(got, want.transpose(1, 0, 2))


def test_restated_dpmpp_order_counts_executed_steps():
    """diffusers 0.14.0 decides the order from lower_order_nums: from k0 on, the first executed step is first order, the others second
    order, the last one first order again when the FULL table is shorter than 15."""
    for n, k0 in ((10, 3), (10, 0), (20, 6)):
        st = edit_ref.DpmState()
        orders = []
        for i in range(k0, n):
            orders.append(edit_ref.dpmpp_order(st, i, n))
            st.lower_order_nums = min(st.lower_order_nums + 1, 2)
        want = [1] + [2] * (n - k0 - 2) + [1 if n < 15 else 2]
        assert orders == want, (n, k0, orders)


def test_ctypes_mirror_and_header_agree():
    from convofusion_amd import _lib, build
    hdr = open(os.path.join(ROOT, "include", "cfdenoise.h")).read()
    body = re.search(r"typedef struct \{([^}]*)\} cfd_edit_args;", re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)).group(1)
    fields = re.findall(r"(\w+)\s*;", body)
    assert fields == [f for f, _ in _lib.EditArgs._fields_] == ["source", "keep", "first_iteration"]
    E = _lib.EditArgs
    assert (E.source.offset, E.keep.offset, E.first_iteration.offset, C.sizeof(E)) == (0, 8, 16, 24)
    assert "cfd_sample_begin_edit" in _lib.SYMBOLS
    build.build()
    lib = _lib.load()
    fn = lib.cfd_sample_begin_edit
    assert fn.restype is C.c_int
    assert fn.argtypes == [C.c_void_p, C.POINTER(_lib.SampleArgs), C.POINTER(_lib.EditArgs), C.c_void_p, C.c_int, C.POINTER(C.c_int),
                           C.c_void_p]
    assert fn(None, None, None, None, 1, None, None) == -1          # (refused before anything touches a device)
    assert b"null" in lib.cfd_last_error()


def test_sample_sharded_slices_the_edit_per_rank():
    from convofusion_amd.distributed import sample_sharded
    total, L = 5, 16
    src = torch.arange(total, dtype=torch.float32).reshape(total, 1, 1).expand(total, L, 128).contiguous()
    keep = torch.zeros(total, L, dtype=torch.bool)
    keep[3, 4] = True
    seen = {}

    def fn(enc, masks, B, first_utterance, **kw):
        seen.update(kw, B=B, first=first_utterance)
        return kw["source_latents"]

    enc = [torch.zeros(7 * total, 3, 512)] * 5
    out = sample_sharded(fn, enc, {}, total, source_latents=src, keep_mask=keep)
    assert torch.equal(out, src) and torch.equal(seen["keep_mask"], keep) and seen["B"] == total
    with pytest.raises(ValueError):
        sample_sharded(fn, enc, {}, total, source_latents=src[:4])
