"""CPU (-m "not gpu"): the float64 restatement of the decoder's reverse sweep (tests/vae_vjp_ref.py) against the reference's autograd
gradient and against finite differences; the C ABI of cfd_vae_decode_vjp; the decoder pack; every refusal of ``decode_vjp`` and
``pose_keyframe_loss``."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from oracle import vae_weights
from tests import vae_vjp_ref as R
from tests.helpers import load_golden
from tests.test_oracle_vae import ABL, KW

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _model():
    import torch
    from convofusion_amd.vae import ConvoFusionVae
    m = ConvoFusionVae(ablation=ABL, **KW)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in vae_weights.make_state_dict().items()}, strict=True)
    return m.eval()


@pytest.mark.parametrize("name", list(R.CASES))
def test_restatement_matches_the_reference_autograd_gradient(name):
    """relative L2 < 1e-3: the project's bar against the reference's autograd (tests/golden/vjp.npz)."""
    g = load_golden("vae_decode_vjp")
    z, lens, d = R.case_inputs(name)
    feats, d_z, taps = R.decode_vjp(vae_weights.make_state_dict(), z, lens, d)
    rel, row = R.errors(d_z, g[name + ".grad"])
    print(f"{name}: float64 restatement vs float64 autograd: rel L2 {rel:.2e}, worst row {row:.2e}; yardstick {g[name + '.yard']}")
    assert d_z.shape == z.shape and rel < 1e-3
    assert 0 < g[name + ".yard"][0] < 1e-4 and 0 < g[name + ".yard"][1] < 1e-4          # float32 autograd is a float32 distance away
    for b, n in enumerate(lens):
        assert not feats[b, n:].any()
    assert set(taps) >= {f"{k}.{s}.{l}" for k in ("g", "dz", "x") for s in range(2) for l in range(5)}


@pytest.mark.parametrize("name", ["tiny", "single"])
def test_restatement_matches_central_finite_differences(name):
    """<c, J v> along three seeded directions v, central difference of the float64 forward against <d_z, v>."""
    sd = vae_weights.make_state_dict()
    z, lens, d = R.case_inputs(name)
    _, state, _ = R.decode_forward(sd, z, lens)
    d_z = R.decode_sweep(state, d)
    d64 = d.astype(np.float64)
    for b, n in enumerate(lens):
        d64[b, n:] = 0
    rng = np.random.Generator(np.random.PCG64(515))
    for _ in range(3):
        v = rng.standard_normal(z.shape)
        h = 1e-5
        fp = R.decode_forward(sd, z.astype(np.float64) + h * v, lens)[0]
        fm = R.decode_forward(sd, z.astype(np.float64) - h * v, lens)[0]
        fd = float(((fp - fm) * d64).sum() / (2 * h))
        an = float((d_z * v).sum())
        print(f"{name}: finite difference {fd:.10e} sweep {an:.10e}")
        assert abs(fd - an) <= 1e-6 * max(abs(fd), abs(an))          # h^2 truncation + 1e-16 / h rounding of a float64 forward


def test_struct_mirror_matches_the_header():
    from convofusion_amd import _lib
    A = _lib.VaeDecodeVjpArgs
    assert C.sizeof(A) == 64
    assert [(n, getattr(A, n).offset) for n, _ in A._fields_] == [
        ("wpack", 0), ("d_model", 8), ("num_heads", 12), ("ff_size", 16), ("num_layers", 20), ("bs", 24), ("nframes", 28), ("n_chunks", 32),
        ("z", 40), ("lengths", 48), ("d_feats", 56)]
    header = open(os.path.join(ROOT, "include", "cfdenoise.h")).read()
    body = re.search(r"typedef struct \{([^}]*)\} cfd_vae_decode_vjp_args;", header).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            names += [v.strip().lstrip("*").strip() for v in re.sub(r"^(const\s+)?\w+\s*\*?", "", decl, count=1).split(",")]
    assert names == [n for n, _ in A._fields_]
    assert "int cfd_vae_decode_vjp(cfd_handle h, const cfd_vae_decode_vjp_args* a, float* feats, float* d_z, void* stream);" in header
    assert "vae.py:268-372" in header and "cross_attention.py:66-125" in header


def test_symbol_is_exported():
    from convofusion_amd import _lib
    assert "cfd_vae_decode_vjp" in _lib.SYMBOLS
    lib = _lib.load()
    assert lib.cfd_vae_decode_vjp.restype is C.c_int and len(lib.cfd_vae_decode_vjp.argtypes) == 5


def _unpack(p, n, k):
    """Inverse of ``_pack_w``: the packed floats of a [n][k] matrix -> the matrix."""
    return p.reshape(n // 16, k // 16, 4, 16, 4).permute(0, 3, 1, 2, 4).reshape(n, k)


def test_decoder_pack_length_and_round_trip():
    import torch
    from convofusion_amd import vae as V
    m = _model()
    pack = m._decoder_pack(torch.device("cpu"))
    assert pack.numel() == V.decoder_pack_floats(m.num_layers) == 8257536 and pack.dtype == torch.float32
    assert m._decoder_pack(torch.device("cpu")) is pack                        # kept ...
    # hands stack, layer 3 (output block 0), linear1.weight in both orders: offsets of csrc/vae_dec.hpp
    d, ff = 128, 1024
    layer = 6 * d + 2 * (2 * 3 * d * d + 3 * d) + 2 * (2 * d * d + d) + 2 * (2 * d * ff) + ff + d
    stack = m.num_layers * layer + 2 * (4 * d * d + d) + 2 * d + 2 * d * d + d
    w1 = stack + 3 * layer + 6 * d + 2 * (2 * 3 * d * d + 3 * d) + 2 * (2 * d * d + d)
    W = m.hands_decoder.output_blocks[0].linear1.weight.detach()
    assert torch.equal(_unpack(pack[w1:w1 + ff * d], ff, d), W)
    assert torch.equal(_unpack(pack[w1 + ff * d:w1 + 2 * ff * d], d, ff), W.t())
    assert torch.equal(pack[w1 + 2 * ff * d:w1 + 2 * ff * d + ff], m.hands_decoder.output_blocks[0].linear1.bias.detach())
    # the padded final layer and the PE tables at the end
    fw = 2 * stack - (2 * d * d + d)
    assert torch.equal(_unpack(pack[fw:fw + d * d], d, d)[:120], m.hands_final_layer.weight.detach())
    assert not _unpack(pack[fw:fw + d * d], d, d)[120:].any()
    assert torch.equal(pack[2 * stack:2 * stack + 256 * d], m.query_pos_decoder.pe[:256].reshape(-1))
    with torch.no_grad():
        m.body_decoder.norm.weight.mul_(2.0)
    assert m._decoder_pack(torch.device("cpu")) is not pack                    # ... until a parameter changes


def test_decode_vjp_refusals():
    import torch
    from convofusion_amd.vae import decode_vjp_refusal
    m = _model()
    z, d = torch.zeros(2, 2, 8, 128), torch.zeros(2, 128, 189)
    with pytest.raises(ValueError, match="at least 1"):
        m.decode_vjp(z, [128, 0], d)
    with pytest.raises(ValueError, match="z must be"):
        m.decode_vjp(z[0], [128, 128], d)
    with pytest.raises(ValueError, match="z must be"):
        m.decode_vjp(torch.zeros(2, 2, 8, 64), [128, 128], d)
    with pytest.raises(ValueError, match="lengths"):
        m.decode_vjp(z, [128], d)
    with pytest.raises(ValueError, match="d_feats must be"):
        m.decode_vjp(z, [128, 128], d[..., :100])
    with pytest.raises(ValueError, match="d_feats must be"):
        m.decode_vjp(z, [128, 128], d[:1])
    with pytest.raises(ValueError, match="must equal"):
        m.decode_vjp(z, [128, 100], torch.zeros(2, 144, 189))
    with pytest.raises(NotImplementedError, match="256 frames"):
        m.decode_vjp(z, [272, 100], torch.zeros(2, 272, 189))
    with pytest.raises(NotImplementedError, match="16 latent chunks"):
        m.decode_vjp(torch.zeros(2, 2, 17, 128), [128, 128], d)
    with pytest.raises(NotImplementedError, match="65535 sequences"):
        m.decode_vjp(torch.zeros(2, 1, 1, 128).expand(2, 65536, 1, 128), [1] * 65536, torch.zeros(1, 1, 189).expand(65536, 1, 189))
    with pytest.raises(RuntimeError, match="MI355X only"):
        m.decode_vjp(z, [128, 128], d)                                         # a CPU tensor: decode's own error
    with pytest.raises(RuntimeError, match="MI355X only"):
        m.decode(z, [128, 128])
    assert decode_vjp_refusal(1, 256, 16) is None and decode_vjp_refusal(65535, 1, 1) is None and "65535" in decode_vjp_refusal(65536, 1, 1)
    assert "num_layers" in decode_vjp_refusal(1, 128, 8, num_layers=11) and "heads" in decode_vjp_refusal(1, 128, 8, num_heads=4)


def test_pose_keyframe_loss_refusals():
    import torch
    from convofusion_amd.edit import pose_keyframe_loss
    m = _model()
    target, fm = torch.zeros(2, 64, 189), torch.zeros(2, 64, dtype=torch.bool)
    with pytest.raises(ValueError, match="select no frame"):
        pose_keyframe_loss(m, target, fm)
    fm[0, 7] = True
    with pytest.raises(ValueError, match="select no frame or no feature"):
        pose_keyframe_loss(m, target, fm, torch.zeros(189, dtype=torch.bool))
    with pytest.raises(ValueError, match="frame_mask must be"):
        pose_keyframe_loss(m, target, fm[:, :32])
    with pytest.raises(ValueError, match="feature_mask must be"):
        pose_keyframe_loss(m, target, fm, torch.ones(100, dtype=torch.bool))
    with pytest.raises(ValueError, match="target must be"):
        pose_keyframe_loss(m, target[0], fm)
    with pytest.raises(ValueError, match="lengths must be"):
        pose_keyframe_loss(m, target, fm, lengths=[64])
    with pytest.raises(ValueError, match="lengths must be"):
        pose_keyframe_loss(m, target, fm, lengths=[60, 50])
    with pytest.raises(ValueError, match="lengths must be"):
        pose_keyframe_loss(m, target, fm, lengths=[64, 0])
    loss = pose_keyframe_loss(m, target, fm, lengths=[64, 20])
    with pytest.raises(ValueError, match="x0 must be"):
        loss(torch.zeros(3, 8, 128))
    with pytest.raises(RuntimeError, match="MI355X only"):
        loss(torch.zeros(2, 8, 128))                                            # decode has no CPU path
