"""CPU tests of ConvoFusionVae.encode: the float64 restatement against the golden outputs of the imported reference
(tests/golden/vae_encode.npz, made by tests/golden/make_golden_vae_encode.py), and the mirror's argument checks."""
import os
from types import SimpleNamespace

import numpy as np
import pytest

from oracle import vae_weights
from tests import vae_encode_ref
from tests.vae_encode_ref import RESEED, golden_cases as cases

GE = np.load(os.path.join(os.path.dirname(__file__), "golden", "vae_encode.npz"))
ABL = SimpleNamespace(MLP_DIST=False, PE_TYPE="convofusion")
KW = dict(nfeats=189, latent_dim=[1, 128], ff_size=1024, num_layers=5, num_heads=2, dropout=0.1, arch="encoder_decoder",
          normalize_before=True, activation="gelu", position_embedding="sine")
NAMES = ["ragged", "single", "long", "offset", "reseed"]


def case(name):
    """(state dict, features, lengths) of a golden case"""
    f, lens = cases()["single" if name == "reseed" else name]
    return vae_weights.make_state_dict(**({"seed": RESEED} if name == "reseed" else {})), f, lens


@pytest.mark.parametrize("name", NAMES)
def test_restatement_matches_reference_golden(name):
    sd, f, lens = case(name)
    mu, lv, feats = vae_encode_ref.encode(sd, f, lens)
    n_seq = f.shape[0] * f.shape[1] // 16
    assert mu.shape == GE[name + "_mu"].shape == (2, n_seq, 128)
    assert float(np.abs(mu - GE[name + "_mu"]).max()) < 1e-5
    assert float(np.abs(lv - GE[name + "_logvar"]).max()) < 1e-5
    assert np.array_equal(feats[..., :3], GE[name + "_root"]) and np.array_equal(feats[..., 3:], f[..., 3:])


def test_golden_root_offsets_are_subtracted():
    f, _ = cases()["offset"]
    root = GE["offset_root"]
    assert np.abs(f[:, :, [0, 2]]).mean() > 40 and np.abs(root[:, :, [0, 2]]).mean() < 5
    assert not root[:, ::16, [0, 2]].any() and np.array_equal(root[..., 1], f[..., 1])


def _mirror(**kw):
    import torch
    from convofusion_amd.vae import ConvoFusionVae
    m = ConvoFusionVae(ablation=ABL, **dict(KW, **kw))
    if not kw:
        m.load_state_dict({k: torch.from_numpy(v) for k, v in vae_weights.make_state_dict().items()}, strict=True)
    return m.eval()


@pytest.mark.parametrize("shape,lengths", [((1, 40, 189), [40]), ((1, 32, 189), [40]), ((2, 32, 189), [16, 16]),
                                           ((2, 32, 189), [32]), ((1, 32, 100), [32]), ((32, 189), [32]), ((1, 0, 189), [0])])
def test_encode_refuses_shapes_the_reference_cannot_run(shape, lengths):
    import torch
    with pytest.raises(ValueError):
        _mirror().encode(torch.zeros(shape), lengths)


@pytest.mark.parametrize("kw", [dict(num_heads=4), dict(ff_size=512), dict(num_layers=11), dict(latent_dim=[1, 256]),
                                dict(latent_dim=[2, 128])])
def test_encode_refuses_configurations_outside_the_kernel(kw):
    import torch
    with pytest.raises(ValueError, match="specialised"):
        _mirror(**kw).encode(torch.zeros(1, 16, 189), [16])


def test_cpu_input_has_no_path():
    import torch
    m = _mirror()
    for lengths in ([16, 16], (16, 9), torch.tensor([16, 3]), None):
        with pytest.raises(NotImplementedError, match="no CPU path"):
            m.encode(torch.zeros(2, 16, 189), lengths)
    with pytest.raises(NotImplementedError):
        m(torch.zeros(2, 16, 189), [16, 16])


def test_pack_matches_the_kernel_layout():
    import torch
    from convofusion_amd.vae import _pack_w, encoder_pack_floats
    assert encoder_pack_floats(5) == 1734400          # ve_stack_floats(5), csrc/vae_enc.hpp
    w = torch.arange(32 * 48, dtype=torch.float32).reshape(32, 48)
    p = _pack_w(w).reshape(-1, 64, 4)                   # [(n/16 * K/16 + k/16)][lane][k % 4]
    for n, k in [(0, 0), (5, 7), (17, 33), (31, 47)]:
        lane = 16 * ((k % 16) // 4) + n % 16
        assert p[(n // 16) * 3 + k // 16, lane, k % 4] == w[n, k]
    padded = _pack_w(torch.ones(16, 69), 128)
    assert padded.numel() == 16 * 128 and padded.sum() == 16 * 69


def test_attach_hip_encode_builds_the_mirror_from_the_module():
    """A module with the reference's attribute layout (the mirror stands in for the reference class) and non-default hyper-parameters:
    the attached mirror takes them over, with the module's weights, and replaces the bound encode."""
    import torch
    from convofusion_amd.vae import ConvoFusionVae, attach_hip_encode
    host = ConvoFusionVae(ablation=ABL, **dict(KW, num_layers=3))
    host.mlp_dist, host.pe_type = False, "convofusion"
    host.body_encoder.middle_block.normalize_before = True
    with torch.no_grad():
        host.body_global_motion_token.fill_(0.25)
    mirror = attach_hip_encode(host)
    assert mirror is not host and host.encode == mirror.encode
    assert (mirror.num_layers, mirror.num_heads, mirror.ff_size, mirror.latent_dim) == (3, 2, 1024, 128)
    assert len(mirror.body_encoder.input_blocks) == 1 and bool((mirror.body_global_motion_token == 0.25).all())
    with pytest.raises(NotImplementedError):
        host.encode(torch.zeros(1, 16, 189), [16])
