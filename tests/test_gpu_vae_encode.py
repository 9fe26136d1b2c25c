"""GPU tests (through the C ABI): ConvoFusionVae.encode in one HIP launch (cfd_vae_encode) against the imported reference's goldens
(tests/golden/vae_encode.npz) and the float64 restatement tests/vae_encode_ref.py."""
import numpy as np
import pytest

from oracle import vae_weights
from tests import vae_encode_ref
from tests.test_vae_encode_host import ABL, GE, KW, NAMES, case

pytestmark = pytest.mark.gpu


def _model(sd=None):
    import torch
    from convofusion_amd.vae import ConvoFusionVae
    m = ConvoFusionVae(ablation=ABL, **KW)
    sd = vae_weights.make_state_dict() if sd is None else sd
    m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
    return m.cuda().eval()


def _check(name, dist, feats, f):
    mu, lv = dist.mean.cpu().numpy(), (2 * dist.stddev.log()).cpu().numpy()
    e_mu = float(np.abs(mu - GE[name + "_mu"]).max())
    e_lv = float(np.abs(lv - GE[name + "_logvar"]).max())
    print(name, "HIP encode vs reference: mu max abs", e_mu, "logvar max abs", e_lv)
    assert e_mu < 1e-4 and e_lv < 1e-4
    got = feats.cpu().numpy()
    assert np.array_equal(got[..., :3], GE[name + "_root"]) and np.array_equal(got[..., 3:], f[..., 3:])


@pytest.mark.parametrize("name", NAMES)
def test_encode_matches_reference_golden(name):
    import torch
    sd, f, lens = case(name)
    latent, dist, feats = _model(sd).encode(torch.from_numpy(f).cuda(), lens)
    bs, nframes, _ = f.shape
    assert tuple(latent.shape) == (2, bs, nframes // 16, 128) and tuple(feats.shape) == f.shape
    assert tuple(dist.mean.shape) == (2, bs * nframes // 16, 128)
    _check(name, dist, feats, f)


@pytest.mark.parametrize("lengths_kind", ["list", "tuple", "tensor"])
def test_rsample_draws_like_the_reference(lengths_kind):
    import torch
    sd, f, lens = case("ragged")
    lengths = {"list": list(lens), "tuple": tuple(lens), "tensor": torch.tensor(lens)}[lengths_kind]
    m = _model(sd)
    torch.manual_seed(11)
    latent, dist, _ = m.encode(torch.from_numpy(f).cuda(), lengths)
    assert isinstance(dist, torch.distributions.Normal)
    torch.manual_seed(11)
    again = torch.distributions.Normal(dist.mean, dist.stddev).rsample()
    assert torch.equal(latent, again.reshape(latent.shape))


def test_test_py_shape_against_float64():
    """test.py's batch: 32 sequences of 128 frames, ragged lengths (fully masked chunks included)."""
    import torch
    rng = np.random.Generator(np.random.PCG64(5))
    bs, nframes = 32, 128
    f = rng.standard_normal((bs, nframes, 189), dtype=np.float32)
    f[:, :, [0, 2]] += rng.uniform(-20, 20, (bs, 1, 2)).astype(np.float32)
    lens = [128] + [int(v) for v in rng.integers(16, 129, bs - 1)]
    sd = vae_weights.make_state_dict()
    _, dist, feats = _model(sd).encode(torch.from_numpy(f).cuda(), lens)
    mu, lv, want_feats = vae_encode_ref.encode(sd, f, lens)
    e_mu = float(np.abs(dist.mean.cpu().numpy() - mu).max())
    e_lv = float(np.abs((2 * dist.stddev.log()).cpu().numpy() - lv).max())
    print("B=32 x 128 frames vs float64: mu max abs", e_mu, "logvar max abs", e_lv)
    assert e_mu < 1e-4 and e_lv < 1e-4
    assert np.array_equal(feats.cpu().numpy(), want_feats)


def test_encode_of_decode_output():
    """test.py's chain (convofusion.py:1053-1057): encode(decode(z, lengths), lengths) on decode's non-contiguous output."""
    import torch
    rng = np.random.Generator(np.random.PCG64(8))
    lens = [64, 41, 64]
    z = torch.from_numpy(rng.standard_normal((2, 3, 4, 128), dtype=np.float32)).cuda()
    sd = vae_weights.make_state_dict()
    m = _model(sd)
    rec = m.decode(z, lens)
    assert not rec.is_contiguous()
    latent, dist, feats = m.encode(rec, lens)
    f = rec.contiguous().cpu().numpy()
    mu, lv, want_feats = vae_encode_ref.encode(sd, f, lens)
    e_mu = float(np.abs(dist.mean.cpu().numpy() - mu).max())
    e_lv = float(np.abs((2 * dist.stddev.log()).cpu().numpy() - lv).max())
    print("encode(decode(z)) vs float64: mu max abs", e_mu, "logvar max abs", e_lv)
    assert e_mu < 1e-4 and e_lv < 1e-4 and tuple(latent.shape) == (2, 3, 4, 128)
    assert np.array_equal(feats.cpu().numpy(), want_feats)


def test_reloading_weights_after_a_first_encode():
    import torch
    sd, f, lens = case("single")
    m = _model(sd)
    x = torch.from_numpy(f).cuda()
    _check("single", m.encode(x, lens)[1], m.encode(x, lens)[2], f)
    sd2, _, _ = case("reseed")
    m.load_state_dict({k: torch.from_numpy(v) for k, v in sd2.items()}, strict=True)
    _, dist, feats = m.encode(x, lens)
    _check("reseed", dist, feats, f)


def test_attach_hip_encode_uses_the_modules_own_weights():
    """attach_hip_encode(vae) on a module with the reference's attribute layout (the mirror stands in for the reference class, which
    cannot travel to the GPU box) reroutes encode to a mirror holding a snapshot of the module's weights."""
    import torch
    from convofusion_amd.vae import attach_hip_encode
    sd, f, lens = case("offset")
    host = _model(sd)
    host.mlp_dist, host.pe_type = False, "convofusion"
    host.body_encoder.middle_block.normalize_before = True
    mirror = attach_hip_encode(host)
    assert mirror is not host
    _, dist, feats = host.encode(torch.from_numpy(f).cuda(), lens)
    _check("offset", dist, feats, f)
