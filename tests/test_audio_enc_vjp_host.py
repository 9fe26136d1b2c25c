"""CPU: the host side of ``cfd_audio_encoder_vjp`` -- the float64 oracle of its GPU tests against torch autograd, the struct's layout,
and every refusal of ``fit.fit_audio_encoder``, none of which needs a device."""
import ctypes as C
from types import SimpleNamespace

import numpy as np
import pytest
import torch
import torch.nn as nn

from tests import audio_enc_vjp_ref as R


def _sequential(params):
    w0, w1, w2 = params[R.KEYS[0]], params[R.KEYS[2]], params[R.KEYS[4]]
    seq = nn.Sequential(nn.Linear(w0.shape[1], w0.shape[0]), nn.LeakyReLU(0.1), nn.Linear(w1.shape[1], w1.shape[0]), nn.LeakyReLU(0.1),
                        nn.Linear(w2.shape[1], w2.shape[0])).double()
    own = [seq[0].weight, seq[0].bias, seq[2].weight, seq[2].bias, seq[4].weight, seq[4].bias]
    with torch.no_grad():
        for p, k in zip(own, R.KEYS):
            p.copy_(torch.from_numpy(params[k]).double())
    return seq, own


@pytest.mark.parametrize("rows,widths,zero", [(7, (80, 256, 512), False), (4, (5, 7, 9), False), (2, (80, 256, 512), True)])
def test_the_restatement_is_torch_autograd_at_float64(rows, widths, zero):
    """``zero``: all-zero biases and an all-zero first row, so every pre-activation of that row is exactly 0 and the slope there is 0.1."""
    params = R.seeded_params(*widths, seed=11, zero_bias=zero)
    x, d = R.seeded_inputs(rows, widths[0], widths[2], seed=12)
    if zero:
        x[0] = 0.0
    seq, own = _sequential(params)
    xt = torch.from_numpy(x).double().requires_grad_(True)
    y = seq(xt)
    grads = torch.autograd.grad(y, [xt] + own, torch.from_numpy(d).double())
    got = R.encoder_vjp(x, params, d, np.float64)
    assert R.rel_l2(got["out"], y.detach().numpy()) < 1e-14
    for name, g in zip(("d_x",) + R.KEYS, grads):
        assert R.rel_l2(got[name], g.numpy()) < 1e-13, name
    if zero:
        w0, w1, w2 = (params[k].astype(np.float64) for k in R.KEYS[0::2])
        np.testing.assert_allclose(got["d_x"][0], 0.01 * (d[0].astype(np.float64) @ w2 @ w1 @ w0), rtol=1e-12, atol=0)


def test_the_float32_restatement_loses_what_float32_loses():
    """The yardstick of the GPU gate is a float32 run: neither exact nor worse than 1e-5 of any tensor at the sizes the tests use."""
    params = R.seeded_params(80, 256, 512, seed=13)
    x, d = R.seeded_inputs(33, 80, 512, seed=14)
    for name, got, f32 in R.gate_report(R.encoder_vjp(x, params, d, np.float32), x, params, d, ("out", "d_x") + R.KEYS):
        print(f"{name}: float32 restatement vs float64 {f32:.2e}")
        assert got == f32 and 0 < f32 < 1e-5, (name, f32)


def test_struct_layout_and_symbol():
    from convofusion_amd import _lib
    A = _lib.AudioEncArgs
    assert [getattr(A, f).offset for f in ("x", "n_rows", "in_dim", "hidden", "latent", "w0", "b0", "w1", "b1", "w2", "b2")] == \
        [0, 8, 16, 20, 24, 32, 40, 48, 56, 64, 72]            # (the three ints, padding, then 8-aligned pointers)
    assert C.sizeof(A) == 80
    assert "cfd_audio_encoder_vjp" in _lib.SYMBOLS


def _fit_args():
    from convofusion_amd.conditioning import AudioConvEncoder
    enc = AudioConvEncoder(80, 256, 512).eval()
    B, L, S = 2, 4, (3, 5, 6, 2, 1)
    sched = SimpleNamespace(config=SimpleNamespace(num_train_timesteps=1000, prediction_type="epsilon"))
    return dict(enc=enc, latents=torch.zeros(B, L, 128), mel=torch.zeros(B, S[1], 80), mems=[torch.zeros(B, s, 512) for s in S], sched=sched)


def _fit(a, **kw):
    from convofusion_amd import fit
    args = dict(steps=1, lr=0.1)
    args.update(kw)
    # the denoiser is never reached: every refusal comes before device work
    return fit.fit_audio_encoder(None, a["sched"], a["enc"], a["latents"], a["mel"], a["mems"], **args)


def test_fit_audio_encoder_refuses_before_device_work():
    from convofusion_amd.conditioning import AUDIO_ENC_KEYS, AudioConvEncoder
    a = _fit_args()
    assert AUDIO_ENC_KEYS == R.KEYS
    with pytest.raises(ValueError, match="train names no parameter"):
        _fit(a, train=())
    with pytest.raises(ValueError, match="does not exist: 'main.1.weight'"):
        _fit(a, train=("main.1.weight",))
    with pytest.raises(ValueError, match="twice"):
        _fit(a, train=("out_net.bias", "out_net.bias"))
    with pytest.raises(ValueError, match=r"mel must be \[B, S, 80\]"):
        _fit({**a, "mel": torch.zeros(2, 5, 64)})
    with pytest.raises(ValueError, match="mel has 3 examples, latents 2"):
        _fit({**a, "mel": torch.zeros(3, 5, 80)})
    with pytest.raises(ValueError, match="5-tuple"):
        _fit({**a, "mems": a["mems"][:4]})
    with pytest.raises(ValueError, match="latents must be"):
        _fit({**a, "latents": torch.zeros(2, 4)})
    with pytest.raises(ValueError, match="steps = 0"):
        _fit(a, steps=0)
    with pytest.raises(ValueError, match="timesteps has 1 entries for 2 steps"):
        _fit(a, steps=2, timesteps=[5])
    with pytest.raises(ValueError, match=r"timestep 1000 outside \[0, 1000\)"):
        _fit(a, timesteps=[1000])
    with pytest.raises(ValueError, match="memory tlsn"):
        _fit({**a, "mems": [m if j != 2 else torch.zeros(3, 6, 512) for j, m in enumerate(a["mems"])]})
    with pytest.raises(ValueError, match="memory alsn"):                     # the encoder's latent_dim is not the denoiser's 512
        _fit({**a, "enc": AudioConvEncoder(80, 256, 256).eval()})
    v = SimpleNamespace(config=SimpleNamespace(num_train_timesteps=1000, prediction_type="v_prediction"))
    with pytest.raises(NotImplementedError, match="v_prediction"):
        _fit({**a, "sched": v})
    with pytest.raises(NotImplementedError, match="row-tile path only"):
        _fit({**a, "latents": torch.zeros(2, 4096, 128)})
    with pytest.raises(NotImplementedError, match="eval mode"):
        _fit({**a, "enc": AudioConvEncoder(80, 256, 512)})
    with pytest.raises(ValueError, match="float32 on the latents' device"):
        _fit({**a, "enc": AudioConvEncoder(80, 256, 512).eval().double()})
    # the alsn entry of the memories is not read: None passes every check, and the first thing past them is the device
    mems = list(a["mems"])
    mems[1] = None
    with pytest.raises(Exception) as e:
        _fit({**a, "mems": mems})
    assert not isinstance(e.value, (ValueError, NotImplementedError)), e.value


def test_direct_call_and_forward_refuse_on_the_host():
    from convofusion_amd.conditioning import AudioConvEncoder, audio_encoder_vjp
    enc = AudioConvEncoder(80, 256, 512)
    with pytest.raises(NotImplementedError, match="eval mode"):
        enc(torch.zeros(1, 2, 80), weight_grad=True)
    enc.eval()
    with pytest.raises(ValueError, match="does not exist"):
        audio_encoder_vjp(enc, torch.zeros(1, 2, 80), torch.zeros(1, 2, 512), want=("out_net",))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        audio_encoder_vjp(enc, torch.zeros(1, 2, 80), torch.zeros(1, 2, 512))
