"""Host-side tests of the fused VAE decode's Python surface: the refusals of ``decode(z, lengths, fused=True)`` are raised before any
device work (no GPU, no library), with a message that names the limit, and ``fused`` stays off by default in every signature that has it."""
import inspect

import pytest
import torch

from tests.test_vae_encode_host import ABL, KW


def _vae(**over):
    from convofusion_amd.vae import ConvoFusionVae
    return ConvoFusionVae(ablation=ABL, **{**KW, **over})


def test_refusals_name_the_limit_without_a_device():
    v = _vae()
    with pytest.raises(NotImplementedError, match=r"decode\(fused=True\): nframes = 257 exceeds the decoder fused forward's 256 frames"):
        v.decode(torch.zeros(2, 1, 8, 128), [257], fused=True)
    with pytest.raises(NotImplementedError, match=r"decode\(fused=True\): n_chunks = 17 exceeds the decoder fused forward's 16 latent chunks"):
        v.decode(torch.zeros(2, 2, 17, 128), [128, 5], fused=True)
    with pytest.raises(NotImplementedError, match=r"decoder's fused forward is specialised for .* 2 heads, .* this module has .* 4 heads"):
        _vae(num_heads=4).decode(torch.zeros(2, 1, 8, 128), [128], fused=True)
    even = _vae()
    even.num_layers = 4                       # (the constructor itself takes odd layer counts only)
    with pytest.raises(NotImplementedError, match=r"odd num_layers <= 9; this module has .* 4 layers"):
        even.decode(torch.zeros(2, 1, 8, 128), [128], fused=True)
    # arguments that mean nothing are ValueErrors, as decode_vjp's; a good shape on the CPU gets as far as the device check
    with pytest.raises(ValueError, match="lengths"):
        v.decode(torch.zeros(2, 2, 8, 128), [128], fused=True)
    with pytest.raises(RuntimeError, match="MI355X"):
        v.decode(torch.zeros(2, 1, 8, 128), [128], fused=True)


def test_the_refusal_is_decode_vjp_refusal_reworded_only_at_backward():
    from convofusion_amd.vae import decode_vjp_refusal
    assert decode_vjp_refusal(3, 128, 8, forward=True) is None and decode_vjp_refusal(3, 128, 8) is None
    cases = [dict(bs=1, nframes=257, n_chunks=8), dict(bs=1, nframes=128, n_chunks=17), dict(bs=65536, nframes=16, n_chunks=1),
             dict(bs=1, nframes=16, n_chunks=1, num_heads=4), dict(bs=1, nframes=16, n_chunks=1, num_layers=4)]
    for kw in cases:
        back, fwd = decode_vjp_refusal(**kw), decode_vjp_refusal(**kw, forward=True)
        assert "backward" in back and "backward" not in fwd
        assert fwd == back.replace("backward", "fused forward")


def test_fused_is_off_by_default_everywhere():
    from convofusion_amd import edit, longform, vae
    for fn, name in ((vae.ConvoFusionVae.decode, "fused"), (vae.attach_hip_decode, "fused"), (edit.pose_keyframe_loss, "fused"),
                     (edit.edit_motion, "fused_decode"), (edit.reperform_motion, "fused_decode"), (longform.synthesize_motion, "fused_decode")):
        assert inspect.signature(fn).parameters[name].default is False, fn.__qualname__


def test_consumers_call_decode_as_before_unless_asked():
    """With the option off a consumer calls ``vae.decode(z, lengths)`` with two arguments -- a vae that knows no ``fused`` keeps working."""
    from convofusion_amd import edit
    calls = []

    class TwoArg:
        def decode(self, z, lengths):
            calls.append((tuple(z.shape), list(lengths)))
            return torch.zeros(z.shape[1], max(lengths), 189)

    target, fmask = torch.zeros(1, 128, 189), torch.ones(1, 128)
    edit.pose_keyframe_loss(TwoArg(), target, fmask)(torch.zeros(1, 16, 128))
    assert calls == [((2, 1, 8, 128), [128])]
    with pytest.raises(TypeError):
        edit.pose_keyframe_loss(TwoArg(), target, fmask, fused=True)(torch.zeros(1, 16, 128))
