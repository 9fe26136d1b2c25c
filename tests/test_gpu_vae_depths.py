"""GPU tests of the VAE decoder (csrc/vae_dec.hpp) at the depths it accepts besides 5: num_layers 1, 3, 7, 9 -- nb = 0, 1, 3, 4 input /
output blocks -- through ``decode_vjp``, ``decode(fused=True)`` and the plain ``decode``.  What depends on the depth: the forward-only
slot rotation (vd_xslot), the skip gradients gskip[nb], the per-layer d_z sum and the workspace layout.

One case (tests/vae_vjp_ref.DEPTH_CASE): z [2, 2, 3, 128], lengths [40, 17] -- three row tiles, the last one partial, a short sequence --
with seeded weights of each depth (oracle.vae_weights.make_state_dict(num_layers=...)).  Everything is held to the float64 restatement
tests/vae_vjp_ref.py, which tests/test_vae_depths_host.py pins to the imported reference at depths 1 and 9.

Gradient and stage taps: relative L2 and worst 128-wide row (vae_vjp_ref.errors), at most GATE = 8 x the yardstick, the factor of
tests/test_gpu_vae_vjp.py; the yardstick is the distance of the restatement's own float32 run (numpy float32) from its float64 run.
Forward: max abs under the project's 1e-4, padded frames exactly 0.

Measured on an MI355X (d_z: relative L2 / worst row, as a multiple of the float32 restatement's own distance from float64):
    num_layers 1   1.2e-06 / 2.5e-06   (2.21 x / 3.01 x)        num_layers 3   1.2e-06 / 2.1e-06   (1.75 x / 1.97 x)
    num_layers 7   1.4e-06 / 2.9e-06   (1.77 x / 2.13 x)        num_layers 9   1.4e-06 / 2.8e-06   (1.64 x / 1.86 x)
the same figures against the reference's float64 autograd at 1 and 9; every stage tap within 3.01 x (vae.dz.0 at num_layers 1, which is
d_z itself; vae.g.* 0.31 x to 2.50 x, vae.dz.* 0.92 x to 2.80 x elsewhere); the three forwards 4.1e-06 to 5.8e-06 max abs from float64.
"""
import functools

import numpy as np
import pytest

from oracle import vae_weights
from tests import vae_vjp_ref as R
from tests.helpers import load_golden
from tests.test_gpu_vae_decode_fused import _c_decode, _ticket, _ws_bytes
from tests.test_gpu_vae_vjp import GATE, _read
from tests.test_oracle_vae import ABL, KW

pytestmark = pytest.mark.gpu

DEPTHS = (1, 3, 7, 9)
ENDS = (1, 9)


@functools.lru_cache(maxsize=None)
def _sd(nl):
    return vae_weights.make_state_dict(num_layers=nl)


@functools.lru_cache(maxsize=None)
def _model(nl):
    import torch
    from convofusion_amd.vae import ConvoFusionVae
    m = ConvoFusionVae(ablation=ABL, **dict(KW, num_layers=nl))
    m.load_state_dict({k: torch.from_numpy(v) for k, v in _sd(nl).items()}, strict=True)
    return m.cuda().eval()


@functools.lru_cache(maxsize=None)
def _restated(nl):
    """(feats, d_z, taps) of the float64 restatement and the yardstick (relative L2, worst row) of its float32 run, once per depth"""
    z, lens, d = R.depth_case_inputs()
    feats, d_z, taps = R.decode_vjp(_sd(nl), z, lens, d, num_layers=nl)
    _, d_z32, _ = R.decode_vjp(_sd(nl), z, lens, d, num_layers=nl, dtype=np.float32)
    assert d_z32.dtype == np.float32
    return feats, d_z, taps, R.errors(d_z32, d_z)


def _dev():
    import torch
    z, lens, d = R.depth_case_inputs()
    return torch.from_numpy(z).cuda(), lens, torch.from_numpy(d).cuda()


@functools.lru_cache(maxsize=None)
def _device_result(nl):
    """(feats, d_z) of one decode_vjp call at depth nl, as numpy arrays; shared by the tests that only read them"""
    z, lens, d = _dev()
    feats, d_z = _model(nl).decode_vjp(z, lens, d)
    return feats.cpu().numpy(), d_z.cpu().numpy()


@pytest.mark.parametrize("nl", DEPTHS)
def test_gradient_matches_the_float64_restatement(nl):
    """Measured on the MI355X (the table at the head of this file): 1.64 x to 2.21 x (relative L2), 1.86 x to 3.01 x (worst row)."""
    got = _device_result(nl)[1]
    _, want, _, yard = _restated(nl)
    rel, row = R.errors(got, want)
    print(f"num_layers {nl}: d_z vs float64 rel L2 {rel:.3e} worst row {row:.3e}; float32 restatement {yard[0]:.3e} {yard[1]:.3e} "
          f"({rel / yard[0]:.2f} x, {row / yard[1]:.2f} x)")
    assert got.shape == want.shape and np.isfinite(got).all()
    assert rel <= GATE * yard[0] and row <= GATE * yard[1]


@pytest.mark.parametrize("nl", ENDS)
def test_gradient_matches_the_reference_float64_autograd(nl):
    """The same gate against the imported reference's own float64 autograd gradient (tests/golden/vae_depths.npz)."""
    got = _device_result(nl)[1]
    yard = _restated(nl)[3]
    rel, row = R.errors(got, load_golden("vae_depths")[f"dec{nl}.grad"])
    print(f"num_layers {nl}: d_z vs the reference's float64 autograd rel L2 {rel:.3e} worst row {row:.3e}")
    assert rel <= GATE * yard[0] and row <= GATE * yard[1]


@pytest.mark.parametrize("nl", DEPTHS)
def test_forwards_match_the_float64_restatement_and_pad_with_zeros(nl):
    """decode_vjp's forward, decode(fused=True) and the plain decode (the launch sequence)."""
    import torch
    z, lens, _ = _dev()
    want = _restated(nl)[0]
    m = _model(nl)
    with torch.no_grad():
        outs = {"decode_vjp": _device_result(nl)[0], "fused": m.decode(z, lens, fused=True).cpu().numpy(),
                "plain": m.decode(z.clone(), lens).cpu().numpy()}
    for k, got in outs.items():
        err = float(np.abs(got - want).max())
        print(f"num_layers {nl}: {k} forward vs float64: max abs {err:.3e}")
        assert got.shape == want.shape == (2, 40, 189) and err < 1e-4, k
        for b, n in enumerate(lens):
            assert not got[b, n:].any() and got[b, :n].any(), k


@pytest.mark.parametrize("nl", DEPTHS)
def test_stage_taps_match_the_restatement(nl):
    """The running gradient entering every layer (with the skip tensors' share) and every layer's contribution to d_z: what names the
    layer when a slot or a skip index is wrong."""
    import torch
    z, lens, d = _dev()
    m = _model(nl)
    m.decode_vjp(z, lens, d)
    torch.cuda.synchronize()
    taps, yard = _restated(nl)[2], _restated(nl)[3]
    bs, nc, nfr = z.shape[1], z.shape[2], max(lens)
    fp = (nfr + 15) // 16 * 16
    info = _read("vae.info", 2)
    assert int(info[1]) == fp and int(info[0]) == (2 * nl + 2) + (2 * nl - 1) + 2          # forward, sweep, the two d_z kernels
    worst = {}
    for l in reversed(range(nl)):
        g = _read(f"vae.g.{l}", 2 * bs * fp * 128).reshape(2, bs, fp, 128)[:, :, :nfr]
        dz = _read(f"vae.dz.{l}", 2 * bs * 16 * 128).reshape(2, bs, 16, 128)[:, :, :nc]
        want_g = np.stack([taps[f"g.{s}.{l}"].transpose(1, 0, 2) for s in range(2)])
        want_dz = np.stack([taps[f"dz.{s}.{l}"] for s in range(2)])
        for b, n in enumerate(lens):
            assert not g[:, b, n:].any() and not want_g[:, b, n:].any()
        worst[f"g.{l}"], worst[f"dz.{l}"] = R.errors(g, want_g), R.errors(dz, want_dz)
    for k, (rel, row) in worst.items():
        print(f"num_layers {nl} {k}: rel L2 {rel:.3e} ({rel / yard[0]:.2f} x) worst row {row:.3e} ({row / yard[1]:.2f} x)")
    for k, (rel, row) in worst.items():
        assert rel <= GATE * yard[0] and row <= GATE * yard[1], k


@pytest.mark.parametrize("nl", ENDS)
def test_bit_properties_at_the_ends_of_the_range(nl):
    """What tests/test_gpu_vae_decode_fused.py and test_gpu_vae_vjp.py hold at depth 5: the forward-only call (vd_xslot's rotation) has
    the saving forward's bits; two calls give the same bits; a kept forward and its sweep are decode_vjp."""
    import torch
    m = _model(nl)
    z, lens, d = _dev()
    want_f, want_g = (torch.from_numpy(a).cuda() for a in _device_result(nl))
    with torch.no_grad():
        fused = m.decode(z, lens, fused=True)
    assert fused.grad_fn is None and torch.equal(fused, want_f) and _ticket() == 0
    feats2, d_z2 = m.decode_vjp(z, lens, d)
    assert torch.equal(feats2, want_f) and torch.equal(d_z2, want_g)
    with torch.no_grad():
        assert torch.equal(m.decode(z, lens, fused=True), fused)
    zg = z.clone().requires_grad_()
    feats = m.decode(zg, lens, fused=True)
    t = _ticket()
    assert feats.grad_fn is not None and torch.equal(feats, want_f) and t != 0 and feats.grad_fn.ticket == t
    (g,) = torch.autograd.grad(feats, zg, d)
    assert torch.equal(g, want_g) and _ticket() == t                          # the sweep over the kept forward: no decode_vjp ran


@pytest.mark.parametrize("nl", DEPTHS)
def test_forward_only_workspace_follows_the_depth(nl):
    """(nb + 6) * 512 bytes per token row (2 * bs * fp rows) plus num_layers * 16 KiB per (stack, sequence) on a fresh handle, and the
    saving forward of the same shape more; both have decode_vjp's forward bits."""
    import torch
    from convofusion_amd import _lib
    m = _model(nl)
    z, lens, _ = _dev()
    bs, fp, nb = z.shape[1], (max(lens) + 15) // 16 * 16, (nl - 1) // 2
    want = torch.from_numpy(_device_result(nl)[0]).cuda()
    lean_h, keep_h = _lib.create_handle(), _lib.create_handle()
    try:
        assert _ws_bytes(lean_h) == 0
        feats, t = _c_decode(lean_h, m, z, lens, keep=False)
        lean = _ws_bytes(lean_h)
        assert t == 0 and _ticket(lean_h) == 0 and torch.equal(feats, want)
        feats, t = _c_decode(keep_h, m, z, lens, keep=True)
        kept = _ws_bytes(keep_h)
        assert t != 0 and _ticket(keep_h) == t and torch.equal(feats, want)
        print(f"num_layers {nl}: forward-only workspace {lean} bytes, saving forward {kept} bytes")
        assert lean == 2 * bs * fp * (nb + 6) * 512 + nl * 2 * bs * 16384
        assert lean < kept
    finally:
        torch.cuda.synchronize()
        _lib.load().cfd_destroy(lean_h)
        _lib.load().cfd_destroy(keep_h)
