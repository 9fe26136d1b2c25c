"""GPU tests of the fused VAE decode: cfd_vae_decode / cfd_vae_decode_sweep (csrc/vae_dec.hpp, the SAVE template flag) through
``ConvoFusionVae.decode(z, lengths, fused=True)``, its autograd function, and the consumers that hand the choice on.

The cases, weights and the ``decode_vjp`` results they are held to are those of tests/test_gpu_vae_vjp.py (one ``decode_vjp`` call per case,
shared).  Everything the fused path computes is held to ``decode_vjp`` bit for bit: it runs the same kernels, and the forward-only
instance performs the same arithmetic in the same order.

Measured on an MI355X: the fused forward against the decode golden 4.2e-06 .. 2.3e-05 (gate 1e-4), as decode_vjp's; the 3-iteration guided
run with ``pose_keyframe_loss(fused=True)`` against ``fused=False``: relative L2 of the final latents 3.9e-05 (the guidance moves them by
0.96) with the two forwards 4.8e-06 apart (max abs); ``synthesize_motion(fused_decode=True)`` against the default: 5.4e-06 max abs.
"""
import ctypes as C

import numpy as np
import pytest

from oracle import vae_ref, vae_weights
from tests import vae_vjp_ref as R
from tests.helpers import load_golden, rel_l2
from tests.test_gpu_vae_vjp import NAMES, _dev, _device_result, _loop_case, _model

pytestmark = pytest.mark.gpu

CFD_E_STATE = -3
TRAJ_TOL = 1e-3          # the project's trajectory budget (tests/test_gpu_edit.py, tests/test_gpu_longform.py)


def _handle():
    from convofusion_amd.conditioning import _engine_handle
    return _engine_handle("cuda")


def _ticket(h=None):
    from convofusion_amd import _lib
    return int(_lib.load().cfd_vae_decode_ticket(_handle() if h is None else h))


def _fused(name):
    import torch
    z, lens, _ = _dev(name)
    with torch.no_grad():
        return _model().decode(z, lens, fused=True)


@pytest.mark.parametrize("name", NAMES)
def test_fused_forward_has_the_bits_of_the_saving_forward(name):
    import torch
    _, lens, _ = R.case_inputs(name)
    want = torch.from_numpy(_device_result(name)[0]).cuda()
    got = _fused(name)
    assert got.grad_fn is None and got.shape == want.shape and torch.equal(got, want)
    assert _ticket() == 0                                              # forward-only: nothing is kept
    for b, n in enumerate(lens):
        assert not got[b, n:].any()                                    # padded frames: exactly 0
        assert bool(got[b, :n].any())


@pytest.mark.parametrize("name", NAMES)
def test_fused_forward_matches_the_decode_golden(name):
    """The gate of test_forward_matches_the_decode_golden_and_pads_with_zeros, on the fused call's own output."""
    z, lens, _ = R.case_inputs(name)
    got = _fused(name).cpu().numpy()
    G = load_golden("vae_decode")
    want = G[name] if name in G else vae_ref.decode(vae_weights.make_state_dict(), z, lens)
    err = float(np.abs(got - want).max())
    print(f"{name}: decode(fused=True) vs the decode golden: max abs {err:.3e}")
    assert got.shape == want.shape and err < 1e-4


@pytest.mark.parametrize("name", NAMES)
def test_kept_forward_and_sweep_are_decode_vjp(name):
    import torch
    m = _model()
    z, lens, d = _dev(name)
    want_f, want_g = (torch.from_numpy(a).cuda() for a in _device_result(name))
    plain = _fused(name)
    zg = z.clone().requires_grad_()
    feats = m.decode(zg, lens, fused=True)
    assert feats.grad_fn is not None and torch.equal(feats, want_f) and torch.equal(feats, plain)
    t = _ticket()
    assert t != 0 and feats.grad_fn.ticket == t                        # the backward below is the sweep over the kept forward
    (g,) = torch.autograd.grad(feats, zg, d)
    assert torch.equal(g, want_g)
    assert _ticket() == t                                              # ... which keeps it: no decode_vjp ran
    with torch.no_grad():
        assert m.decode(zg, lens, fused=True).grad_fn is None


def test_a_stale_ticket_falls_back_to_decode_vjp_and_the_c_call_refuses_it():
    import torch
    from convofusion_amd import _lib
    m = _model()
    z, lens, d = _dev("ragged")
    z2, lens2, _ = _dev("single")
    want = torch.from_numpy(_device_result("ragged")[1]).cuda()
    lib, h = _lib.load(), _handle()
    for second_under_grad in (False, True):
        zg = z.clone().requires_grad_()
        feats = m.decode(zg, lens, fused=True)
        t1 = feats.grad_fn.ticket
        assert t1 != 0 and _ticket() == t1
        if second_under_grad:
            other = m.decode(z2.clone().requires_grad_(), lens2, fused=True)        # keeps its own forward: a new ticket
            assert _ticket() not in (0, t1) and other.grad_fn.ticket == _ticket()
        else:
            with torch.no_grad():
                m.decode(z2, lens2, fused=True)                                      # forward-only: nothing kept
            assert _ticket() == 0
        # the C call refuses the old ticket before any launch
        dz = torch.full_like(z, float("nan"))
        dc = d.contiguous()
        rc = lib.cfd_vae_decode_sweep(h, C.c_uint64(t1), C.c_void_p(dc.data_ptr()), C.c_void_p(dz.data_ptr()), None)
        msg = lib.cfd_last_error().decode()
        print(f"stale ticket {t1}: {rc}: {msg}")
        assert rc == CFD_E_STATE and "stale" in msg and str(t1) in msg
        torch.cuda.synchronize()
        assert bool(torch.isnan(dz).all())                                           # nothing ran
        # the backward of the first forward recomputes (decode_vjp on the saved z): the same bits, no exception
        (g,) = torch.autograd.grad(feats, zg, d)
        assert torch.equal(g, want)
        assert _ticket() != t1
    rc = lib.cfd_vae_decode_sweep(h, C.c_uint64(0), C.c_void_p(dc.data_ptr()), C.c_void_p(dz.data_ptr()), None)
    assert rc == CFD_E_STATE


def _c_decode(h, m, z, lens, keep):
    """One cfd_vae_decode on handle ``h`` through the C ABI; returns (feats, ticket)."""
    import torch
    from convofusion_amd import _lib
    pack = m._decoder_pack(z.device)
    lens_d = torch.tensor(lens, dtype=torch.int32, device=z.device)
    feats = torch.empty(z.shape[1], max(lens), 189, device=z.device)
    args = _lib.VaeDecodeArgs(C.c_void_p(pack.data_ptr()), 128, 2, 1024, m.num_layers, z.shape[1], max(lens), z.shape[2],
                              C.c_void_p(z.data_ptr()), C.c_void_p(lens_d.data_ptr()))
    t = C.c_uint64(0)
    torch.cuda.synchronize()
    _lib.check(_lib.load().cfd_vae_decode(h, C.byref(args), C.c_void_p(feats.data_ptr()), C.byref(t) if keep else None, None))
    torch.cuda.synchronize()
    return feats, t.value


def _ws_bytes(h):
    from convofusion_amd import _lib
    n = C.c_longlong(-1)
    _lib.check(_lib.load().cfd_debug_vae_workspace(h, C.byref(n)))
    return n.value


@pytest.mark.parametrize("name", ["tiny", "ragged"])
def test_forward_only_workspace_is_lean(name):
    """On a fresh handle the forward-only call allocates what DESIGN.md section 5.3.2 states: (nb + 6) * 512 bytes per token row (2 * bs *
    fp rows, fp = nframes rounded up to 16; nb = (num_layers - 1) / 2) plus num_layers * 16 KiB per (stack, sequence) -- and a saving
    forward of the same shape on another fresh handle more."""
    import torch
    from convofusion_amd import _lib
    m = _model()
    z, lens, _ = _dev(name)
    bs, fp, nl = z.shape[1], (max(lens) + 15) // 16 * 16, m.num_layers
    want = torch.from_numpy(_device_result(name)[0]).cuda()
    lean_h, keep_h = _lib.create_handle(), _lib.create_handle()
    try:
        assert _ws_bytes(lean_h) == 0
        feats, t = _c_decode(lean_h, m, z, lens, keep=False)
        lean = _ws_bytes(lean_h)
        assert t == 0 and _ticket(lean_h) == 0 and torch.equal(feats, want)
        feats, t = _c_decode(keep_h, m, z, lens, keep=True)
        kept = _ws_bytes(keep_h)
        assert t != 0 and _ticket(keep_h) == t and torch.equal(feats, want)
        print(f"{name}: forward-only workspace {lean} bytes, saving forward {kept} bytes")
        assert lean == 2 * bs * fp * ((nl - 1) // 2 + 6) * 512 + nl * 2 * bs * 16384
        assert lean < kept
    finally:
        torch.cuda.synchronize()
        _lib.load().cfd_destroy(lean_h)
        _lib.load().cfd_destroy(keep_h)


def test_two_fused_forwards_give_the_same_bits():
    import torch
    assert torch.equal(_fused("long"), _fused("long"))
    m = _model()
    z, lens, d = _dev("long")
    grads = []
    for _ in range(2):
        zg = z.clone().requires_grad_()
        grads.append(torch.autograd.grad(m.decode(zg, lens, fused=True), zg, d)[0])
    assert torch.equal(grads[0], grads[1])


def test_attach_hip_decode_hands_the_choice_on():
    """A second mirror stands in for the reference class, as in test_gpu_vae_vjp.py."""
    import torch
    from convofusion_amd.vae import ConvoFusionVae, attach_hip_decode
    from tests.test_oracle_vae import ABL, KW
    m = _model()
    z, lens, _ = _dev("single")
    host = ConvoFusionVae(ablation=ABL, **KW)
    host.load_state_dict(m.state_dict(), strict=True)
    host = host.cuda().eval()
    host.mlp_dist, host.pe_type = False, "convofusion"
    host.body_decoder.middle_block.normalize_before = True
    # (every default-path call gets a z of its own: at bs 1 the launch sequence adds the memory PE into a contiguous z[s] in place)
    with torch.no_grad():
        plain = m.decode(z.clone(), lens)
        attach_hip_decode(host, fused=True)
        assert torch.equal(host.decode(z, lens), _fused("single")) and torch.equal(host.decode(z.clone(), lens, fused=False), plain)
        attach_hip_decode(host)
        assert torch.equal(host.decode(z.clone(), lens), plain)


def test_fused_decode_between_two_steps_leaves_an_open_run_s_bits():
    import torch
    from convofusion_amd import scheduler
    from convofusion_amd.sampler import SamplingRun
    from tests.gpu_helpers import SCHED_KW, hip_denoiser
    vae, m = _model(), hip_denoiser(1234, 1.0)
    cb, mems, masks, _, _, _ = _loop_case()
    sch = scheduler.DDIMScheduler(**SCHED_KW)
    z, lens, d = _dev("single")
    want_f, want_g = (torch.from_numpy(a).cuda() for a in _device_result("single"))

    def go(interleave):
        outs = []
        with SamplingRun(m, sch, mems, masks, 1, 16, 4, guidance_scale=7.5, eta=0.0, seed=3) as run:
            for i in range(4):
                run.steps(1)
                if interleave and i % 2 == 0:
                    with torch.no_grad():
                        outs.append(vae.decode(z, lens, fused=True))
                elif interleave:
                    zg = z.clone().requires_grad_()
                    f = vae.decode(zg, lens, fused=True)
                    outs.append(f.detach())
                    assert torch.equal(torch.autograd.grad(f, zg, d)[0], want_g)
            return run.read(), outs

    plain, _ = go(False)
    mixed, outs = go(True)
    assert torch.equal(plain, mixed)
    assert len(outs) == 4 and all(torch.equal(o, want_f) for o in outs)


def test_pose_keyframe_loss_fused_in_the_guided_loop():
    """The two 3-iteration guided runs differ only through the forward that feeds the loss (the gradient's kernels are the same): the final
    latents agree within the project's trajectory budget (relative L2 1e-3) -- loose next to the figure observed, printed below."""
    import torch
    from convofusion_amd import edit, sampler, scheduler
    from tests.gpu_helpers import SCHED_KW, hip_denoiser, to_dev
    vae, m = _model(), hip_denoiser(1234, 1.0)
    cb, mems, masks, target, fmask, cmask = _loop_case()
    sch = scheduler.DDIMScheduler(**SCHED_KW)
    kw = dict(B=1, L=16, num_inference_steps=3, guidance_scale=7.5, eta=0.0, init_latents=to_dev(cb["init"]))
    runs = {}
    for fused in (False, True):
        loss = edit.pose_keyframe_loss(vae, target, fmask, cmask, fused=fused)
        runs[fused] = sampler.sample_with_loss_guidance(m, sch, mems, masks, loss, 40.0, **kw)
    plain = sampler.sample(m, sch, mems, masks, **kw)
    with torch.no_grad():
        zv = edit.loop_to_vae(runs[False])
        fwd = float((vae.decode(zv, [128], fused=True) - vae.decode(zv, [128])).abs().max())
    err = rel_l2(runs[True].cpu().numpy(), runs[False].cpu().numpy())
    moved = rel_l2(runs[False].cpu().numpy(), plain.cpu().numpy())
    print(f"guided latents fused vs unfused: rel L2 {err:.3e} (the guidance itself moved them {moved:.3e}); the two forwards differ by {fwd:.3e} max abs")
    assert bool(torch.isfinite(runs[True]).all()) and not torch.equal(runs[True], plain)
    assert fwd < 2e-4                       # each forward is within 1e-4 of the reference's decode
    assert err < TRAJ_TOL


def test_synthesize_motion_fused_decode():
    import torch
    from types import SimpleNamespace
    from convofusion_amd.longform import synthesize_motion
    from tests.gpu_helpers import hip_denoiser
    from tests.test_gpu_longform import _inputs, _sched
    U, W, n, seed = 2, 3, 4, 17
    mems, masks = _inputs(U * W, seed)
    model = SimpleNamespace(vae=_model(), denoiser=hip_denoiser(1234, 1.0), scheduler=_sched("ddpm"), guidance_scale=7.5, clf_guidance_drops=6,
                            do_classifier_free_guidance=True,
                            cfg=SimpleNamespace(model=SimpleNamespace(scheduler=SimpleNamespace(num_inference_timesteps=n, eta=0.0))))
    out, win, seq = synthesize_motion(model, mems, masks, n_utterances=U, n_windows=W, seed=seed)
    out_f, win_f, seq_f = synthesize_motion(model, mems, masks, n_utterances=U, n_windows=W, seed=seed, fused_decode=True)
    err = float((out - out_f).abs().max())
    print(f"synthesize_motion fused_decode vs default: max abs {err:.3e}")
    assert torch.equal(win, win_f) and torch.equal(seq, seq_f)
    assert out_f.shape == out.shape and bool(torch.isfinite(out_f).all()) and err < 1e-4
