"""GPU tests of the differentiable VAE decode: cfd_vae_decode_vjp (csrc/vae_dec.hpp) through ``ConvoFusionVae.decode_vjp``, ``decode``
under autograd, and ``edit.pose_keyframe_loss`` in the loss-guided loop.

The gradient is measured against the reference's float64 autograd gradient (tests/golden/vae_decode_vjp.npz); the bar of every case is
8 x the distance of the reference's own float32 autograd gradient from it (the file's yardstick): relative L2 and worst 128-wide row.
Measured on an MI355X (d_z: relative L2 / worst row, as a multiple of the yardstick):
    tiny    7.6e-07 / 1.2e-06   (1.25 x / 1.16 x)        single  9.1e-07 / 1.5e-06   (1.13 x / 1.26 x)
    ragged  1.3e-06 / 2.4e-06   (1.23 x / 1.00 x)        long    3.1e-06 / 9.0e-06   (0.95 x / 0.90 x)
the forward against the decode golden 4.2e-06 .. 2.3e-05 (gate 1e-4); every stage tap within 2.3 x its case's yardstick.
"""
import ctypes as C
import functools

import numpy as np
import pytest

from oracle import inputs, vae_ref, vae_weights
from tests import vae_vjp_ref as R
from tests.helpers import load_golden
from tests.test_oracle_vae import ABL, KW

pytestmark = pytest.mark.gpu

GATE = 8.0
NAMES = tuple(R.CASES)


@functools.lru_cache(maxsize=None)
def _model():
    import torch
    from convofusion_amd.vae import ConvoFusionVae
    m = ConvoFusionVae(ablation=ABL, **KW)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in vae_weights.make_state_dict().items()}, strict=True)
    return m.cuda().eval()


@functools.lru_cache(maxsize=None)
def _golden():
    return load_golden("vae_decode_vjp")


@functools.lru_cache(maxsize=None)
def _restated(name):
    """(feats, d_z, taps) of the float64 restatement, computed once per case."""
    z, lens, d = R.case_inputs(name)
    return R.decode_vjp(vae_weights.make_state_dict(), z, lens, d)


@functools.lru_cache(maxsize=None)
def _device_result(name):
    """(feats, d_z) of one decode_vjp call on the case, as numpy arrays; shared by the tests that only read them."""
    import torch
    z, lens, d = R.case_inputs(name)
    feats, d_z = _model().decode_vjp(torch.from_numpy(z).cuda(), lens, torch.from_numpy(d).cuda())
    return feats.cpu().numpy(), d_z.cpu().numpy()


def _dev(name):
    import torch
    z, lens, d = R.case_inputs(name)
    return torch.from_numpy(z).cuda(), lens, torch.from_numpy(d).cuda()


def _read(what, numel):
    import torch
    from convofusion_amd import _lib
    from convofusion_amd.conditioning import _engine_handle
    t = torch.empty(numel, device="cuda")
    _lib.check(_lib.load().cfd_debug_read(_engine_handle(t.device), what.encode(), C.c_void_p(t.data_ptr()), numel))
    return t.cpu().numpy()


@pytest.mark.parametrize("name", NAMES)
def test_gradient_matches_the_reference_float64_autograd(name):
    got = _device_result(name)[1]
    want, yard = _golden()[name + ".grad"], _golden()[name + ".yard"]
    rel, row = R.errors(got, want)
    print(f"{name}: d_z vs float64 autograd rel L2 {rel:.3e} worst row {row:.3e}; yardstick {yard[0]:.3e} {yard[1]:.3e} "
          f"({rel / yard[0]:.2f} x, {row / yard[1]:.2f} x)")
    assert np.isfinite(got).all()
    assert rel <= GATE * yard[0] and row <= GATE * yard[1]


@pytest.mark.parametrize("name", NAMES)
def test_forward_matches_the_decode_golden_and_pads_with_zeros(name):
    """ragged / single / long: the reference's decode (vae_decode.npz); tiny has no entry there: oracle.vae_ref, which that file pins."""
    z, lens, _ = R.case_inputs(name)
    got = _device_result(name)[0]
    G = load_golden("vae_decode")
    want = G[name] if name in G else vae_ref.decode(vae_weights.make_state_dict(), z, lens)
    err = float(np.abs(got - want).max())
    print(f"{name}: decode_vjp's forward vs the decode golden: max abs {err:.3e}")
    assert got.shape == want.shape and err < 1e-4
    for b, n in enumerate(lens):
        assert not got[b, n:].any()


@pytest.mark.parametrize("name", NAMES)
def test_stage_taps_match_the_restatement(name):
    """The running gradient entering each layer and each layer's memory-side contribution, against the float64 restatement."""
    import torch
    z, lens, d = _dev(name)
    m = _model()
    m.decode_vjp(z, lens, d)
    torch.cuda.synchronize()
    taps, yard = _restated(name)[2], _golden()[name + ".yard"]
    bs, nc, nfr = z.shape[1], z.shape[2], max(lens)
    fp = (nfr + 15) // 16 * 16
    info = _read("vae.info", 2)
    assert int(info[1]) == fp and 0 < int(info[0]) <= 36          # a few dozen launches
    worst = {}
    for l in reversed(range(m.num_layers)):
        g = _read(f"vae.g.{l}", 2 * bs * fp * 128).reshape(2, bs, fp, 128)[:, :, :nfr]
        dz = _read(f"vae.dz.{l}", 2 * bs * 16 * 128).reshape(2, bs, 16, 128)[:, :, :nc]
        want_g = np.stack([taps[f"g.{s}.{l}"].transpose(1, 0, 2) for s in range(2)])
        want_dz = np.stack([taps[f"dz.{s}.{l}"] for s in range(2)])
        for b, n in enumerate(lens):
            assert not g[:, b, n:].any() and not want_g[:, b, n:].any()      # frames beyond the length carry no gradient
        worst[f"g.{l}"], worst[f"dz.{l}"] = R.errors(g, want_g), R.errors(dz, want_dz)
    for k, (rel, row) in worst.items():
        print(f"{name} {k}: rel L2 {rel:.3e} ({rel / yard[0]:.2f} x) worst row {row:.3e} ({row / yard[1]:.2f} x)")
    for k, (rel, row) in worst.items():
        assert rel <= GATE * yard[0] and row <= GATE * yard[1], k


@pytest.mark.parametrize("name", ["tiny", "ragged", "long"])
def test_exact_properties(name):
    import torch
    m = _model()
    z, lens, d = _dev(name)
    feats, d_z = m.decode_vjp(z, lens, d)
    feats2, d_z2 = m.decode_vjp(z, lens, d)
    assert torch.equal(d_z, d_z2) and torch.equal(feats, feats2)                  # no atomics: the same bits
    none, d_z3 = m.decode_vjp(z, lens, d, want_out=False)
    assert none is None and torch.equal(d_z, d_z3)
    # a cotangent in one sequence only
    b0 = len(lens) - 1
    d1 = torch.zeros_like(d)
    d1[b0] = d[b0]
    g1 = m.decode_vjp(z, lens, d1)[1]
    assert torch.equal(g1[:, b0], d_z[:, b0]) and float(g1[:, b0].abs().max()) > 0
    assert not g1[:, :b0].any()
    # a cotangent on the hands features only
    dh = d.clone()
    dh[..., :69] = 0
    gh = m.decode_vjp(z, lens, dh)[1]
    assert not gh[0].any() and torch.equal(gh[1], d_z[1])
    # the cotangent beyond each length is not read
    dj = d.clone()
    for b, n in enumerate(lens):
        dj[b, n:] = 1e30
    assert torch.equal(m.decode_vjp(z, lens, dj)[1], d_z)


def test_decode_under_autograd_is_the_same_forward_with_decode_vjp_behind_it():
    import torch
    from convofusion_amd.vae import attach_hip_decode
    m = _model()
    z, lens, c = _dev("ragged")
    with torch.no_grad():
        plain = m.decode(z, lens)
    assert plain.grad_fn is None and m.decode(z, lens).grad_fn is None          # a z that needs no gradient: today's call
    zg = z.clone().requires_grad_()
    feats = m.decode(zg, lens)
    assert feats.grad_fn is not None and torch.equal(feats, plain)
    (g,) = torch.autograd.grad((feats * c).sum(), zg)
    assert torch.equal(g, m.decode_vjp(z, lens, c)[1])
    with torch.no_grad():
        assert m.decode(zg, lens).grad_fn is None
    # attach_hip_decode inherits it (a second mirror stands in for the reference class, as in test_gpu_vae.py)
    from convofusion_amd.vae import ConvoFusionVae
    host = ConvoFusionVae(ablation=ABL, **KW)
    host.load_state_dict(m.state_dict(), strict=True)
    host = host.cuda().eval()
    host.mlp_dist, host.pe_type = False, "convofusion"
    host.body_decoder.middle_block.normalize_before = True
    mirror = attach_hip_decode(host)
    zg2 = z.clone().requires_grad_()
    f2 = host.decode(zg2, lens)
    assert mirror is not host and torch.equal(f2, plain)
    (g2,) = torch.autograd.grad((f2 * c).sum(), zg2)
    assert torch.equal(g2, g)


# ----------------------------------------------------------------------------- with the loop
def _loop_case():
    """B = 1, L = 16, the row-tile-eligible memories of test_gpu_denoise_vjp.py's row_maps case as a replicated 7-chunk batch."""
    from tests.gpu_helpers import to_dev
    cb = inputs.make_cfg_batch(seed=43, B=1, L=16, S=(24, 161, 24, 8, 1), pad_tail=(5, 0, 7, 0, 0))
    mems = [to_dev(v) for v in cb["memories"]]
    masks = {k: to_dev(v) for k, v in cb["masks"].items()}
    rng = np.random.Generator(np.random.PCG64(4343))
    target = to_dev(rng.standard_normal((1, 128, 189), dtype=np.float32))
    fmask = np.zeros((1, 128), dtype=bool)
    fmask[0, [5, 73, 127]] = True
    cmask = np.zeros(189, dtype=bool)
    cmask[60:100] = True                                      # a wrist's worth of body columns and some fingers
    return cb, mems, masks, target, to_dev(fmask), to_dev(cmask)


def test_pose_keyframe_loss_in_the_guided_loop():
    import torch
    from convofusion_amd import edit, sampler, scheduler
    from convofusion_amd.sampler import SamplingRun
    from tests.gpu_helpers import SCHED_KW, hip_denoiser, to_dev
    vae, m = _model(), hip_denoiser(1234, 1.0)
    cb, mems, masks, target, fmask, cmask = _loop_case()
    B, L, N, scale, step, G = 1, 16, 3, 7.5, 40.0, 7
    sch = scheduler.DDIMScheduler(**SCHED_KW)
    kw = dict(B=B, L=L, num_inference_steps=N, guidance_scale=scale, eta=0.0, init_latents=to_dev(cb["init"]))
    loss = edit.pose_keyframe_loss(vae, target, fmask, cmask)
    plain = sampler.sample(m, sch, mems, masks, **kw)
    assert torch.equal(sampler.sample_with_loss_guidance(m, sch, mems, masks, loss, 0.0, **kw), plain)
    got = sampler.sample_with_loss_guidance(m, sch, mems, masks, loss, step, **kw)
    assert not torch.equal(got, plain) and bool(torch.isfinite(got).all())

    # the same loop by hand: denoiser.vjp and vae.decode_vjp called explicitly, torch autograd only over the element-wise glue
    chunks = sampler.guided_chunks(sampler.default_guidance_weights(G, scale))
    states, smasks = sampler.guidance_chunk_rows(mems, masks, chunks, G, B)
    states = [s.detach().contiguous() for s in states]
    w = torch.tensor(sampler.default_guidance_weights(G, scale), dtype=torch.float32, device="cuda").expand(B, 8)
    acp = sch.alphas_cumprod.detach().to("cpu", torch.float64)
    lens = [128]
    n_sel = int(fmask.sum().item()) * int(cmask.sum().item())
    sch.set_timesteps(N)
    with SamplingRun(m, sch, mems, masks, B, L, N, guidance_scale=scale, guidance_chunks=G, eta=0.0, init_latents=kw["init_latents"]) as run:
        for i, t in enumerate(run.timesteps):
            run.inpaint()
            x = run.read()
            rows = x.repeat(len(chunks), 1, 1)
            with torch.no_grad():
                out, _ = m(sample=rows, timestep=int(t), encoder_hidden_states=states, mem_mask_dict=smasks, side_engine=True)
            xl, ol = x.detach().clone().requires_grad_(True), out.detach().clone().requires_grad_(True)
            with torch.enable_grad():
                e = ol.view(len(chunks), B, L, 128)
                eps = e[0]
                for n, c in enumerate(chunks[1:], start=1):
                    eps = eps + w[:, c].view(B, 1, 1) * (e[n] - e[0])
                a_t = float(acp[int(t)])
                x0 = (xl - (1.0 - a_t) ** 0.5 * eps) / a_t ** 0.5
                zv = edit.loop_to_vae(x0)
                with torch.no_grad():
                    feats = vae.decode(zv.detach(), lens)
                fl = feats.detach().clone().requires_grad_(True)
                wm = (fmask.unsqueeze(-1) & cmask).to(fl.dtype)
                dd = (fl - target) * wm
                (d_feats,) = torch.autograd.grad((dd * dd).sum() / n_sel, fl)
                d_z = vae.decode_vjp(zv.detach(), lens, d_feats, want_out=False)[1]
                g_direct, d_out = torch.autograd.grad(zv, [xl, ol], d_z)
            g_rows = m.vjp(rows, int(t), states, smasks, d_out, side_engine=True)[1]
            xr = x.detach().clone().requires_grad_(True)
            (g_via,) = torch.autograd.grad(xr.repeat(len(chunks), 1, 1), xr, g_rows)
            run.write(x.detach() - step * (g_direct + g_via))
            run.steps(1)
        by_hand = run.read()
    assert torch.equal(got, by_hand)


def test_decode_vjp_between_two_steps_leaves_an_open_run_s_bits():
    import torch
    from convofusion_amd import scheduler
    from convofusion_amd.sampler import SamplingRun
    from tests.gpu_helpers import SCHED_KW, hip_denoiser
    vae, m = _model(), hip_denoiser(1234, 1.0)
    cb, mems, masks, _, _, _ = _loop_case()
    sch = scheduler.DDIMScheduler(**SCHED_KW)
    z, lens, d = _dev("single")

    def go(interleave):
        grads = []
        with SamplingRun(m, sch, mems, masks, 1, 16, 4, guidance_scale=7.5, eta=0.0, seed=3) as run:
            for _ in range(4):
                run.steps(1)
                if interleave:
                    grads.append(vae.decode_vjp(z, lens, d)[1])
            return run.read(), grads

    plain, _ = go(False)
    mixed, grads = go(True)
    assert torch.equal(plain, mixed)
    assert all(torch.equal(g, grads[0]) for g in grads) and float(grads[0].abs().max()) > 0
