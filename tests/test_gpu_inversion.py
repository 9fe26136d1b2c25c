"""-m gpu: DDIM inversion in the captured loop (scheduler kind 3, cfd_sample_begin_invert, ``sampler.invert``) and the anchored DDIM
regeneration over its trajectory (cfd_sample_begin_anchored, ``sample(..., anchor_trajectory=, keep_mask=)``, ``edit.reperform_motion``).

The stand-alone step against the numpy oracle (tests/inversion_ref.py), the fused loop against a host loop of Denoiser.forward and the
mirror's step, against the trajectories made with the REFERENCE denoiser (tests/golden/traj_invert_*.npz, traj_anchored_*.npz,
make_golden_inversion.py), the recorded ring against a plain run, the anchoring's exact values, the round trip, the ABI's refusals and
``reperform_motion`` against its steps done by hand.  Errors are printed."""
import ctypes as C

import numpy as np
import pytest

from oracle import inputs, philox_ref, vae_weights
from tests import inversion_ref
from tests.helpers import load_golden, rel_l2

pytestmark = pytest.mark.gpu
TRAJ_TOL = 1e-3          # as tests/test_gpu_edit.py
SMALL = ((6, 20, 6, 8, 1), (2, 0, 1, 0, 0))
# Round trip (invert at N = 50, DDIM back under the same conditioning and guidance, nothing kept): relative L2 distance of the result from
# the source, measured on an MI355X with the seeded weights: 9.88e-2 at the small shape, 9.96e-2 at the headline shape (DESIGN.md section
# 1.4; the run is deterministic).  The bounds leave ~10 % headroom over the measurement.
ROUND_TRIP_BOUND = {"small": 0.11, "headline": 0.11}


def _sched(kind, **kw):
    from convofusion_amd import scheduler
    from tests.gpu_helpers import SCHED_KW
    base = dict(SCHED_KW, clip_sample=False)
    base.update(kw)
    return scheduler.DDIMInverseScheduler(**base) if kind == "inverse" else scheduler.DDIMScheduler(**base)


def _inputs(B, L, S, pad, seed):
    from tests.gpu_helpers import to_dev
    cb = inputs.make_cfg_batch(seed=seed, B=B, L=L, S=S, pad_tail=pad)
    return [to_dev(x) for x in cb["memories"]], {k: to_dev(v) for k, v in cb["masks"].items()}


def _source(B, seed, L=16):
    from tests.gpu_helpers import to_dev
    return to_dev((0.8 * philox_ref.normal_tensor(seed, 0, range(B), 2, L)).astype(np.float32))


def test_standalone_step_matches_the_oracle():
    """DDIMInverseScheduler.step (cfd_scheduler_step, kind 3) against DDIMInverseRef.step on the mirror's own table, at the first step
    (final_alpha), inside the schedule and at its end, with and without set_alpha_to_one."""
    import torch
    for one in (True, False):
        s = _sched("inverse", set_alpha_to_one=one)
        s.set_timesteps(20)
        ref = inversion_ref.DDIMInverseRef(set_alpha_to_one=one)
        ref.set_timesteps(20)
        ref.alphas_cumprod = s.alphas_cumprod.numpy()
        ref.final_alpha_cumprod = np.float32(s.final_alpha_cumprod)
        g = torch.Generator().manual_seed(4)
        x = torch.randn((3, 16, 128), generator=g)
        eps = torch.randn((3, 16, 128), generator=g)
        for t in (0, 50, 500, 950):
            out = s.step(eps.cuda(), t, x.cuda())
            want = ref.step(eps.numpy(), t, x.numpy())
            e = rel_l2(out.prev_sample.cpu().numpy(), want)
            print(f"set_alpha_to_one={one} t={t}: {e:.2e}")
            assert e < 1e-6, (one, t, e)
            assert torch.isfinite(out.pred_original_sample).all()


def _host_loop(m, s, n, x, mems, masks, factors):
    import torch
    s.set_timesteps(n)
    with torch.no_grad():
        for t in s.timesteps:
            out, _ = m(torch.cat([x] * 7), int(t), mems, mem_mask_dict=masks)
            u, *c = out.chunk(7)
            acc = None
            for k in range(6):
                if factors[k] != 0.0:
                    term = float(factors[k]) * (c[k] - u)
                    acc = term if acc is None else acc + term
            x = s.step(u + acc, t, x).prev_sample
    return x


@pytest.mark.parametrize("weights", ["conditional", "reference"])
def test_fused_inversion_equals_host_loop_of_the_mirror(weights):
    """The captured kind-3 loop against a host loop of Denoiser.forward, the same weighted combine and the mirror's stand-alone ``step``,
    on the same source: bit for bit.  conditional: ``invert``'s default (w_all = 1 at scale 1; 2 of 7 chunks evaluated); reference: the
    reference's weights at 7.5 (5 of 7)."""
    import torch
    from convofusion_amd.sampler import INVERSION_WEIGHTS, REFERENCE_MODALITY_WEIGHTS, MODALITY_NAMES, SamplingRun, invert
    from tests.gpu_helpers import hip_denoiser
    B, L, n, seed = 2, 16, 12, 5
    mems, masks = _inputs(B, L, *SMALL, seed)
    src = _source(B, seed)
    m = hip_denoiser(1234, 1.0)
    w, scale = (INVERSION_WEIGHTS, 1.0) if weights == "conditional" else (REFERENCE_MODALITY_WEIGHTS, 7.5)
    fused = invert(m, _sched("inverse"), mems, masks, source_latents=src, num_inference_steps=n, guidance_scale=scale, modality_weights=w)
    with SamplingRun(m, _sched("inverse"), mems, masks, B, L, n, guidance_scale=scale, init_latents=src, modality_weights=w) as run:
        assert run.chunks_evaluated == (2 if weights == "conditional" else 6)
    host = _host_loop(m, _sched("inverse"), n, src.clone(), mems, masks, [float(np.float32(scale * w[k])) for k in MODALITY_NAMES])
    e = rel_l2(fused.cpu().numpy(), host.cpu().numpy())
    print(f"{weights}: fused vs host loop {e:.2e}, max abs {float((fused - host).abs().max()):.2e}")
    assert torch.isfinite(fused).all() and torch.equal(fused, host), e


def _anchored_case():
    g = load_golden("traj_anchored_ddim10")
    m = [int(v) for v in g["meta"]]
    return g, m[0], m[1], tuple(m[2:7]), tuple(m[7:12]), m[12]


@pytest.mark.parametrize("n", [10, 50])
def test_fused_inversion_matches_reference_trajectory(n):
    """Every recorded slot of the N = 10 / 50 inversion against the restated inversion on the REFERENCE denoiser."""
    import torch
    from convofusion_amd.sampler import invert
    from tests.gpu_helpers import hip_denoiser, to_dev
    g = load_golden(f"traj_invert_ddim{n}")
    meta = [int(v) for v in g["meta"]]
    B, L, S, pad, seed = meta[0], meta[1], tuple(meta[2:7]), tuple(meta[7:12]), meta[12]
    mems, masks = _inputs(B, L, S, pad, seed)
    lat, ring = invert(hip_denoiser(1234, 1.0), _sched("inverse"), mems, masks, source_latents=to_dev(g["source"]), num_inference_steps=n,
                       return_trajectory=True)
    assert tuple(ring.shape) == (n + 1, B, L, 128) and torch.equal(ring[n], lat) and torch.equal(ring[0].cpu(), torch.from_numpy(g["source"]))
    errs = {int(k[4:]): rel_l2(ring[int(k[4:])].cpu().numpy(), g[k]) for k in g.files if k.startswith("slot")}
    errs["final"] = rel_l2(lat.cpu().numpy(), g["latents"])
    print(f"invert N={n}", {k: f"{v:.2e}" for k, v in errs.items()})
    assert len(errs) >= 6 and all(v < TRAJ_TOL for v in errs.values()), errs


def test_anchored_regeneration_matches_reference_trajectory():
    """The anchored DDIM-10 regeneration from the reference inversion's ring (traj_invert_ddim10) under another conditioning, a partial keep
    mask, reference combine at 7.5: every snapshot against the restated loop on the REFERENCE denoiser."""
    from convofusion_amd.sampler import SamplingRun
    from tests.gpu_helpers import hip_denoiser, to_dev
    g, B, L, S, pad, seed = _anchored_case()
    n = int(g["n"])
    inv = load_golden("traj_invert_ddim10")
    ring = to_dev(np.stack([inv[f"slot{j}"] for j in range(n + 1)]))
    mems, masks = _inputs(B, L, S, pad, seed)
    run = SamplingRun(hip_denoiser(1234, 1.0), _sched("ddim"), mems, masks, B, L, n, guidance_scale=7.5, init_latents=ring[n],
                      anchor_trajectory=ring, keep_mask=to_dev(g["keep"]))
    errs = {}
    for k in sorted(int(f[4:]) for f in g.files if f.startswith("step")):
        run.steps(k - run.position)
        errs[k] = rel_l2(run.read().cpu().numpy(), g[f"step{k}"])
    errs["final"] = rel_l2(run.read(close=True).cpu().numpy(), g["latents"])
    print("anchored", {k: f"{v:.2e}" for k, v in errs.items()})
    assert all(v < TRAJ_TOL for v in errs.values()), errs


def test_ring_slots_equal_a_plain_run_step_by_step():
    """Slot j of the recorded trajectory = ``run.steps(j); run.read()`` of a kind-3 run without one, bit for bit, for every j."""
    import torch
    from convofusion_amd.sampler import INVERSION_WEIGHTS, SamplingRun, invert
    from tests.gpu_helpers import hip_denoiser
    B, L, n, seed = 3, 16, 10, 12
    mems, masks = _inputs(B, L, (24, 161, 24, 8, 1), (2, 3, 0, 0, 0), seed)
    src = _source(B, seed)
    m = hip_denoiser(1234, 1.0)
    lat, ring = invert(m, _sched("inverse"), mems, masks, source_latents=src, num_inference_steps=n, return_trajectory=True)
    with SamplingRun(m, _sched("inverse"), mems, masks, B, L, n, guidance_scale=1.0, init_latents=src, modality_weights=INVERSION_WEIGHTS) as run:
        assert torch.equal(run.read(), ring[0])
        for j in range(1, n + 1):
            run.steps(1)
            assert torch.equal(run.read(), ring[j]), j
    assert torch.equal(ring[n], lat) and torch.isfinite(ring).all()


def test_full_mask_anchors_every_kept_token_exactly():
    """Every token kept: after ``run.inpaint()`` at iteration i the latents are ring[N - i] exactly (the read-back of
    test_gpu_edit.test_inpaint_sets_the_kept_tokens_exactly); with a partial mask the other tokens are untouched."""
    import torch
    from convofusion_amd.sampler import SamplingRun, invert
    from tests.gpu_helpers import hip_denoiser
    B, L, n, seed = 2, 16, 10, 8
    mems, masks = _inputs(B, L, *SMALL, seed)
    m = hip_denoiser(1234, 1.0)
    inv, ring = invert(m, _sched("inverse"), mems, masks, source_latents=_source(B, seed), num_inference_steps=n, return_trajectory=True)
    g = torch.Generator().manual_seed(seed)
    for keep in (torch.ones((B, L), dtype=torch.bool).cuda(), (torch.rand((B, L), generator=g) < 0.5).cuda()):
        run = SamplingRun(m, _sched("ddim"), mems, masks, B, L, n, guidance_scale=7.5, init_latents=inv, anchor_trajectory=ring, keep_mask=keep)
        checked = 0
        for pos in (0, 1, 4, 9):
            run.steps(pos - run.position)
            before = run.read()
            run.inpaint()
            after = run.read()
            assert torch.equal(after[keep], ring[n - pos][keep]), pos
            assert torch.equal(after[~keep], before[~keep]), pos
            checked += 1
            run.steps(1)
            assert torch.isfinite(run.read()).all()
        run.close()
        assert checked == 4
    # without inpaint(): the captured iteration does the overwrite itself -- with everything kept the run ends one step past ring[1]
    run = SamplingRun(m, _sched("ddim"), mems, masks, B, L, n, guidance_scale=7.5, init_latents=inv, anchor_trajectory=ring,
                      keep_mask=torch.ones((B, L), dtype=torch.bool).cuda())
    run.steps(n - 1)
    run.inpaint()
    assert torch.equal(run.read(), ring[1])
    run.close()


def test_empty_mask_is_bit_identical_to_plain_ddim():
    """An anchored run with nothing kept (an all-zero mask, or none) computes the plain DDIM run from the same initial latents."""
    import torch
    from convofusion_amd.sampler import sample, invert
    from tests.gpu_helpers import hip_denoiser
    B, L, n, seed = 2, 16, 10, 9
    mems, masks = _inputs(B, L, *SMALL, seed)
    m = hip_denoiser(1234, 1.0)
    inv, ring = invert(m, _sched("inverse"), mems, masks, source_latents=_source(B, seed), num_inference_steps=n, return_trajectory=True)
    kw = dict(B=B, L=L, num_inference_steps=n, guidance_scale=7.5, init_latents=inv, skip_zero_weight_chunks=True)
    plain = sample(m, _sched("ddim"), mems, masks, **kw)
    zero = sample(m, _sched("ddim"), mems, masks, anchor_trajectory=ring, keep_mask=torch.zeros((B, L), dtype=torch.bool).cuda(), **kw)
    none = sample(m, _sched("ddim"), mems, masks, anchor_trajectory=ring, **kw)
    assert torch.isfinite(plain).all() and torch.equal(plain, zero) and torch.equal(plain, none)


def test_sample_with_the_inverse_scheduler_is_invert():
    import torch
    from convofusion_amd.sampler import INVERSION_WEIGHTS, sample, invert
    from tests.gpu_helpers import hip_denoiser
    B, L, n, seed = 2, 16, 10, 3
    mems, masks = _inputs(B, L, *SMALL, seed)
    src = _source(B, seed)
    m = hip_denoiser(1234, 1.0)
    a = invert(m, _sched("inverse"), mems, masks, source_latents=src, num_inference_steps=n)
    b = sample(m, _sched("inverse"), mems, masks, B=B, L=L, num_inference_steps=n, guidance_scale=1.0, init_latents=src,
               modality_weights=INVERSION_WEIGHTS)
    assert torch.equal(a, b)


@pytest.mark.parametrize("shape", ["small", "headline"])
def test_round_trip_lands_near_the_source(shape):
    """Invert at N = 50, then DDIM back under the same conditioning and the same (conditional-only) guidance with nothing kept: the
    distance from the source is measured (printed) and bounded by ROUND_TRIP_BOUND, set from an MI355X measurement."""
    import torch
    from convofusion_amd.sampler import INVERSION_WEIGHTS, sample, invert
    from tests.gpu_helpers import hip_denoiser
    n = 50
    if shape == "small":
        B, L, S, pad, seed = 2, 16, SMALL[0], SMALL[1], 21
    else:
        B, L, S, pad, seed = 32, 196, (32, 1500, 32, 8, 1), (8, 100, 0, 0, 0), 22
    mems, masks = _inputs(B, L, S, pad, seed)
    src = _source(B, seed, L)
    m = hip_denoiser(1234, 1.0)
    inv = invert(m, _sched("inverse"), mems, masks, source_latents=src, num_inference_steps=n)
    back = sample(m, _sched("ddim"), mems, masks, B=B, L=L, num_inference_steps=n, guidance_scale=1.0, init_latents=inv,
                  modality_weights=INVERSION_WEIGHTS)
    e = rel_l2(back.cpu().numpy(), src.cpu().numpy())
    e_inv = rel_l2(inv.cpu().numpy(), src.cpu().numpy())
    print(f"round trip {shape}: |back - src| / |src| = {e:.3e} (|inverted - src| / |src| = {e_inv:.3e})")
    assert torch.isfinite(back).all() and e < ROUND_TRIP_BOUND[shape], e


def test_abi_refusals():
    """Kind 3 with preseq, a dynamic memory, an edit, a WEG update (cfd_sample_write), eta != 0, clip_sample = 1, a descending table; an
    inversion entry with another kind or no trajectory; an anchored run with a ring from another shape, another kind, eta != 0 or
    clipping: CFD_E_ARG.  Good calls afterwards open runs on the same handle."""
    import torch
    from convofusion_amd import _lib
    from convofusion_amd.sampler import SamplingRun
    from tests.gpu_helpers import hip_denoiser
    B, L, n = 1, 16, 10
    mems, masks = _inputs(B, L, *SMALL, 4)
    src = _source(B, 4)
    m = hip_denoiser(1234, 1.0)
    run = SamplingRun(m, _sched("inverse"), mems, masks, B, L, n, guidance_scale=1.0, init_latents=src)
    assert run._args.scheduler == 3
    lat = run.read()
    assert lib_call_write(run, lat) == -1           # WEG's update of the open inversion run
    run.close()
    lib = _lib.load()
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    traj = torch.empty((n + 1, B, L, 128), device="cuda")
    preseq = torch.zeros((B, 4, 128), device="cuda")
    ts_desc = (C.c_int32 * n)(*[900 - 100 * i for i in range(n)])
    g_eval = C.c_int(-7)

    def args(**kw):
        a = _lib.SampleArgs.from_buffer_copy(run._args)
        for k, v in kw.items():
            setattr(a, k, v)
        return a

    def invert_call(a, t=traj):
        return lib.cfd_sample_begin_invert(run.handle, C.byref(a), C.c_void_p(t.data_ptr()) if t is not None else None, None, 1,
                                           C.byref(g_eval), stream)

    e = _lib.EditArgs()
    e.source, e.keep, e.first_iteration = src.data_ptr(), None, 0
    cases = [("preseq", lambda: invert_call(args(preseq=preseq.data_ptr(), preseq_len=4))),
             ("dynamic memory", lambda: invert_call(args(dynamic_memory_mask=1))),
             ("eta", lambda: invert_call(args(eta=0.5))),
             ("clip", lambda: invert_call(args(clip_sample=1))),
             ("descending table", lambda: invert_call(args(timesteps=C.cast(ts_desc, C.c_void_p)))),
             ("no table", lambda: invert_call(args(timesteps=None))),
             ("NULL trajectory", lambda: invert_call(args(), None)),
             ("invert with kind 1", lambda: invert_call(args(scheduler=1))),
             ("edit", lambda: lib.cfd_sample_begin_edit(run.handle, C.byref(args()), C.byref(e), None, 1, C.byref(g_eval), stream)),
             ("plain begin, eta", lambda: lib.cfd_sample_begin(run.handle, C.byref(args(eta=0.5)), stream))]
    for what, call in cases:
        rc = call()
        print(what, "->", rc, lib.cfd_last_error().decode())
        assert rc == -1, what
    assert invert_call(args()) == 0 and g_eval.value == 7
    assert lib.cfd_sample_steps(run.handle, n) == 0
    out = torch.empty((B, L, 128), device="cuda")
    assert lib.cfd_sample_read(run.handle, C.c_void_p(out.data_ptr()), 1) == 0
    assert torch.equal(out, traj[n]) and torch.equal(traj[0], src)
    # anchored runs
    ddim = SamplingRun(m, _sched("ddim"), mems, masks, B, L, n, guidance_scale=7.5, init_latents=out)
    ddim.close()

    def anchored(steps=n, b=B, l_=L, **kw):
        a = _lib.SampleArgs.from_buffer_copy(ddim._args)
        for k, v in kw.items():
            setattr(a, k, v)
        an = _lib.AnchorArgs()
        an.trajectory, an.steps, an.B, an.L, an.keep = traj.data_ptr(), steps, b, l_, None
        return lib.cfd_sample_begin_anchored(ddim.handle, C.byref(a), C.byref(an), None, 1, C.byref(g_eval), stream)

    for what, kw in (("steps", dict(steps=n + 1)), ("B", dict(b=B + 1)), ("L", dict(l_=L - 2)), ("kind 0", dict(scheduler=0)),
                     ("eta", dict(eta=0.5)), ("clip", dict(clip_sample=1)), ("preseq", dict(preseq=preseq.data_ptr(), preseq_len=4))):
        rc = anchored(**kw)
        print("anchored", what, "->", rc, lib.cfd_last_error().decode())
        assert rc == -1, what
    assert anchored() == 0
    assert lib.cfd_sample_steps(ddim.handle, n) == 0
    assert lib.cfd_sample_read(ddim.handle, C.c_void_p(out.data_ptr()), 1) == 0 and torch.isfinite(out).all()


def lib_call_write(run, lat):
    from convofusion_amd import _lib
    return _lib.load().cfd_sample_write(run.handle, C.c_void_p(lat.data_ptr()))


def _vae():
    import torch
    from convofusion_amd.vae import ConvoFusionVae
    from tests.test_vae_encode_host import ABL, KW
    v = ConvoFusionVae(ablation=ABL, **KW)
    v.load_state_dict({k: torch.from_numpy(a) for k, a in vae_weights.make_state_dict().items()}, strict=True)
    return v.cuda().eval()


def test_reperform_motion_equals_its_steps_by_hand():
    """reperform_motion = HIP encode (posterior mean) -> vae_to_loop -> invert (source conditioning) -> anchored DDIM (target conditioning)
    -> loop_to_vae -> HIP decode, bit for bit, on seeded VAE and denoiser weights; the DDIM schedulers are built from the model DDPM
    scheduler's betas."""
    import torch
    from types import SimpleNamespace
    from convofusion_amd import scheduler
    from convofusion_amd.edit import loop_to_vae, reperform_motion, token_mask, vae_to_loop
    from convofusion_amd.sampler import invert, sample
    from tests.gpu_helpers import SCHED_KW, hip_denoiser
    B, n, seed = 2, 10, 17
    src_c, src_m = _inputs(B, 16, *SMALL, seed)
    tgt_c, tgt_m = _inputs(B, 16, *SMALL, seed + 1)
    model = SimpleNamespace(vae=_vae(), denoiser=hip_denoiser(1234, 1.0),
                            scheduler=scheduler.DDPMScheduler(variance_type="fixed_small", **SCHED_KW), guidance_scale=7.5,
                            clf_guidance_drops=6, do_classifier_free_guidance=True)
    g = torch.Generator().manual_seed(seed)
    feats = (0.5 * torch.randn((B, 128, 189), generator=g)).cuda()
    lengths = [128, 128]
    keep = token_mask(B, keep_frames=[(0, 32)], keep_parts=("body",)).cuda()
    out, lat, inv = reperform_motion(model, feats, lengths, src_c, tgt_c, source_masks=src_m, target_masks=tgt_m, num_inference_steps=n,
                                     keep_mask=keep)
    _, dist, _ = model.vae.encode(feats, lengths)
    src = vae_to_loop(dist.mean.reshape(2, B, 8, 128))
    kw = dict(SCHED_KW, clip_sample=False)
    want_inv, ring = invert(model.denoiser, scheduler.DDIMInverseScheduler(**kw), src_c, src_m, source_latents=src, num_inference_steps=n,
                            return_trajectory=True)
    want_lat = sample(model.denoiser, scheduler.DDIMScheduler(**kw), tgt_c, tgt_m, B=B, L=16, num_inference_steps=n, guidance_scale=7.5,
                      init_latents=want_inv, skip_zero_weight_chunks=True, anchor_trajectory=ring, keep_mask=keep)
    want = model.vae.decode(loop_to_vae(want_lat), lengths)
    assert tuple(out.shape) == (B, 128, 189) and tuple(lat.shape) == (B, 16, 128) and tuple(inv.shape) == (B, 16, 128)
    assert torch.equal(inv, want_inv) and torch.equal(lat, want_lat) and torch.equal(out, want)
    assert torch.isfinite(out).all()
