"""-m gpu: the captured sampling loop with DPM-Solver++ (2M) (scheduler kind 2, convofusion_amd.scheduler.DPMSolverMultistepScheduler)
against trajectories made with the REFERENCE denoiser and the restated diffusers 0.14.0 solver (tests/golden/traj_*dpmpp*.npz,
make_golden_dpmsolver.py), against a host loop of the mirror's own ``step``, and through the ABI's argument checks.

Tolerance on latents: 1e-3 relative L2 (BASELINE.json north_star), as for the DDPM / DDIM loops; the errors are printed."""
import ctypes as C

import numpy as np
import pytest

from oracle import inputs, philox_ref
from tests.helpers import load_golden, rel_l2

pytestmark = pytest.mark.gpu
TRAJ_TOL = 1e-3
SCHED_KW = dict(num_train_timesteps=1000, beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear")


def _sched():
    from convofusion_amd.scheduler import DPMSolverMultistepScheduler
    return DPMSolverMultistepScheduler(**SCHED_KW)


def _case(name):
    g = load_golden("traj_" + name)
    m = [int(x) for x in g["meta"]]
    B, L, S, pad, n, seed = m[0], m[1], tuple(m[2:7]), tuple(m[7:12]), m[12], m[13]
    return g, B, L, S, pad, n, seed


def _inputs(B, L, S, pad, seed):
    from tests.gpu_helpers import to_dev
    cb = inputs.make_cfg_batch(seed=seed, B=B, L=L, S=S, pad_tail=pad)
    return [to_dev(x) for x in cb["memories"]], {k: to_dev(v) for k, v in cb["masks"].items()}


@pytest.mark.parametrize("name", ["dpmpp20_b2", "dpmpp10", "inpaint_dpmpp20"])
def test_fused_loop_matches_reference_trajectory(name):
    """Small goldens (these shapes take the row-tile path): every snapshot and the final latents."""
    from convofusion_amd.sampler import SamplingRun
    from tests.gpu_helpers import hip_denoiser, to_dev
    g, B, L, S, pad, n, seed = _case(name)
    mems, masks = _inputs(B, L, S, pad, seed)
    init = philox_ref.normal_tensor(seed, 0, range(B), 1, L)
    run = SamplingRun(hip_denoiser(1234, 1.0), _sched(), mems, masks, B, L, n, guidance_scale=7.5, init_latents=to_dev(init),
                      preseq=to_dev(g["preseq"]) if "inpaint" in name else None)
    assert run.N == n
    errs = {}
    for k in sorted(int(f[4:]) for f in g.files if f.startswith("step")):
        run.steps(k - run.position)
        errs[k] = rel_l2(run.read().cpu().numpy(), g[f"step{k}"])
    run.steps(n - run.position)
    lat = run.read(close=True).permute(1, 0, 2).cpu().numpy()
    errs["final"] = rel_l2(lat, g["latents"])
    print(name, {k: f"{v:.2e}" for k, v in errs.items()})
    assert np.isfinite(lat).all() and all(v < TRAJ_TOL for v in errs.values()), errs


@pytest.mark.parametrize("variant", ["b32", "b1_shard"])
def test_headline_shape_row_matches_reference(variant):
    """B = 32, L = 196, 1500 audio tokens (the fused cross-attention path): utterance 17 of the B = 32 run, and a one-utterance shard with
    first_utterance = 17, against traj_c2_dpmpp20 (the restated loop on the reference denoiser for that utterance alone)."""
    from convofusion_amd.distributed import shard_cfg_batch
    from convofusion_amd.sampler import SamplingRun
    from tests.gpu_helpers import hip_denoiser, to_dev
    g = load_golden("traj_c2_dpmpp20")
    meta = [int(v) for v in g["meta"]]
    B, L, S, pad, n, seed, u = meta[0], meta[1], tuple(meta[2:7]), tuple(meta[7:12]), meta[12], meta[13], meta[14]
    cb = inputs.make_cfg_batch(seed=seed, B=B, L=L, S=S, pad_tail=pad, uncond_pad_tail=pad)
    mems = [to_dev(x) for x in cb["memories"]]
    masks = {k: to_dev(v) for k, v in cb["masks"].items()}
    m = hip_denoiser(1234, 1.0)
    if variant == "b1_shard":
        mems = [shard_cfg_batch(x, u, u + 1, B) for x in mems]
        masks = {k: shard_cfg_batch(v, u, u + 1, B) for k, v in masks.items()}
        run, row = SamplingRun(m, _sched(), mems, masks, 1, L, n, guidance_scale=7.5, seed=seed, first_utterance=u), 0
    else:
        run, row = SamplingRun(m, _sched(), mems, masks, B, L, n, guidance_scale=7.5, seed=seed), u
    errs = {}
    for k in sorted(int(f[4:]) for f in g.files if f.startswith("step")):
        run.steps(k - run.position)
        errs[k] = rel_l2(run.read().cpu().numpy()[row], g[f"step{k}"][0])
    run.steps(n - run.position)
    lat = run.read(close=True).cpu().numpy()
    errs["final"] = rel_l2(lat[row], g["latents"][:, 0])
    print("c2 dpmpp20", variant, {k: f"{v:.2e}" for k, v in errs.items()})
    assert np.isfinite(lat).all() and all(v < TRAJ_TOL for v in errs.values()), errs


def test_fused_loop_equals_host_loop_of_the_mirror():
    """The captured loop against a host loop of Denoiser.forward, the guidance combine and the mirror's stand-alone ``step``
    (cfd_dpmsolver_step), on the same initial latents: within 1e-5."""
    import torch
    from convofusion_amd.sampler import sample
    from tests.gpu_helpers import hip_denoiser, to_dev
    B, L, S, pad, n, seed = 2, 16, (6, 20, 6, 8, 1), (2, 0, 1, 0, 0), 12, 5
    mems, masks = _inputs(B, L, S, pad, seed)
    init = to_dev(philox_ref.normal_tensor(seed, 0, range(B), 1, L))
    m = hip_denoiser(1234, 1.0)
    fused = sample(m, _sched(), mems, masks, B=B, L=L, num_inference_steps=n, init_latents=init)
    s = _sched()
    s.set_timesteps(n)
    x = init.clone()
    with torch.no_grad():
        for t in s.timesteps:
            out, _ = m(torch.cat([x] * 7), int(t), mems, mem_mask_dict=masks)
            u, *c = out.chunk(7)
            eps = u + sum(7.5 * (ck - u) for ck in c[:5])     # (the full-conditioning chunk has weight 7.5 * 0)
            x = s.step(eps, t, x).prev_sample
    e = rel_l2(fused.cpu().numpy(), x.cpu().numpy())
    print(f"fused vs host loop: {e:.2e}")
    assert s.lower_order_nums == 2 and e < 1e-5


def test_runs_are_deterministic_and_resumable():
    """steps(7) + steps(13) is steps(20) bit for bit, and two runs are bit-identical."""
    import torch
    from convofusion_amd.sampler import SamplingRun
    from tests.gpu_helpers import hip_denoiser
    B, L, S, pad, seed = 3, 16, (24, 161, 24, 8, 1), (2, 3, 0, 0, 0), 9
    mems, masks = _inputs(B, L, S, pad, seed)
    m = hip_denoiser(1234, 1.0)
    outs = []
    for split in ((20,), (7, 13), (20,)):
        with SamplingRun(m, _sched(), mems, masks, B, L, 20, guidance_scale=7.5, seed=seed) as run:
            for k in split:
                run.steps(k)
            outs.append(run.read(close=True))
    assert torch.isfinite(outs[0]).all()
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2])


def test_model_level_drop_in():
    """A reference-shaped model whose yaml names convofusion_amd.scheduler.DPMSolverMultistepScheduler with 20 inference steps: ``install``,
    then the rebound ``_diffusion_reverse`` gives sample()'s latents; the rollout entry point runs the same scheduler."""
    import importlib
    from types import SimpleNamespace
    import torch
    import convofusion_amd
    from convofusion_amd.sampler import diffusion_reverse_forecast, sample
    from tests.gpu_helpers import hip_denoiser, to_dev
    mod, cls = "convofusion_amd.scheduler.DPMSolverMultistepScheduler".rsplit(".", 1)     # configs/modules/scheduler.yaml target
    sched = getattr(importlib.import_module(mod), cls)(**SCHED_KW)
    B, L, S, pad = 2, 16, (6, 20, 6, 8, 1), (2, 0, 1, 0, 0)
    mems, masks = _inputs(B, L, S, pad, 3)
    model = SimpleNamespace(
        denoiser=hip_denoiser(1234, 1.0), scheduler=sched, guidance_scale=7.5, clf_guidance_drops=6, latent_dim=[1, 128],
        do_classifier_free_guidance=True, cfg=SimpleNamespace(model=SimpleNamespace(scheduler=SimpleNamespace(num_inference_timesteps=20, eta=0.0))))
    convofusion_amd.install(model)
    init = to_dev(philox_ref.normal_tensor(21, 0, range(B), 1, L))
    lat, atts = model._diffusion_reverse(mems, None, masks)
    assert tuple(lat.shape) == (L, B, 128) and torch.isfinite(lat).all() and len(atts) >= 1
    lat, _ = convofusion_amd.sampler.diffusion_reverse(model, mems, None, masks, init_latents=init, seed=21)
    want = sample(model.denoiser, _sched(), mems, masks, B=B, L=L, num_inference_steps=20, init_latents=init, seed=21)
    assert torch.equal(lat.permute(1, 0, 2), want)
    pre = 0.3 * torch.randn((B, 8, 128), device="cuda")
    f, att = diffusion_reverse_forecast(model, mems, None, pre, masks, init_latents=init, seed=21)
    assert tuple(f.shape) == (L, B, 128) and torch.isfinite(f).all() and len(att) == 5
    # the word-excitation-guidance branch (focus_indices) refuses the solver
    model.weg_parameters = dict(scale_factor=1000, scale_range=[1.0, 0.5], max_iter_to_alter=2, thresholds={0: 0.05}, max_refinement_steps=1)
    with pytest.raises(NotImplementedError, match="DPMSolverMultistepScheduler"):
        convofusion_amd.sampler.diffusion_reverse(model, mems, None, masks, focus_indices=[[2]], init_latents=init, seed=21)


def test_abi_refuses_bad_kind2_arguments():
    """Through the C ABI: kind 2 without a table, with a table that does not decrease strictly, with clip_sample; and
    cfd_scheduler_step with kind 2."""
    import torch
    from convofusion_amd import _lib
    from convofusion_amd.sampler import SamplingRun
    from tests.gpu_helpers import hip_denoiser
    B, L, S, pad = 1, 16, (6, 20, 6, 8, 1), (2, 0, 1, 0, 0)
    mems, masks = _inputs(B, L, S, pad, 4)
    run = SamplingRun(hip_denoiser(1234, 1.0), _sched(), mems, masks, B, L, 10, guidance_scale=7.5, seed=1)
    run.close()
    lib = _lib.load()
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    bad_ts = (C.c_int32 * 10)(*[900, 800, 800, 600, 500, 400, 300, 200, 100, 1])
    for what, edit in (("no table", lambda a: setattr(a, "timesteps", None)),
                       ("not strictly decreasing", lambda a: setattr(a, "timesteps", C.cast(bad_ts, C.c_void_p))),
                       ("clip_sample", lambda a: setattr(a, "clip_sample", 1))):
        a = _lib.SampleArgs.from_buffer_copy(run._args)
        edit(a)
        rc = lib.cfd_sample_begin(run.handle, C.byref(a), stream)
        assert rc == -1, (what, rc, lib.cfd_last_error())
        print(what, "->", lib.cfd_last_error().decode())
    x = torch.zeros(128, device="cuda")
    acp = _sched().alphas_cumprod.contiguous()
    rc = lib.cfd_scheduler_step(run.handle, 2, C.c_void_p(acp.data_ptr()), 1000, 10, 900, 0, 0.0, 1, C.c_void_p(x.data_ptr()), None,
                                C.c_void_p(x.data_ptr()), x.numel(), None, stream)
    assert rc == -1 and b"cfd_dpmsolver_step" in lib.cfd_last_error()
