"""-m gpu: ``prediction_type="sample"`` (an x0-predicting denoiser, the reference's TRAIN.ABLATION.PREDICT_EPSILON: False) on the device --
the stand-alone steps against the restatement (tests/prediction_ref.py), the captured loop (cfd_sample_args.prediction_type = 1) against
trajectories made with the REFERENCE denoiser read as x0 (tests/golden/traj_pred_*.npz, make_golden_prediction.py) and against a host
loop of the mirror's own ``step``, what composes with it bit for bit, the epsilon run's unchanged arguments, and the ABI's refusals.

Tolerance on trajectories: 1e-3 relative L2 (BASELINE.json north_star), as for the epsilon loops; the errors are printed.  Every weight
is seeded: the trajectories show that the loop computes the restated arithmetic, not how an x0-predicting checkpoint samples."""
import ctypes as C

import numpy as np
import pytest

from oracle import inputs, philox_ref
from tests.helpers import load_golden, rel_l2

pytestmark = pytest.mark.gpu
TRAJ_TOL = 1e-3
YAML = dict(num_train_timesteps=1000, beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear")
SMALL = dict(B=2, L=16, S=(6, 20, 6, 8, 1), pad=(2, 0, 1, 0, 0))


def _sched(kind, prediction_type="sample", **kw):
    from convofusion_amd import scheduler
    if kind == "ddpm":
        return scheduler.DDPMScheduler(**YAML, variance_type="fixed_small", clip_sample=True, prediction_type=prediction_type, **kw)
    if kind == "ddim":
        return scheduler.DDIMScheduler(**YAML, **dict(dict(clip_sample=True), **kw), prediction_type=prediction_type)
    return scheduler.DPMSolverMultistepScheduler(**YAML, prediction_type=prediction_type, **kw)


def _inputs(B, L, S, pad, seed):
    from tests.gpu_helpers import to_dev
    cb = inputs.make_cfg_batch(seed=seed, B=B, L=L, S=S, pad_tail=pad)
    return [to_dev(x) for x in cb["memories"]], {k: to_dev(v) for k, v in cb["masks"].items()}


# ---- the stand-alone steps ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["ddpm", "ddim_eta0", "ddim_eta05", "dpmpp"])
def test_standalone_steps_match_the_restatement(kind):
    """[2, 16, 128], out in [-2, 2] (the clip acts), at the first, a middle and the last table entry of N = 1000 and N = 50: prev_sample
    and pred_original_sample at rtol = atol = 2e-5, the tolerance of test_scheduler_step_and_add_noise for the epsilon steps.  DPM++: the
    first call after set_timesteps is order 1, the next one order 2 (its history: the first call's x0)."""
    import torch
    from tests.prediction_ref import DDIMSampleRef, DDPMSampleRef, DPMSolverSampleRef
    rng = np.random.default_rng(11)
    x = rng.standard_normal((2, 16, 128)).astype(np.float32)
    out = rng.uniform(-2.0, 2.0, x.shape).astype(np.float32)
    out2 = rng.uniform(-2.0, 2.0, x.shape).astype(np.float32)
    z = rng.standard_normal(x.shape).astype(np.float32)
    dev = lambda a: torch.from_numpy(a).cuda()   # noqa: E731
    close = lambda a, b: np.testing.assert_allclose(a.cpu().numpy(), b, rtol=2e-5, atol=2e-5)   # noqa: E731
    assert (np.abs(out) > 1).any()
    for n in (1000, 50):
        if kind == "dpmpp":
            if n == 1000:
                n = 999     # (the solver's table needs N < num_train_timesteps)
            s, r = _sched("dpmpp"), DPMSolverSampleRef(**YAML)
            for i in (0, n // 2, n - 1):       # order 1 at entry i - 1 (i = 0: none), then at entry i: order 2 (i = 0: order 1)
                s.set_timesteps(n)
                r.set_timesteps(n)
                np.testing.assert_array_equal(s.timesteps.numpy(), r.timesteps)
                xs, xr = dev(x), x
                if i > 0:
                    t0 = int(r.timesteps[i - 1])
                    got, xr = s.step(dev(out2), t0, xs), r.step(out2, t0, xr)
                    xs = got.prev_sample
                    close(xs, xr)
                t = int(r.timesteps[i])
                got, want = s.step(dev(out), t, xs), r.step(out, t, xr)
                assert s.lower_order_nums == r.lower_order_nums == (2 if i > 0 else 1)
                close(got.prev_sample, want)
                assert np.array_equal(s.model_outputs[-1].cpu().numpy(), out)     # x0, the next step's history, is the output itself
            continue
        eta = 0.5 if kind == "ddim_eta05" else 0.0
        s, r = (_sched("ddpm"), DDPMSampleRef()) if kind == "ddpm" else (_sched("ddim"), DDIMSampleRef())
        s.set_timesteps(n)
        r.set_timesteps(n)
        np.testing.assert_array_equal(s.timesteps.numpy(), r.timesteps)
        for t in (int(r.timesteps[0]), int(r.timesteps[n // 2]), int(r.timesteps[-1])):
            if kind == "ddpm":
                got, want = s.step(dev(out), t, dev(x), variance_noise=dev(z)), r.step(out, t, x, noise=z)
            else:
                got, want = s.step(dev(out), t, dev(x), eta=eta, variance_noise=dev(z)), r.step(out, t, x, eta=eta, noise=z)
            close(got.prev_sample, want)
            close(got.pred_original_sample, r.pred_original_sample)
            assert np.array_equal(got.pred_original_sample.cpu().numpy(), np.clip(out, -1, 1))     # the clipped model output, exactly


# ---- the fused loop against the goldens -----------------------------------------------------------------------------------------------
GOLDENS = {"pred_ddpm20": "ddpm", "pred_ddim10": "ddim", "pred_dpmpp10": "dpmpp", "pred_inpaint20": "ddpm", "pred_modality_ddpm20": "ddpm"}


@pytest.mark.parametrize("name", sorted(GOLDENS))
def test_fused_loop_matches_reference_trajectory(name):
    """Every stored snapshot and the final latents of every golden, every element (the clip is continuous in the output)."""
    from convofusion_amd.sampler import SamplingRun
    from tests.gpu_helpers import hip_denoiser, to_dev
    g = load_golden("traj_" + name)
    m = [int(x) for x in g["meta"]]
    B, L, S, pad, n, seed = m[0], m[1], tuple(m[2:7]), tuple(m[7:12]), m[12], m[13]
    mems, masks = _inputs(B, L, S, pad, seed)
    kw = {}
    if "inpaint" in name:
        kw["preseq"] = to_dev(g["preseq"])
    if "modality" in name:
        kw["modality_weights"] = g["weights"]
    run = SamplingRun(hip_denoiser(1234, 1.0), _sched(GOLDENS[name]), mems, masks, B, L, n, guidance_scale=7.5, seed=seed,
                      init_latents=to_dev(philox_ref.normal_tensor(seed, 0, range(B), 1, L)), **kw)
    assert run.N == n and run._args.prediction_type == 1 and run._args.operand_policy == 0
    if "modality" in name:
        assert run.chunks_evaluated == 6       # apb is 0 throughout: pruned
    errs = {}
    for k in sorted(int(f[4:]) for f in g.files if f.startswith("step")):
        run.steps(k - run.position)
        errs[k] = rel_l2(run.read().cpu().numpy(), g[f"step{k}"])
    run.steps(n - run.position)
    lat = run.read(close=True).permute(1, 0, 2).cpu().numpy()
    errs["final"] = rel_l2(lat, g["latents"])
    print(name, {k: f"{v:.2e}" for k, v in errs.items()})
    assert np.isfinite(lat).all() and all(v < TRAJ_TOL for v in errs.values()), errs


# ---- the fused loop against a host loop of the mirror -----------------------------------------------------------------------------------
def _host_loop(m, s, mems, masks, init, n, step_noise, factors):
    """Denoiser.forward, the combine u + sum_k factors[:, k] (c_k - u) in the reference's order, the mirror's own ``step``."""
    import torch
    s.set_timesteps(n)
    x = init.clone()
    f = factors.reshape(factors.shape[0], 6, 1, 1)
    with torch.no_grad():
        for i, t in enumerate(s.timesteps):
            out, _ = m(torch.cat([x] * 7), int(t), mems, mem_mask_dict=masks)
            u, *c = out.chunk(7)
            acc = f[:, 0] * (c[0] - u)
            for k in range(1, 6):
                acc = acc + f[:, k] * (c[k] - u)
            comb = u + acc
            if s.KIND == 0:
                x = s.step(comb, t, x, variance_noise=step_noise[i]).prev_sample
            else:
                x = s.step(comb, t, x).prev_sample
    return x


def _table_len(s, n):
    """Entries of the scheduler's table for num_inference_steps = n: n itself, but n + 1 for the unpinned DDPM table arange(0, T, T // n)
    when n does not divide T (13 for n = 12, 4 for n = 3) -- the step noise has one slice per entry."""
    s.set_timesteps(n)
    return len(s.timesteps)


@pytest.mark.parametrize("kind", ["ddpm", "ddim", "dpmpp"])
def test_fused_loop_equals_host_loop_of_the_mirror(kind):
    """B = 2, N = 12, the same initial latents and step noise: within 1e-5 (test_fused_loop_equals_host_loop_of_the_mirror's bound).
    12 does not divide 1000, so the DDPM mirror is built with allow_unpinned_timesteps=True (the table arange(0, T, T // N)[::-1]); both
    sides of the comparison read that same table, which has 13 entries."""
    import torch
    from convofusion_amd.sampler import sample
    from tests.gpu_helpers import hip_denoiser, to_dev
    B, L, S, pad, n, seed = SMALL["B"], SMALL["L"], SMALL["S"], SMALL["pad"], 12, 5
    mems, masks = _inputs(B, L, S, pad, seed)
    init = to_dev(philox_ref.normal_tensor(seed, 0, range(B), 1, L))
    kw = dict(allow_unpinned_timesteps=True) if kind == "ddpm" else {}
    noise = torch.randn((_table_len(_sched(kind, **kw), n), B, L, 128), device="cuda", generator=torch.Generator("cuda").manual_seed(3))
    m = hip_denoiser(1234, 1.0)
    fused = sample(m, _sched(kind, **kw), mems, masks, B=B, L=L, num_inference_steps=n, init_latents=init, step_noise=noise)
    factors = torch.tensor([[7.5] * 5 + [0.0]] * B, device="cuda")
    host = _host_loop(m, _sched(kind, **kw), mems, masks, init, n, noise, factors)
    e = rel_l2(fused.cpu().numpy(), host.cpu().numpy())
    print(f"{kind}: fused vs host loop {e:.2e}")
    assert torch.isfinite(fused).all() and e < 1e-5


@pytest.mark.parametrize("combine", ["default", "weighted"])
def test_second_grid_stride_pass_equals_host_loop(combine):
    """DDPM, B = 13, L = 160, 3 steps: B x L = 2080 tokens are 66 560 groups of four elements, more than the 65 536 threads of
    cfg_step_kernel's 256 x 256 grid, so its grid-stride loop takes a second pass -- which the small goldens never reach.  3 does not
    divide 1000: allow_unpinned_timesteps=True on both sides, as above (num_inference_steps = 3 gives the four entries 999, 666, 333, 0)."""
    import torch
    from convofusion_amd.sampler import sample
    from tests.gpu_helpers import hip_denoiser, to_dev
    B, L, S, pad, n, seed = 13, 160, SMALL["S"], SMALL["pad"], 3, 8
    assert B * L * 32 > 256 * 256
    mems, masks = _inputs(B, L, S, pad, seed)
    init = to_dev(philox_ref.normal_tensor(seed, 0, range(B), 1, L))
    noise = torch.randn((_table_len(_sched("ddpm", allow_unpinned_timesteps=True), n), B, L, 128), device="cuda",
                        generator=torch.Generator("cuda").manual_seed(4))
    m = hip_denoiser(1234, 1.0)
    kw, w = {}, np.array([[1.0] * 5 + [0.0]] * B)
    if combine == "weighted":
        w = np.random.default_rng(6).uniform(0.0, 2.0, (B, 6))
        kw["modality_weights"] = w
    fused = sample(m, _sched("ddpm", allow_unpinned_timesteps=True), mems, masks, B=B, L=L, num_inference_steps=n, init_latents=init,
                   step_noise=noise, **kw)
    factors = torch.from_numpy((7.5 * w).astype(np.float32)).cuda()
    host = _host_loop(m, _sched("ddpm", allow_unpinned_timesteps=True), mems, masks, init, n, noise, factors)
    e = rel_l2(fused.cpu().numpy(), host.cpu().numpy())
    print(f"{combine}: fused vs host loop at B x L = {B * L}: {e:.2e}")
    assert torch.isfinite(fused).all() and e < 1e-5


# ---- composition ------------------------------------------------------------------------------------------------------------------------
def test_composition_is_bit_for_bit():
    """A no-op edit (strength 1, nothing kept) and a tie table of -1 equal the plain run; the reference's weights given explicitly equal
    the default path; steps(7) + steps(13) is steps(20); two runs are identical."""
    import torch
    from convofusion_amd.sampler import REFERENCE_MODALITY_WEIGHTS, SamplingRun, sample
    from tests.gpu_helpers import hip_denoiser
    B, L, S, pad, n, seed = 3, 16, (24, 161, 24, 8, 1), (2, 3, 0, 0, 0), 20, 9
    mems, masks = _inputs(B, L, S, pad, seed)
    m = hip_denoiser(1234, 1.0)
    for kind in ("ddpm", "dpmpp"):
        kw = dict(B=B, L=L, num_inference_steps=n, seed=seed)
        plain = sample(m, _sched(kind), mems, masks, **kw)
        assert torch.isfinite(plain).all()
        assert torch.equal(plain, sample(m, _sched(kind), mems, masks, **kw))
        assert torch.equal(plain, sample(m, _sched(kind), mems, masks, source_latents=torch.zeros((B, L, 128), device="cuda"), **kw))
        assert torch.equal(plain, sample(m, _sched(kind), mems, masks, tie=torch.full((B, L), -1, dtype=torch.int64), **kw))
        skipped = sample(m, _sched(kind), mems, masks, skip_zero_weight_chunks=True, **kw)
        assert torch.equal(skipped, sample(m, _sched(kind), mems, masks, modality_weights=dict(REFERENCE_MODALITY_WEIGHTS), **kw))
        assert torch.equal(plain, skipped)
        with SamplingRun(m, _sched(kind), mems, masks, B, L, n, seed=seed) as run:
            run.steps(7)
            run.steps(13)
            assert torch.equal(plain, run.read(close=True))


# ---- epsilon unchanged, and the ABI's refusals ---------------------------------------------------------------------------------------------
def _raw_run(lib, run, a, stream):
    import torch
    out = torch.empty((run.B, run.L, 128), dtype=torch.float32, device="cuda")
    assert lib.cfd_sample_begin(run.handle, C.byref(a), stream) == 0, lib.cfd_last_error()
    assert lib.cfd_sample_steps(run.handle, run.N) == 0 and lib.cfd_sample_read(run.handle, C.c_void_p(out.data_ptr()), 1) == 0
    return out


def test_epsilon_run_is_unchanged():
    """An epsilon run's args carry prediction_type 0, and a run opened through the raw ABI with the field zeroed gives its latents; the same
    arguments with the field set to 1 give the "sample" run's."""
    import torch
    from convofusion_amd import _lib
    from convofusion_amd.sampler import SamplingRun
    from tests.gpu_helpers import hip_denoiser
    B, L, S, pad, n, seed = SMALL["B"], SMALL["L"], SMALL["S"], SMALL["pad"], 10, 2
    mems, masks = _inputs(B, L, S, pad, seed)
    m = hip_denoiser(1234, 1.0)
    lib, stream = _lib.load(), C.c_void_p(torch.cuda.current_stream().cuda_stream)
    outs = {}
    for ptype in ("epsilon", "sample"):
        run = SamplingRun(m, _sched("ddpm", ptype), mems, masks, B, L, n, seed=seed, operands=0)
        assert run._args.prediction_type == (0 if ptype == "epsilon" else 1)
        run.steps(n)
        outs[ptype] = run.read(close=True)
    assert not torch.equal(outs["epsilon"], outs["sample"])
    for ptype, field in (("epsilon", 0), ("sample", 1)):
        a = _lib.SampleArgs.from_buffer_copy(run._args)
        a.prediction_type = field
        assert torch.equal(_raw_run(lib, run, a, stream), outs[ptype])
    default = SamplingRun(m, _sched("ddpm", "epsilon"), mems, masks, B, L, n, seed=seed)
    assert default._args.prediction_type == 0 and default._args.operand_policy == 15      # (the kind's default policy stays)
    default.close()


def test_abi_refusals():
    """prediction_type = 2 or -1 is CFD_E_ARG naming the field; kind 3, the anchored opener, cfd_ddpm_invert, cfd_sample_parallel and the
    replay opener refuse 1; so do the two _pred entry points for a value other than 0 / 1."""
    import torch
    from convofusion_amd import _lib, scheduler
    from convofusion_amd.sampler import SamplingRun
    from tests.gpu_helpers import hip_denoiser
    B, L, S, pad, n = 1, 16, SMALL["S"], SMALL["pad"], 10
    mems, masks = _inputs(B, L, S, pad, 4)
    m = hip_denoiser(1234, 1.0)
    lib, stream = _lib.load(), C.c_void_p(torch.cuda.current_stream().cuda_stream)
    ring = torch.zeros((n + 1, B, L, 128), device="cuda")
    noise = torch.zeros((n, B, L, 128), device="cuda")
    lat = torch.zeros((B, L, 128), device="cuda")

    def args_of(sch, value, **kw):
        run = SamplingRun(m, sch, mems, masks, B, L, n, seed=1, **kw)
        run.close()
        a = _lib.SampleArgs.from_buffer_copy(run._args)
        a.prediction_type = value
        return run, a

    def refused(rc, what):
        msg = lib.cfd_last_error().decode()
        print(what, "->", msg)
        assert rc == -1 and "prediction_type" in msg, (what, rc, msg)

    for bad in (2, -1):
        run, a = args_of(_sched("ddpm", "epsilon"), bad)
        refused(lib.cfd_sample_begin(run.handle, C.byref(a), stream), f"prediction_type = {bad}")
    run, a = args_of(scheduler.DDIMInverseScheduler(**YAML), 1, init_latents=lat)
    refused(lib.cfd_sample_begin(run.handle, C.byref(a), stream), "kind 3")
    run, a = args_of(_sched("ddim", "epsilon", clip_sample=False), 1)
    an = _lib.AnchorArgs()
    an.trajectory, an.steps, an.B, an.L = ring.data_ptr(), n, B, L
    refused(lib.cfd_sample_begin_anchored(run.handle, C.byref(a), C.byref(an), None, 0, None, stream), "anchored")
    run, a = args_of(_sched("ddpm", "epsilon"), 1)
    rp = _lib.ReplayArgs()
    rp.trajectory, rp.noise, rp.steps, rp.B, rp.L = ring.data_ptr(), noise.data_ptr(), n, B, L
    refused(lib.cfd_sample_begin_replay(run.handle, C.byref(a), C.byref(rp), None, 0, None, stream), "replay")
    iv = _lib.DdpmInvertArgs()
    iv.source, iv.trajectory, iv.noise = lat.data_ptr(), ring.data_ptr(), noise.data_ptr()
    refused(lib.cfd_ddpm_invert(run.handle, C.byref(a), C.byref(iv), None, None, stream), "cfd_ddpm_invert")
    pa = _lib.ParallelArgs()
    pa.latents, pa.tolerance = lat.data_ptr(), 0.0
    refused(lib.cfd_sample_parallel(run.handle, C.byref(a), C.byref(pa), None, stream), "cfd_sample_parallel")
    # the openers still open the run with the field at 0 (the refusals above are the field's)
    a.prediction_type = 0
    assert lib.cfd_sample_begin(run.handle, C.byref(a), stream) == 0 and lib.cfd_sample_read(run.handle, C.c_void_p(lat.data_ptr()), 1) == 0
    acp = _sched("ddpm").alphas_cumprod.contiguous()
    x = torch.zeros(128, device="cuda")
    p = C.c_void_p(x.data_ptr())
    for bad in (2, -1):
        refused(lib.cfd_scheduler_step_pred(run.handle, 0, C.c_void_p(acp.data_ptr()), 1000, 10, 900, 0, 0.0, 1, bad, p, p, p, x.numel(), None,
                                            stream), f"cfd_scheduler_step_pred {bad}")
        refused(lib.cfd_dpmsolver_step_pred(run.handle, C.c_void_p(acp.data_ptr()), 1000, 900, 800, -1, bad, p, None, p, p, x.numel(), stream),
                f"cfd_dpmsolver_step_pred {bad}")
    refused(lib.cfd_scheduler_step_pred(run.handle, 3, C.c_void_p(acp.data_ptr()), 1000, 10, 900, 0, 0.0, 1, 1, p, None, p, x.numel(), None, stream),
            "cfd_scheduler_step_pred kind 3")


# ---- the model-level drop-in --------------------------------------------------------------------------------------------------------------
def test_model_level_drop_in():
    """A reference-shaped model whose scheduler is built by dotted path with prediction_type="sample" in its params -- what
    convofusion.py:102 produces for PREDICT_EPSILON: False: ``install``, then the rebound ``_diffusion_reverse`` gives sample()'s latents bit
    for bit; the rollout entry point runs; focus_indices is refused."""
    import importlib
    from types import SimpleNamespace
    import torch
    import convofusion_amd
    from convofusion_amd.sampler import diffusion_reverse_forecast, sample
    from tests.gpu_helpers import hip_denoiser, to_dev
    params = dict(YAML, variance_type="fixed_small", clip_sample=True)
    params["prediction_type"] = "sample"                                                    # convofusion.py:101-103
    mod, cls = "convofusion_amd.scheduler.DDPMScheduler".rsplit(".", 1)                     # configs/modules/scheduler.yaml target
    sched = getattr(importlib.import_module(mod), cls)(**params)
    B, L, S, pad = SMALL["B"], SMALL["L"], SMALL["S"], SMALL["pad"]
    mems, masks = _inputs(B, L, S, pad, 3)
    model = SimpleNamespace(
        denoiser=hip_denoiser(1234, 1.0), scheduler=sched, guidance_scale=7.5, clf_guidance_drops=6, latent_dim=[1, 128],
        do_classifier_free_guidance=True, cfg=SimpleNamespace(model=SimpleNamespace(scheduler=SimpleNamespace(num_inference_timesteps=20, eta=0.0))))
    convofusion_amd.install(model)
    init = to_dev(philox_ref.normal_tensor(21, 0, range(B), 1, L))
    lat, atts = model._diffusion_reverse(mems, None, masks)
    assert tuple(lat.shape) == (L, B, 128) and torch.isfinite(lat).all() and len(atts) >= 1
    lat, _ = convofusion_amd.sampler.diffusion_reverse(model, mems, None, masks, init_latents=init, seed=21)
    want = sample(model.denoiser, _sched("ddpm"), mems, masks, B=B, L=L, num_inference_steps=20, init_latents=init, seed=21)
    assert torch.equal(lat.permute(1, 0, 2), want)
    eps = sample(model.denoiser, _sched("ddpm", "epsilon"), mems, masks, B=B, L=L, num_inference_steps=20, init_latents=init, seed=21, operands=0)
    assert not torch.equal(want, eps)
    pre = 0.3 * torch.randn((B, 8, 128), device="cuda")
    f, att = diffusion_reverse_forecast(model, mems, None, pre, masks, init_latents=init, seed=21)
    assert tuple(f.shape) == (L, B, 128) and torch.isfinite(f).all() and len(att) == 5
    model.weg_parameters = dict(scale_factor=1000, scale_range=[1.0, 0.5], max_iter_to_alter=2, thresholds={0: 0.05}, max_refinement_steps=1)
    with pytest.raises(NotImplementedError, match="prediction_type='sample'"):
        convofusion_amd.sampler.diffusion_reverse(model, mems, None, masks, focus_indices=[[2]], init_latents=init, seed=21)
