"""-m gpu: per-modality guidance weights in the captured loop (cfd_sample_begin_weighted, ``SamplingRun(modality_weights=...)``).

The weighted path with the reference's weights against the default path (bit for bit), against trajectories made with the REFERENCE
denoiser and the restated weighted combine (tests/golden/traj_modality_*.npz, make_golden_modality.py), pruning of zero-weight chunks,
per-utterance rows against one-utterance shards, the model-level drop-in and the ABI's refusals.  Errors are printed."""
import ctypes as C

import numpy as np
import pytest

from oracle import inputs, philox_ref
from tests.helpers import load_golden, rel_l2

pytestmark = pytest.mark.gpu
TRAJ_TOL = 1e-3
DPM_KW = dict(num_train_timesteps=1000, beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear")
REF = dict(text=1, audio=1, spk=1, apb=1, lsnid=1, all=0)


def _sched(kind):
    from convofusion_amd import scheduler
    from tests.gpu_helpers import SCHED_KW
    if kind == "dpmpp":
        return scheduler.DPMSolverMultistepScheduler(**DPM_KW)
    return scheduler.DDIMScheduler(**SCHED_KW) if kind == "ddim" else scheduler.DDPMScheduler(variance_type="fixed_small", **SCHED_KW)


def _inputs(B, L, S, pad, seed, uncond_pad=None):
    from tests.gpu_helpers import to_dev
    kw = dict(uncond_pad_tail=uncond_pad) if uncond_pad is not None else {}
    cb = inputs.make_cfg_batch(seed=seed, B=B, L=L, S=S, pad_tail=pad, **kw)
    return [to_dev(x) for x in cb["memories"]], {k: to_dev(v) for k, v in cb["masks"].items()}


def _small(B=2, seed=2025):
    return _inputs(B, 16, (6, 20, 6, 8, 1), (2, 0, 1, 0, 0), seed)


@pytest.mark.parametrize("shape", ["golden_ddpm20", "golden_dpmpp10", "headline_b32"])
def test_reference_weights_are_bit_identical_to_the_default_path(shape):
    """modality_weights = the reference's 1, 1, 1, 1, 1, 0 given explicitly: pruning drops the full-conditioning chunk, as the default path
    with skip_zero_weight_chunks=True does -- 6 chunks each, the same denoiser rows, the same combine: the latents are bit-identical."""
    import torch
    from convofusion_amd.sampler import SamplingRun
    from tests.gpu_helpers import hip_denoiser
    m = hip_denoiser(1234, 1.0)
    if shape == "headline_b32":          # B = 32, L = 196, 1500 audio keys (the fused cross-attention path, the default operand policy)
        g = load_golden("traj_c2_ddpm5")
        meta = [int(v) for v in g["meta"]]
        B, L, S, pad, seed = meta[0], meta[1], tuple(meta[2:7]), tuple(meta[7:12]), meta[13]
        mems, masks = _inputs(B, L, S, pad, seed, uncond_pad=pad)
        kind, n, steps = "ddpm", 1000, 3
    else:
        kind, n = ("dpmpp", 10) if "dpmpp" in shape else ("ddpm", 20)
        B, L, seed, steps = 2, 16, 2025, n
        mems, masks = _small(B, seed)
    outs = []
    for mw in (None, REF):
        with SamplingRun(m, _sched(kind), mems, masks, B, L, n, guidance_scale=7.5, seed=seed, skip_zero_weight_chunks=True,
                         modality_weights=mw) as run:
            assert run.chunks_evaluated == 6
            run.steps(steps)
            outs.append(run.read(close=True))
    assert torch.isfinite(outs[0]).all()
    assert torch.equal(outs[0], outs[1]), float((outs[0] - outs[1]).abs().max())


def _golden_case(name):
    g = load_golden("traj_modality_" + name)
    meta = [int(x) for x in g["meta"]]
    B, L, S, pad, n, seed = meta[0], meta[1], tuple(meta[2:7]), tuple(meta[7:12]), meta[12], meta[13]
    return g, B, L, S, pad, n, seed


@pytest.mark.parametrize("operands", [None, 0])
@pytest.mark.parametrize("name", ["ddpm20", "dpmpp10", "inpaint20"])
def test_weighted_loop_matches_reference_trajectory(name, operands):
    """Per-utterance weights -- an interval schedule and a ramp, apb 0 throughout (pruned), the full-conditioning chunk guided -- against
    the restated loop on the reference denoiser: every snapshot and the final latents within 1e-3 relative L2."""
    from convofusion_amd.sampler import SamplingRun
    from tests.gpu_helpers import hip_denoiser, to_dev
    g, B, L, S, pad, n, seed = _golden_case(name)
    mems, masks = _inputs(B, L, S, pad, seed)
    init = philox_ref.normal_tensor(seed, 0, range(B), 1, L)
    kind = "dpmpp" if "dpmpp" in name else "ddpm"
    noise = None if kind == "dpmpp" else to_dev(np.stack([philox_ref.normal_tensor(seed, i, range(B), 0, L) for i in range(n)]))
    run = SamplingRun(hip_denoiser(1234, 1.0), _sched(kind), mems, masks, B, L, n, guidance_scale=7.5, init_latents=to_dev(init),
                      step_noise=noise, preseq=to_dev(g["preseq"]) if "inpaint" in name else None, operands=operands,
                      modality_weights=g["weights"])
    assert run.N == n and run.chunks_evaluated == 6
    errs = {}
    for k in sorted(int(f[4:]) for f in g.files if f.startswith("step")):
        run.steps(k - run.position)
        errs[k] = rel_l2(run.read().cpu().numpy(), g[f"step{k}"])
    run.steps(n - run.position)
    lat = run.read(close=True).permute(1, 0, 2).cpu().numpy()
    errs["final"] = rel_l2(lat, g["latents"])
    print("modality", name, "operands", operands, {k: f"{v:.2e}" for k, v in errs.items()})
    assert np.isfinite(lat).all() and all(v < TRAJ_TOL for v in errs.values()), errs


def test_pruning_drops_zero_weight_chunks_and_keeps_the_result():
    """apb = lsnid = all = 0: 4 chunks evaluated (uncond, text, audio, spk), the latents of the unpruned run (7 chunks) within 1e-6.  With
    every iteration's attention maps (the ring keeps the full-conditioning chunk's), 5 chunks and a complete dict."""
    import torch
    from convofusion_amd.sampler import SamplingRun, sample
    from tests.gpu_helpers import hip_denoiser
    m = hip_denoiser(1234, 1.0)
    B, L, n, seed = 3, 16, 20, 31
    mems, masks = _small(B, seed)
    mw = dict(text=2.0, audio=0.5, spk=1.5, apb=0, lsnid=0, all=0)
    outs = {}
    for prune in (True, False):
        with SamplingRun(m, _sched("ddpm"), mems, masks, B, L, n, guidance_scale=7.5, seed=seed, modality_weights=mw,
                         prune_zero_weight_chunks=prune) as run:
            assert run.chunks_evaluated == (4 if prune else 7)
            run.steps(n)
            outs[prune] = run.read(close=True)
    e = float((outs[True] - outs[False]).norm() / outs[False].norm())
    print(f"pruned (4 chunks) vs unpruned (7): {e:.2e}")
    assert torch.isfinite(outs[True]).all() and e < 1e-6
    with SamplingRun(m, _sched("ddpm"), mems, masks, B, L, n, guidance_scale=7.5, seed=seed, modality_weights=mw, attention_ring=True) as run:
        assert run.chunks_evaluated == 5
    lat, atts = sample(m, _sched("ddpm"), mems, masks, B=B, L=L, num_inference_steps=n, seed=seed, modality_weights=mw, return_attention="all")
    e = float((lat - outs[False]).norm() / outs[False].norm())
    print(f"with the attention ring (5 chunks) vs unpruned: {e:.2e}")
    assert e < 1e-6
    assert sorted(atts) == sorted(range(0, 1000, 1000 // n)) and all(len(v) == 5 for v in atts.values())
    assert all(torch.isfinite(a).all() and tuple(a.shape[:2]) == (B, 9) for v in atts.values() for a in v)


def test_per_utterance_rows_match_one_utterance_runs():
    """Row b of a batch with per-utterance scheduled weights equals a B = 1 run of utterance b's inputs and weights with first_utterance = b
    (Philox streams are keyed by global utterance id) within 1e-5."""
    import torch
    from convofusion_amd.distributed import shard_cfg_batch, shard_modality_weights
    from convofusion_amd.sampler import sample
    from tests.gpu_helpers import hip_denoiser
    m = hip_denoiser(1234, 1.0)
    B, L, n, seed = 3, 16, 20, 12
    mems, masks = _small(B, seed)
    rng = np.random.default_rng(5)
    w = rng.uniform(0.0, 2.0, size=(n, B, 6))
    w[:, 1, :] *= (np.arange(n) >= n // 2)[:, None]      # utterance 1: guided in the second half only
    w[:, :, 4] = 0.0                                     # lsnid: pruned
    full = sample(m, _sched("ddpm"), mems, masks, B=B, L=L, num_inference_steps=n, seed=seed, modality_weights=torch.from_numpy(w))
    for b in range(B):
        enc = [shard_cfg_batch(x, b, b + 1, B) for x in mems]
        mk = {k: shard_cfg_batch(v, b, b + 1, B) for k, v in masks.items()}
        one = sample(m, _sched("ddpm"), enc, mk, B=1, L=L, num_inference_steps=n, seed=seed, first_utterance=b,
                     modality_weights=shard_modality_weights(w, b, b + 1, B))
        e = float((one[0] - full[b]).norm() / full[b].norm())
        print(f"utterance {b}: {e:.2e}")
        assert e < 1e-5


@pytest.mark.parametrize("kind", ["ddim", "dpmpp"])
def test_install_binds_the_weights(kind):
    """install(model, modality_weights=...): the rebound _diffusion_reverse gives sample(modality_weights=...)'s latents, without and (DDIM)
    with focus_indices, where the weights change the result."""
    import torch
    from types import SimpleNamespace
    import convofusion_amd
    from convofusion_amd.sampler import diffusion_reverse, sample
    from tests.gpu_helpers import hip_denoiser, to_dev
    B, L, n = 1, 16, 10
    mems, masks = _inputs(B, L, (6, 20, 12, 8, 1), (2, 0, 3, 0, 0), 4)
    mw = dict(text=2.0, audio=0.25, apb=0)
    model = SimpleNamespace(
        denoiser=hip_denoiser(1234, 1.0), scheduler=_sched(kind), guidance_scale=7.5, clf_guidance_drops=6, latent_dim=[1, 128],
        do_classifier_free_guidance=True, cfg=SimpleNamespace(model=SimpleNamespace(scheduler=SimpleNamespace(num_inference_timesteps=n, eta=0.0))))
    init = to_dev(philox_ref.normal_tensor(21, 0, range(B), 1, L))
    convofusion_amd.install(model, modality_weights=mw)
    lat, atts = model._diffusion_reverse(mems, None, masks)
    assert tuple(lat.shape) == (L, B, 128) and torch.isfinite(lat).all() and len(atts) >= 1
    lat, _ = diffusion_reverse(model, mems, None, masks, init_latents=init, seed=21)
    want = sample(model.denoiser, _sched(kind), mems, masks, B=B, L=L, num_inference_steps=n, init_latents=init, seed=21, modality_weights=mw)
    assert torch.equal(lat.permute(1, 0, 2), want)
    plain = sample(model.denoiser, _sched(kind), mems, masks, B=B, L=L, num_inference_steps=n, init_latents=init, seed=21)
    assert (want - plain).norm() / plain.norm() > 1e-3
    if kind == "ddim":
        model.weg_parameters = dict(scale_factor=1000, scale_range=[1.0, 0.5], max_iter_to_alter=2, thresholds={0: 0.05}, max_refinement_steps=1)
        steered, _ = diffusion_reverse(model, mems, None, masks, focus_indices=[[2, 4]], init_latents=init, seed=21)
        convofusion_amd.install(model)
        steered_ref, _ = diffusion_reverse(model, mems, None, masks, focus_indices=[[2, 4]], init_latents=init, seed=21)
        assert torch.isfinite(steered).all() and (steered - steered_ref).norm() / steered_ref.norm() > 1e-3
        convofusion_amd.install(model, modality_weights=REF)
        again, _ = diffusion_reverse(model, mems, None, masks, focus_indices=[[2, 4]], init_latents=init, seed=21)
        assert torch.equal(again, steered_ref)          # the reference's weights, explicitly: the default path's latents
    convofusion_amd.uninstall(model)


def test_abi_refusals():
    """cfd_sample_begin_weighted refuses a NULL table, a NaN entry and a guidance batch of other than 7 chunks with CFD_E_ARG."""
    import torch
    from convofusion_amd import _lib
    from convofusion_amd.sampler import SamplingRun, modality_weight_table
    from tests.gpu_helpers import hip_denoiser
    B, L, n = 1, 16, 10
    mems, masks = _small(B, 4)
    run = SamplingRun(hip_denoiser(1234, 1.0), _sched("ddpm"), mems, masks, B, L, n, guidance_scale=7.5, seed=1)
    run.close()
    lib = _lib.load()
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    table = modality_weight_table(REF, 7.5, n, B)
    nan = table.copy()
    nan[3, 0, 2] = np.nan
    g_eval = C.c_int(-7)
    for what, tab, G in (("NULL table", None, 7), ("NaN", nan, 7), ("G = 1", table, 1), ("G = 6", table, 6)):
        a = _lib.SampleArgs.from_buffer_copy(run._args)
        a.G = G
        ptr = tab.ctypes.data_as(C.c_void_p) if tab is not None else None
        rc = lib.cfd_sample_begin_weighted(run.handle, C.byref(a), ptr, 1, C.byref(g_eval), stream)
        print(what, "->", rc, lib.cfd_last_error().decode())
        assert rc == -1 and g_eval.value == -7, what
    with pytest.raises(ValueError):     # the Python layer refuses first
        SamplingRun(hip_denoiser(1234, 1.0), _sched("ddpm"), mems, masks, B, L, n, guidance_scale=7.5, seed=1, modality_weights=nan[:, :, 1:7])
    # a good table still opens a run on the same handle afterwards
    a = _lib.SampleArgs.from_buffer_copy(run._args)
    assert lib.cfd_sample_begin_weighted(run.handle, C.byref(a), table.ctypes.data_as(C.c_void_p), 1, C.byref(g_eval), stream) == 0
    assert g_eval.value == 6
    out = torch.empty((B, L, 128), device="cuda")
    assert lib.cfd_sample_steps(run.handle, n) == 0 and lib.cfd_sample_read(run.handle, C.c_void_p(out.data_ptr()), 1) == 0
    assert torch.isfinite(out).all()
