"""Host-side checks of the edit-friendly DDPM inversion (no GPU): the restated pair (tests/ddpm_inversion_ref) closes on a toy denoiser,
the ring slot convention, noise[N - 1] == 0, the argument refusals of ``invert_ddpm`` / ``sample(noise_space=)``, and the struct layout
and exported symbols of the new header entries.  test_restated_pair_closes and test_ring_convention_and_last_noise_row check the
restatement itself (tests/ddpm_inversion_ref.py on oracle/ alone): they do not touch the library and so do not depend on the feature
being built; the other two tests, and every test of tests/test_gpu_ddpm_inversion.py, fail without it."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from oracle.scheduler_ref import DDPMSchedulerRef
from tests import ddpm_inversion_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "cfdenoise.h")


def _toy(x, t, enc, masks):
    """A smooth, chunk-dependent stand-in for the denoiser on the 7-chunk batch."""
    x = np.asarray(x, np.float32)
    k = np.repeat(np.arange(7, dtype=np.float32), x.shape[0] // 7).reshape(-1, 1, 1)
    return (np.tanh(0.7 * x + 0.01 * k) * np.float32(0.5 + t / 2000.0)).astype(np.float32), None


def _space(N=20, B=2, L=4, clip=True, seed=0):
    rng = np.random.default_rng(seed)
    source = (0.5 * rng.standard_normal((B, L, 128))).astype(np.float32)
    eps = rng.standard_normal((N, B, L, 128)).astype(np.float32)
    traj, noise = ref.invert(_toy, DDPMSchedulerRef(clip_sample=clip), None, None, source, eps, N, guidance_scale=1.5)
    return source, eps, traj, noise


@pytest.mark.parametrize("clip", [True, False])
def test_restated_pair_closes(clip):
    """The replay under the same conditioning is trajectory[N - i] entering every iteration i <= N - 1, to float32 rounding; with other
    step noise it is nowhere near."""
    N = 20
    source, eps, traj, noise = _space(N, clip=clip)
    keep_steps = tuple(range(1, N + 1))
    _, snaps = ref.replay(_toy, DDPMSchedulerRef(clip_sample=clip), None, None, traj, noise, N, guidance_scale=1.5, keep_steps=keep_steps)
    for done in range(1, N):          # after `done` iterations the latents enter iteration `done`: slot N - done
        assert ref.rel_l2(snaps[done], traj[N - done]) < 5e-6, done
    other = np.random.default_rng(1).standard_normal(noise.shape).astype(np.float32)
    _, far = ref.replay(_toy, DDPMSchedulerRef(clip_sample=clip), None, None, traj, noise, N, guidance_scale=1.5, keep_steps=(N - 1,),
                        step_noise=other)
    assert ref.rel_l2(far[N - 1], traj[1]) > 100 * ref.rel_l2(snaps[N - 1], traj[1])


def test_ring_convention_and_last_noise_row():
    N = 10
    source, eps, traj, noise = _space(N)
    s = DDPMSchedulerRef(clip_sample=True)
    s.set_timesteps(N)
    assert traj.shape == (N + 1, 2, 4, 128) and noise.shape == (N, 2, 4, 128)
    assert np.array_equal(traj[0], source)
    for i, t in enumerate(s.timesteps):      # slot N - i: the level entering iteration i; slot N the noisiest
        assert np.array_equal(traj[N - i], ref.level(s, int(t), source, eps[i]))
    assert int(s.timesteps[-1]) == 0 and not noise[N - 1].any() and noise[:N - 1].any(axis=(1, 2, 3)).all()
    # a kept token of the replay is the ring's value at every level, and k0 > 0 starts from slot N - k0
    keep = np.zeros((2, 4), bool)
    keep[0, 1] = True
    out, snaps = ref.replay(_toy, DDPMSchedulerRef(clip_sample=True), None, None, traj, noise, N, keep=keep, first_iteration=3,
                            guidance_scale=4.0, keep_steps=(4,))
    x = traj[N - 3].copy()
    eps_hat, _ = _toy(np.concatenate([x] * 7), int(s.timesteps[3]), None, None)
    from oracle.sampler_ref import cfg_combine
    want = s.step(cfg_combine(eps_hat, 4.0), int(s.timesteps[3]), x, noise=noise[3])
    assert np.array_equal(snaps[4], want)


def test_python_refusals():
    import torch
    from convofusion_amd import sampler, scheduler
    N, B, L = 20, 2, 16
    traj, noise = torch.zeros((N + 1, B, L, 128)), torch.zeros((N, B, L, 128))
    ok = dict(noise_space=(traj, noise), keep_mask=None, strength=1.0, B=B, L=L, N=N)
    t, z, keep, k0 = sampler.check_noise_space(**ok)
    assert k0 == 0 and keep is None and t.shape[0] == N + 1 and z.shape[0] == N
    assert sampler.check_noise_space(**dict(ok, strength=0.5))[3] == N - 10
    src = torch.zeros((B, L, 128))
    for bad in (dict(scheduler_kind=1), dict(scheduler_kind=3), dict(preseq=src), dict(source_latents=src), dict(anchor_trajectory=traj),
                dict(tie=torch.zeros((B, L), dtype=torch.int32)), dict(dynamic_memories=(0,)), dict(noise_space=(traj[1:], noise)),
                dict(noise_space=(traj, noise[:, :1])), dict(noise_space=traj), dict(noise_space=(traj.long(), noise)),
                dict(keep_mask=torch.full((B, L), 2)), dict(keep_mask=torch.zeros((B, L + 1), dtype=torch.bool)), dict(strength=0.0),
                dict(strength=1.5), dict(strength=0.01)):
        with pytest.raises(ValueError):
            sampler.check_noise_space(**dict(ok, **bad))
    assert "noise_space" in sampler.sample.__kwdefaults__ and sampler.LEVEL_NOISE_STREAM == 2
    sig = list(__import__("inspect").signature(sampler.invert_ddpm).parameters)
    assert sig[:4] == ["denoiser", "scheduler", "enc", "masks"]
    for name in ("source_latents", "num_inference_steps", "guidance_scale", "modality_weights", "seed", "level_noise", "levels_per_batch"):
        assert name in sig
    den = object.__new__(__import__("convofusion_amd.denoiser", fromlist=["Denoiser"]).Denoiser)
    ddpm = scheduler.DDPMScheduler(num_train_timesteps=1000, beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear")
    ddim = scheduler.DDIMScheduler(num_train_timesteps=1000, beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear")
    enc = [torch.zeros((7 * B, 3, 512))] * 5
    with pytest.raises(TypeError):
        sampler.invert_ddpm(object(), ddpm, enc, source_latents=src)
    with pytest.raises(TypeError):
        sampler.invert_ddpm(den, ddim, enc, source_latents=src)
    for bad in (dict(source_latents=src[0]), dict(source_latents=src.long()), dict(source_latents=src, levels_per_batch=0),
                dict(source_latents=src, levels_per_batch=2.5), dict(source_latents=src, level_noise=noise[:, :1]),
                dict(source_latents=src, modality_weights=dict(text=float("inf"))), dict(source_latents=src, modality_weights=dict(nope=1.0))):
        with pytest.raises(ValueError):
            sampler.invert_ddpm(den, ddpm, enc, num_inference_steps=N, **bad)
    with pytest.raises(RuntimeError):      # (no CPU fallback)
        sampler.invert_ddpm(den, ddpm, enc, source_latents=src, num_inference_steps=N)
    from convofusion_amd import edit
    with pytest.raises(ValueError):
        edit.reperform_motion(None, None, None, None, None, method="dpm")


def _struct_fields(text, name):
    end = text.index("} " + name + ";")
    body = text[text.rindex("typedef struct {", 0, end) + len("typedef struct {"):end]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    return [re.sub(r"\[.*\]", "", d.split()[-1].lstrip("*")) for d in body.split(";") if d.strip()]


def test_header_entries_and_struct_layout():
    from convofusion_amd import _lib
    text = open(HEADER).read()
    for sym in ("cfd_ddpm_invert", "cfd_sample_begin_replay"):
        assert sym in _lib.SYMBOLS and re.search(r"\bint " + sym + r"\(", text)
    assert _struct_fields(text, "cfd_ddpm_invert_args") == [f for f, _ in _lib.DdpmInvertArgs._fields_]
    assert _struct_fields(text, "cfd_replay_args") == [f for f, _ in _lib.ReplayArgs._fields_]
    # natural alignment on LP64: pointers 8, ints 4, size_t 8
    assert C.sizeof(_lib.DdpmInvertArgs) == 64 and _lib.DdpmInvertArgs.levels_per_batch.offset == 48
    assert _lib.DdpmInvertArgs.workspace_bytes.offset == 56 and _lib.DdpmInvertArgs.level_noise.offset == 24
    assert C.sizeof(_lib.ReplayArgs) == 48 and _lib.ReplayArgs.keep.offset == 32 and _lib.ReplayArgs.first_iteration.offset == 40
    lib_path = _lib.LIB_PATH
    if os.path.exists(lib_path):       # the built library exports them (the build is the clean checkout's first step)
        blob = open(lib_path, "rb").read()
        assert b"cfd_ddpm_invert" in blob and b"cfd_sample_begin_replay" in blob
