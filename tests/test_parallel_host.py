"""Host-side checks of parallel-in-time DDPM sampling (no GPU): the restated sweep / scan / slide loop (tests/parallel_ref) reproduces the
sequential DDPM loop bit for bit at tolerance 0, its bookkeeping (strides, sweeps, the ring convention), the stride rule -- restated and
the library's own (cfd_test_picard_stride: no device needed) on hand-made arrays --, the argument refusals of ``sample_parallel`` and
the struct layout and exported symbols of the new header entries.  The module imports the feature: every test fails without it."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from convofusion_amd import _lib
from convofusion_amd.sampler import ParallelStats, sample_parallel
from oracle.scheduler_ref import DDPMSchedulerRef
from tests import parallel_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "cfdenoise.h")
HEADER_DEV = os.path.join(ROOT, "include", "cfdenoise_dev.h")
assert _lib.ParallelArgs is not None and ParallelStats is not None and callable(sample_parallel)


def _toy(x, t, enc, masks):
    """A fixed nonlinear, chunk- and timestep-dependent stand-in for the denoiser on the 7-chunk batch."""
    x = np.asarray(x, np.float32)
    k = np.repeat(np.arange(7, dtype=np.float32), x.shape[0] // 7).reshape(-1, 1, 1)
    return (np.tanh(0.7 * x + 0.01 * k) * np.float32(0.5 + t / 2000.0) + np.float32(0.1) * np.sin(3.0 * x).astype(np.float32)).astype(np.float32), None


def _draws(N, B=2, L=4, seed=0):
    rng = np.random.default_rng(seed)
    return rng.standard_normal((B, L, 128)).astype(np.float32), rng.standard_normal((N, B, L, 128)).astype(np.float32)


@pytest.mark.parametrize("clip", [True, False])
@pytest.mark.parametrize("N", [10, 20])
def test_tolerance_zero_is_the_sequential_chain(N, clip):
    """tau = 0: the final latents and EVERY trajectory slot np.array_equal the sequential loop's, for J in {1, 3, N} (N no multiple of 3);
    the strides sum to N and there are at most N sweeps."""
    init, noise = _draws(N)
    eps_fn = ref.guided(_toy, guidance_scale=2.0)
    want = ref.sequential(eps_fn, DDPMSchedulerRef(clip_sample=clip), init, noise, N)
    assert want.shape == (N + 1, 2, 4, 128) and np.array_equal(want[N], init)
    for J in (1, 3, N):
        lat, traj, strides = ref.sample_parallel(eps_fn, DDPMSchedulerRef(clip_sample=clip), init, noise, N, J, 0.0)
        assert np.array_equal(lat, want[0]) and np.array_equal(traj, want), J
        assert sum(strides) == N and len(strides) <= N and min(strides) >= 1 and max(strides) <= J, (J, strides)
        if J == 1:
            assert strides == [1] * N


def test_one_level_per_batch_ignores_the_tolerance():
    N = 10
    init, noise = _draws(N, seed=3)
    eps_fn = ref.guided(_toy, guidance_scale=2.0)
    outs = [ref.sample_parallel(eps_fn, DDPMSchedulerRef(), init, noise, N, 1, tau) for tau in (0.0, 0.1, 1e9)]
    for lat, traj, strides in outs[1:]:
        assert np.array_equal(lat, outs[0][0]) and np.array_equal(traj, outs[0][1]) and strides == [1] * N


def test_a_tolerance_trades_sweeps_for_error():
    """tau > 0: fewer sweeps than tau = 0 needs, strides that still sum to N, a finite result near the sequential one; a huge tau passes
    every window in one sweep; max_sweeps is honoured."""
    N, J = 20, 6
    init, noise = _draws(N, seed=5)
    eps_fn = ref.guided(_toy, guidance_scale=2.0)
    want = ref.sequential(eps_fn, DDPMSchedulerRef(), init, noise, N)[0]
    exact = ref.sample_parallel(eps_fn, DDPMSchedulerRef(), init, noise, N, J, 0.0)
    loose = ref.sample_parallel(eps_fn, DDPMSchedulerRef(), init, noise, N, J, 0.5)
    huge = ref.sample_parallel(eps_fn, DDPMSchedulerRef(), init, noise, N, J, 1e9)
    assert sum(loose[2]) == N and sum(huge[2]) == N and len(huge[2]) == -(-N // J) and len(loose[2]) <= len(exact[2]) <= N
    assert np.isfinite(loose[0]).all() and np.linalg.norm(loose[0] - want) < 0.5 * np.linalg.norm(want)
    with pytest.raises(RuntimeError):
        ref.sample_parallel(eps_fn, DDPMSchedulerRef(), init, noise, N, J, 0.0, max_sweeps=2)


def _lib_stride(err, p, i0, sched, ts, tau, L):
    lib = _lib.load()
    coef = np.zeros((len(ts), 8), np.float32)
    for i, t in enumerate(ts):
        sb, sa, c0, cx, sigma = sched.coefficients(int(t))
        coef[i] = (sb, sa, c0, cx, sigma, 1.0 if int(t) > 0 else 0.0, 0.0, 0.0)
    err = np.ascontiguousarray(err, np.float32)
    return lib.cfd_test_picard_stride(C.c_void_p(err.ctypes.data), err.shape[1], p, i0, C.c_void_p(coef.ctypes.data), len(ts), float(tau), L)


def test_stride_rule():
    """Hand-made error arrays, through the restated rule and the library's: the first window position over its bound stops the window;
    the worst utterance decides; row 0 (the final first level) is never read; the last iteration (t = 0, no noise) is judged against the
    variance of the iteration before it; tau = 0 passes exact zeros only; a NaN stops."""
    N, L, B = 10, 4, 2
    sched = DDPMSchedulerRef()
    sched.set_timesteps(N)
    ts = [int(t) for t in sched.timesteps]
    v = ref.variances(sched, ts)
    assert ts[-1] == 0 and v[N - 1] == v[N - 2] > 0 and sched.coefficients(0)[4] == 0
    n_el = L * 128
    tau = 0.1

    def both(err, p, i0, tau=tau):
        a, b = ref.stride(err, p, i0, v, tau, n_el), _lib_stride(err, p, i0, sched, ts, tau, L)
        assert a == b, (a, b)
        return a

    def at(i, f):          # a squared change f times the bound of the latent X(i)
        return np.float32(f * tau * tau * float(v[i]) * n_el)

    p, i0 = 5, 2
    err = np.zeros((p, B), np.float32)
    assert both(err, p, i0) == p                                    # nothing moved: the whole window
    err[0] = 1e30
    assert both(err, p, i0) == p                                    # row 0 is not read
    err[3] = [at(i0 + 3, 0.5), at(i0 + 3, 2.0)]
    assert both(err, p, i0) == 3                                    # the worst utterance decides
    err[3] = [at(i0 + 3, 0.5), at(i0 + 3, 0.9)]
    assert both(err, p, i0) == p
    err[1, 0] = at(i0 + 1, 1.5)
    assert both(err, p, i0) == 1                                    # the first position over its bound
    err[1, 0] = np.nan
    assert both(err, p, i0) == 1
    err[:] = 0
    err[2, 1] = 1e-30
    assert both(err, p, i0, tau=0.0) == 2 and both(np.zeros_like(err), p, i0, tau=0.0) == p
    # the window that ends at the table's end: position k = 2 is the latent entering the no-noise iteration N - 1
    p, i0 = 3, N - 3
    err = np.zeros((p, B), np.float32)
    err[2] = at(N - 2, 0.9)
    assert both(err, p, i0) == 3
    err[2] = at(N - 2, 1.1)
    assert both(err, p, i0) == 2
    assert both(np.zeros((1, B), np.float32), 1, N - 1) == 1        # one level left
    assert _lib_stride(np.zeros((4, B), np.float32), 4, N - 3, sched, ts, tau, L) == -1     # a window beyond the table: CFD_E_ARG


def test_python_refusals():
    import inspect

    import torch
    from convofusion_amd import sampler, scheduler
    sig = inspect.signature(sampler.sample_parallel).parameters
    assert list(sig)[:4] == ["denoiser", "scheduler", "enc", "masks"]
    for name, default in (("L", 16), ("num_inference_steps", 1000), ("tolerance", 0.1), ("levels_per_batch", None), ("workspace_bytes", None),
                          ("modality_weights", None), ("init_latents", None), ("step_noise", None), ("trajectory", False), ("max_sweeps", None)):
        assert sig[name].kind is inspect.Parameter.KEYWORD_ONLY and sig[name].default == default, name
    N, B, L = 20, 2, 16
    den = object.__new__(__import__("convofusion_amd.denoiser", fromlist=["Denoiser"]).Denoiser)
    kw = dict(num_train_timesteps=1000, beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear")
    ddpm, ddim = scheduler.DDPMScheduler(**kw), scheduler.DDIMScheduler(**kw)
    enc = [torch.zeros((7 * B, 3, 512))] * 5
    with pytest.raises(TypeError):
        sampler.sample_parallel(object(), ddpm, enc, B=B)
    for other in (ddim, scheduler.DPMSolverMultistepScheduler(**kw), object()):
        with pytest.raises(TypeError):
            sampler.sample_parallel(den, other, enc, B=B)
    lat, z = torch.zeros((B, L, 128)), torch.zeros((N, B, L, 128))
    for bad in (dict(tolerance=-0.1), dict(tolerance=float("nan")), dict(tolerance=float("inf")), dict(tolerance="x"), dict(tolerance=None),
                dict(levels_per_batch=0), dict(levels_per_batch=2.5), dict(levels_per_batch=-3), dict(max_sweeps=0), dict(max_sweeps=1.5),
                dict(init_latents=lat[0]), dict(init_latents=lat.long()), dict(init_latents=lat[:, :8]), dict(step_noise=z[1:]),
                dict(step_noise=z[:, :1]), dict(step_noise=lat), dict(modality_weights=dict(text=float("inf"))),
                dict(modality_weights=dict(nope=1.0)), dict(B=0), dict(L=0)):
        with pytest.raises(ValueError):
            sampler.sample_parallel(den, ddpm, enc, **dict(dict(B=B, L=L, num_inference_steps=N), **bad))
    with pytest.raises(RuntimeError):      # (no CPU fallback)
        sampler.sample_parallel(den, ddpm, enc, B=B, L=L, num_inference_steps=N, init_latents=lat, step_noise=z)
    st = sampler.ParallelStats(3, [4, 4, 2], 4, 6)
    assert (st.sweeps, st.strides, st.levels_per_batch, st.chunks_evaluated) == (3, [4, 4, 2], 4, 6) and "sweeps=3" in repr(st)


def _struct_fields(text, name):
    end = text.index("} " + name + ";")
    body = text[text.rindex("typedef struct {", 0, end) + len("typedef struct {"):end]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    return [re.sub(r"\[.*\]", "", d.split()[-1].lstrip("*")) for d in body.split(";") if d.strip()]


def test_header_entries_and_struct_layout():
    text = open(HEADER).read()
    assert "cfd_sample_parallel" in _lib.SYMBOLS and re.search(r"\bint cfd_sample_parallel\(", text)
    assert "cfd_test_picard_stride" in _lib.SYMBOLS and re.search(r"\bint cfd_test_picard_stride\(", open(HEADER_DEV).read())
    assert _struct_fields(text, "cfd_parallel_args") == [f for f, _ in _lib.ParallelArgs._fields_]
    assert _struct_fields(text, "cfd_parallel_stats") == [f for f, _ in _lib.ParallelStats._fields_]
    # natural alignment on LP64: pointers 8, ints and floats 4, size_t 8
    P, S = _lib.ParallelArgs, _lib.ParallelStats
    assert C.sizeof(P) == 56 and (P.weights.offset, P.prune.offset, P.tolerance.offset, P.levels_per_batch.offset) == (0, 8, 12, 16)
    assert (P.workspace_bytes.offset, P.max_sweeps.offset, P.latents.offset, P.trajectory.offset) == (24, 32, 40, 48)
    assert C.sizeof(S) == 32 and (S.sweeps.offset, S.strides.offset, S.strides_capacity.offset) == (8, 16, 24)
    # the sweep-kernel hook: one declaration per field in the header, in the binding's order; enum values; LP64 offsets
    dev = open(HEADER_DEV).read()
    T = _lib.TestPicardArgs
    assert "cfd_test_picard_sweep" in _lib.SYMBOLS and re.search(r"\bint cfd_test_picard_sweep\(cfd_handle h, const cfd_test_picard_args\* args,", dev)
    assert _struct_fields(dev, "cfd_test_picard_args") == [f for f, _ in T._fields_]
    for name, val in (("FILL", 1), ("LOAD", 2), ("STEP", 4), ("SCAN", 8)):
        assert re.search(r"\bCFD_PICARD_%s = %d\b" % (name, val), dev) and getattr(_lib, "PICARD_" + name) == val
    assert [getattr(T, f).offset for f, _ in T._fields_] == [0, 4, 8, 12, 16, 20, 24, 28, 32, 40, 48, 52, 56, 64, 72, 80, 88, 92, 124, 156, 160,
                                                            168, 176, 184, 192, 200] and C.sizeof(T) == 208
    assert (T.pos.size, T.w.size, T.seed.size, T.first_utterance.size) == (32, 32, 8, 4)
    blob = open(_lib.LIB_PATH, "rb").read()      # the built library exports them, with the kernels of a sweep
    for name in (b"cfd_sample_parallel", b"cfd_test_picard_stride", b"cfd_test_picard_sweep", b"picard_load_kernel", b"picard_step_kernel", b"picard_scan_kernel",
                 b"picard_err_kernel", b"picard_fill_kernel"):
        assert name in blob, name
